"""TEST INFRASTRUCTURE: the host-side helpers every test module shares: the bit-for-bit comparer, the
cameras, frames and synthetic planes that more than one module builds, and the reason census.

    from support import assert_bits, assert_all_bits, words

Everything here is host data: nothing touches the GPU except frame_planes(), which makes the public
synchronous calls its caller used to make itself. Device objects (scenes, sessions, tensors) stay in
the modules that own them; tests/tools/device_io.py holds the helpers that need torch or the HIP
runtime.
"""
import functools
import math

import numpy as np

import raytracinginoneweekend_amd as rt

F = np.float32
POS, LOOK = (-4.0, 3.2, 5.0), (0.0, 1.0, 0.0)  # the default camera's position and look-at point
STEP_DEG = 1.5                                   # the preview orbit's step per frame
STILL = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))       # no shift of (position, look-at point)
TEMPORAL_OUTPUTS = ("color", "variance", "history")


# ---- bit for bit ---------------------------------------------------------------------------------------
def words(a):
    """The contiguous array's own bytes as words: uint32 for a 4-byte dtype, uint8 for a 1-byte dtype.
    Any other item size raises TypeError. The values are never converted."""
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize == 4:
        return a.view(np.uint32)
    if a.dtype.itemsize == 1:
        return a.view(np.uint8)
    raise TypeError(f"words(): {a.dtype} has neither 4-byte nor 1-byte items")


def _difference(got, ref):
    """None where got is ref bit for bit, else what differs: the shapes, the dtypes, or the word count."""
    if got.shape != ref.shape:
        return f"shape {got.shape} against {ref.shape}"
    if got.dtype != ref.dtype:
        return f"dtype {got.dtype} against {ref.dtype}"
    bad = int(np.count_nonzero(words(got) != words(ref)))
    return f"{bad} of {words(ref).size} words differ" if bad else None


def assert_bits(got, ref, what=""):
    """The suite's one meaning of "bit for bit": got.shape == ref.shape, got.dtype == ref.dtype and
    zero differing words (signed zeros and NaN payloads count). Neither side is converted: where a
    reference comes in another dtype, the call site converts the reference and says why. Prints the
    result, so `pytest -s` keeps a census; names `what` in the failure."""
    d = _difference(got, ref)
    print(f"{what}: {d or '0 of %d words differ' % words(ref).size}")
    assert d is None, f"{what}: {d}"


def assert_all_bits(got, ref, what="", names=None):
    """assert_bits over planes: two dicts (names: the keys compared, every key of ref if None) or two
    sequences (names: one per position, the temporal stage's three outputs if None). Every plane is
    compared before anything is asserted, so a failure reports each plane's difference."""
    if isinstance(ref, dict):
        names = tuple(ref) if names is None else names
        pairs = [(n, got[n], ref[n]) for n in names]
    else:
        names = TEMPORAL_OUTPUTS if names is None else names
        assert len(got) == len(ref) == len(names), (what, len(got), len(ref), names)
        pairs = list(zip(names, got, ref))
    report = {n: _difference(g, r) for n, g, r in pairs}
    print(f"{what}: differences per plane: {report}")
    assert not any(report.values()), f"{what}: {report}"


# ---- cameras -------------------------------------------------------------------------------------------
def camera_at(w, h, pos=POS, look=LOOK, mode=rt.CORRECTED):
    """The default camera's lens (42 degrees, aperture 0.0625, up = y) for a w x h image, standing at
    pos and focused on look: the focus distance is their float32 distance."""
    focus = float(np.float32(np.linalg.norm(np.subtract(pos, look).astype(F))))
    return rt.Camera(pos, look, (0, 1, 0), w / h, 42.0, 0.0625, focus, mode)


@functools.lru_cache(maxsize=None)
def shifted_camera(w, h, mode=rt.CORRECTED, shift=STILL, view=(POS, LOOK)):
    """camera_at with view's position and look-at point shifted by shift[0] and shift[1]."""
    return camera_at(w, h, tuple(np.add(view[0], shift[0])), tuple(np.add(view[1], shift[1])), mode)


@functools.lru_cache(maxsize=None)
def orbit_camera(w, h, i, step_deg=STEP_DEG, pos=POS, look=LOOK, mode=rt.CORRECTED):
    """Frame i's camera: the one at pos turned by i steps around the vertical axis through look."""
    a = math.radians(i * step_deg)
    dx, dz = pos[0] - look[0], pos[2] - look[2]
    turned = (look[0] + dx * math.cos(a) + dz * math.sin(a), pos[1], look[2] - dx * math.sin(a) + dz * math.cos(a))
    return camera_at(w, h, turned, look, mode)


# ---- planes --------------------------------------------------------------------------------------------
def frozen(planes):
    """The dict of arrays with every array made read-only (shared references stay as computed)."""
    for a in planes.values():
        a.setflags(write=False)
    return planes


def frame_planes(records, params, camera, aov_samples=0, aov_planes=None):
    """A frame's planes from the public synchronous calls, read-only: beauty and variance
    (rt.render_var) and the feature buffers of samples 0..aov_samples-1 (rt.render_aov; 0: every
    sample; aov_planes: those planes only)."""
    beauty, variance, _ = rt.render_var(records, params, camera)
    which = () if aov_planes is None else (tuple(aov_planes),)
    return frozen(dict(beauty=beauty, variance=variance, **rt.render_aov(records, params, camera, aov_samples, *which)))


def synthetic_planes(w, h, block=False, variance_scale=None, seed=None):
    """Seeded random planes (seed: w * 1000 + h if None), read-only: beauty in [0, 1), unit normals,
    depth in [0, 4), albedo in [0, 1) and, with a variance_scale, variance in [0, variance_scale).
    block: the left half carries one colour, sky-like guides (normal 0, depth 0, one albedo) and a
    variance of 0."""
    g = np.random.default_rng(w * 1000 + h if seed is None else seed)
    beauty = g.random((h, w, 3), dtype=np.float32)
    n = g.standard_normal((h, w, 3)).astype(np.float32)
    normal = (n / np.sqrt((n * n).sum(-1, keepdims=True))).astype(np.float32)
    depth = (g.random((h, w), dtype=np.float32) * F(4)).astype(np.float32)
    planes = dict(beauty=beauty, albedo=g.random((h, w, 3), dtype=np.float32), normal=normal, depth=depth)
    if variance_scale is not None:
        planes["variance"] = (g.random((h, w), dtype=np.float32) * F(variance_scale)).astype(np.float32)
    if block:
        half = w // 2
        beauty[:, :half] = (F(0.25), F(0.5), F(0.75))
        planes["albedo"][:, :half] = (F(0.5), F(0.625), F(0.75))
        for name in set(planes) - {"beauty", "albedo"}:
            planes[name][:, :half] = 0
    return frozen(planes)


def census(reason, reasons):
    """How many pixels carry each reason code: {name: count} over reasons (code -> name), printed."""
    c = {name: int((reason == k).sum()) for k, name in reasons.items()}
    print("reasons:", c)
    return c
