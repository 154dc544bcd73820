"""The temporal stage's history clamp without a GPU (rt_temporal_clip*, rt_preview_set_clip, DESIGN.md
§4.17): the record and its defaults, every argument check (all made before any device call, the
underlying stage's first), properties of the numpy restatement (tests/tools/temporal_clip_ref.py), and
the conditions that make the GPU module's synthetic cases (tests/tools/clip_cases.py) say something.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import clip_cases  # noqa: E402
import temporal_clip_ref as R  # noqa: E402
import temporal_motion_ref  # noqa: E402
import temporal_ref  # noqa: E402
from support import assert_bits, words as u32  # noqa: E402

F = np.float32


# ---- the record --------------------------------------------------------------------------------------
W0, H0 = 6, 4
_HOST = {n: np.zeros((H0, W0, 3) if ch == 3 else (H0, W0), dtype=dt) for n, (ch, dt) in abi.TEMPORAL_PLANES.items()}
_TABLES = np.zeros((2, 4, 4), dtype=F)
PREV = tuple(n for n in abi.TEMPORAL_PLANES if n.startswith("prev_"))
OUT = tuple(n for n in abi.TEMPORAL_PLANES if n.startswith("out_"))
CUR = tuple(n for n in abi.TEMPORAL_PLANES if n not in PREV + OUT)
DEFAULT = object()


def _degenerate():
    c = abi.RtCamera.from_buffer_copy(bytes(rt.Camera.default(W0, H0).c))
    c.vertical[:] = (0.0, 1.0, 0.0)
    c.horizontal[:] = (0.0, 2.0, 0.0)
    return c


def _call(device, drop=(), alias=None, params_size=None, buffers_size=None, camera=True, prev_camera=True, raw=None,
          clip=DEFAULT, clip_raw=None, motion=None, **fields):
    """The status and message of rt_temporal_clip (host) or rt_temporal_clip_device with host addresses,
    which a call that fails its checks never touches. clip: a record, None (a null pointer) or the
    default one with clip_raw's fields set; motion: None or a dict of rt_temporal_motion_t fields."""
    p = rt.temporal_params(W0, H0, **fields)
    for k, v in (raw or {}).items():
        setattr(p, k, v)
    if params_size is not None:
        p.size = params_size
    ptr = {n: a.ctypes.data for n, a in _HOST.items() if n not in drop}
    for a, b in (alias or {}).items():
        ptr[a] = ptr[b]
    rec = rt.temporal_buffers(ptr)
    if buffers_size is not None:
        rec.size = buffers_size
    cam = C.byref(rt.Camera.default(W0, H0).c) if camera else None
    prev = None if not prev_camera else C.byref(prev_camera if prev_camera is not True else rt.Camera.default(W0, H0).c)
    if clip is DEFAULT:
        clip = rt.temporal_clip()
        for k, v in (clip_raw or {}).items():
            setattr(clip, k, v)
    m = None
    if motion is not None:
        m = abi.RtTemporalMotion(C.sizeof(abi.RtTemporalMotion), 4, _TABLES[0].ctypes.data, _TABLES[1].ctypes.data)
        for k, v in motion.items():
            setattr(m, k, v)
    L = rt.lib()
    f = L.rt_temporal_clip_device if device else L.rt_temporal_clip
    rc = f(C.byref(p), cam, prev, C.byref(rec), C.byref(m) if m is not None else None,
           C.byref(clip) if clip is not None else None, None)
    return rc, L.rt_last_error().decode()


def test_record_and_default():
    assert C.sizeof(abi.RtTemporalClip) == 16
    assert [n for n, _ in abi.RtTemporalClip._fields_] == ["size", "radius", "gamma", "flags"]
    L = rt.lib()
    c = abi.RtTemporalClip()
    assert L.rt_temporal_clip_default(C.byref(c)) == abi.RT_OK
    assert c.size == 16 and c.flags == 0 and 1 <= c.radius <= 3 and np.isfinite(c.gamma) and c.gamma >= 0
    assert L.rt_temporal_clip_default(None) == abi.RT_ERR_INVALID
    # the default record passes its own checks (RT_ERR_DEVICE without a GPU: the checks all passed), with
    # and without motion tables
    for motion in (None, {}):
        rc, msg = _call(False, clip=c, motion=motion)
        assert rc != abi.RT_ERR_INVALID, msg
    q = rt.temporal_clip(radius=3, gamma=2.5)
    assert (q.size, q.radius, q.gamma, q.flags) == (16, 3, 2.5, 0)
    assert rt.temporal_clip(gamma=0.0).radius == c.radius
    with pytest.raises(KeyError):
        rt.temporal_clip(sigma=1.0)


# ---- argument checks -----------------------------------------------------------------------------------
# the underlying stage's checks: test_temporal_cpu.py's list, restated
STAGE_BAD = [
    ("params.size", dict(params_size=28)),
    ("buffers.size", dict(buffers_size=120)),
    ("width", dict(raw=dict(width=0))),
    ("width", dict(raw=dict(width=65537))),
    ("height", dict(raw=dict(height=0))),
    ("height", dict(raw=dict(height=65537))),
    ("alpha_min", dict(alpha_min=0.0)),
    ("alpha_min", dict(alpha_min=1.5)),
    ("alpha_min", dict(alpha_min=float("nan"))),
    ("max_history", dict(max_history=0.5)),
    ("max_history", dict(max_history=float("inf"))),
    ("normal_tol", dict(normal_tol=-1e-3)),
    ("normal_tol", dict(normal_tol=float("nan"))),
    ("depth_tol", dict(depth_tol=-1.0)),
    ("depth_tol", dict(depth_tol=float("inf"))),
    ("flags", dict(flags=1)),
    ("camera", dict(camera=False)),
    ("prev_camera", dict(prev_camera=False)),
    ("prev_camera", dict(prev_camera=_degenerate())),
] + [(n, dict(drop=(n,))) for n in CUR + OUT + PREV] + [
    ("prev_", dict(drop=PREV[1:])),
] + [(o, dict(alias={o: i})) for o in OUT for i in CUR + PREV] + [
    ("out_variance", dict(alias={"out_variance": "out_color"})),
    ("out_history", dict(alias={"out_history": "out_color"})),
    ("out_history", dict(alias={"out_history": "out_variance"})),
]
MOTION_BAD = [
    ("motion.size", dict(motion=dict(size=20))),
    ("motion.centres", dict(motion=dict(centres=None))),
    ("motion.prev_centres", dict(motion=dict(prev_centres=None))),
    ("motion.centres", dict(motion=dict(centres=_HOST["out_color"].ctypes.data))),
    ("motion.prev_centres", dict(motion=dict(prev_centres=_HOST["out_history"].ctypes.data))),
]
CLIP_BAD = [
    ("clip is null", dict(clip=None)),
    ("clip.size", dict(clip_raw=dict(size=12))),
    ("clip.size", dict(clip_raw=dict(size=0))),
    ("clip.radius", dict(clip_raw=dict(radius=0))),
    ("clip.radius", dict(clip_raw=dict(radius=4))),
    ("clip.radius", dict(clip_raw=dict(radius=0xffffffff))),
    ("clip.gamma", dict(clip_raw=dict(gamma=-0.5))),
    ("clip.gamma", dict(clip_raw=dict(gamma=float("nan")))),
    ("clip.gamma", dict(clip_raw=dict(gamma=float("inf")))),
    ("clip.flags", dict(clip_raw=dict(flags=1))),
]
BAD = STAGE_BAD + MOTION_BAD + CLIP_BAD + [(f, dict(kw, motion={})) for f, kw in CLIP_BAD]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("field,kw", BAD, ids=[f"{i}-{f.replace(' ', '-')}" for i, (f, _) in enumerate(BAD)])
def test_argument_checks_name_the_field(field, kw, device):
    """RT_ERR_INVALID before any device call (this test runs without a GPU), the field named."""
    rc, msg = _call(device, **kw)
    assert rc == abi.RT_ERR_INVALID, (rc, msg)
    assert field in msg and msg.startswith("rt_temporal_clip_device:" if device else "rt_temporal_clip:"), msg


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_underlying_checks_come_first_and_the_record_is_checked_without_history(device):
    # a bad stage argument and a bad clip record: the stage's field is the one named
    rc, msg = _call(device, alpha_min=0.0, clip_raw=dict(radius=9))
    assert rc == abi.RT_ERR_INVALID and "alpha_min" in msg and "clip" not in msg.split(":", 1)[1], msg
    rc, msg = _call(device, motion=dict(size=20), clip=None)
    assert rc == abi.RT_ERR_INVALID and "motion.size" in msg, msg
    # the prev_ planes NULL: the record is still checked ...
    for field, kw in CLIP_BAD:
        rc, msg = _call(device, drop=PREV, prev_camera=False, **kw)
        assert rc == abi.RT_ERR_INVALID and field in msg, (field, rc, msg)
    # ... and a good one passes (without a GPU only the device is missing; host call: the planes are host memory)
    if not device:
        rc, msg = _call(False, drop=PREV, prev_camera=False)
        assert rc != abi.RT_ERR_INVALID, msg
    # gamma = 0 and -0.0 are in range
    for gamma in (0.0, -0.0):
        if not device:
            rc, msg = _call(False, clip_raw=dict(gamma=gamma))
            assert rc != abi.RT_ERR_INVALID, msg


def test_null_records_and_the_session_call():
    L = rt.lib()
    assert L.rt_temporal_clip(None, None, None, None, None, None, None) == abi.RT_ERR_INVALID
    assert L.rt_temporal_clip_device(None, None, None, None, None, None, None) == abi.RT_ERR_INVALID
    c = rt.temporal_clip()
    assert L.rt_preview_set_clip(None, C.byref(c)) == abi.RT_ERR_INVALID
    assert b"rt_preview_set_clip" in L.rt_last_error()
    assert L.rt_preview_set_clip(None, None) == abi.RT_ERR_INVALID


def test_python_wrapper_passes_the_record():
    cam = rt.Camera.default(W0, H0)
    cur = {n: _HOST[n] for n in CUR}
    bad = rt.temporal_clip()
    bad.radius = 7
    with pytest.raises(rt.RtError) as e:
        rt.temporal(cur, None, cam, None, clip=bad)
    assert e.value.status == abi.RT_ERR_INVALID and "clip.radius" in str(e.value) and "rt_temporal_clip:" in str(e.value)
    with pytest.raises(rt.RtError) as e:
        rt.temporal_device({n: a.ctypes.data for n, a in _HOST.items() if n not in PREV}, rt.temporal_params(W0, H0), cam, None,
                           clip=bad, motion=(_TABLES[0].ctypes.data, _TABLES[1].ctypes.data, 4))
    assert e.value.status == abi.RT_ERR_INVALID and "clip.radius" in str(e.value) and "rt_temporal_clip_device:" in str(e.value)


# ---- properties of the restatement -------------------------------------------------------------------
@pytest.mark.parametrize("radius", clip_cases.RADII)
def test_restatement_without_prev_returns_the_current_frame(radius):
    cur, _, cam, _ = clip_cases.planes(70, 37)
    out = R.accumulate(cur, None, cam, None, clip_cases.params(70, 37), clip_cases.clip(radius))
    assert np.array_equal(u32(out[0]), u32(cur["beauty"])) and np.array_equal(u32(out[1]), u32(cur["variance"]))
    assert (out[2] == 1).all() and (out[3] == R.NO_PREV).all() and out[4] is None


@pytest.mark.parametrize("motion", [False, True], ids=["static", "motion"])
@pytest.mark.parametrize("radius", clip_cases.RADII)
@pytest.mark.parametrize("w,h", clip_cases.SIZES)
def test_restatement_clamps_into_the_box_and_the_cases_say_something(w, h, radius, motion):
    """Every clamped channel lies in [lo, hi]; the blend is the contract's over the clamped colour; and,
    at every size, more than a tenth of the pixels with history have a channel changed by the clamp and
    more than a tenth have none changed (the GPU module asserts the same)."""
    cur, prev, cam, prev_cam = clip_cases.planes(w, h)
    par, clip = clip_cases.params(w, h), clip_cases.clip(radius)
    tabs = clip_cases.tables() if motion else (None, None)
    c, v, n, reason, info = R.accumulate(cur, prev, cam, prev_cam, par, clip, *tabs)
    kept = reason == R.KEPT
    assert (info["lo"] <= info["hi"]).all()
    assert (info["clamped"][kept] >= info["lo"][kept]).all() and (info["clamped"][kept] <= info["hi"][kept]).all()
    inside = (info["resampled"] >= info["lo"]) & (info["resampled"] <= info["hi"])
    assert_bits(info["clamped"][kept & inside.all(axis=2)], info["resampled"][kept & inside.all(axis=2)])
    assert np.array_equal(u32(c[~kept]), u32(cur["beauty"][~kept])) and (n[~kept] == 1).all()
    k = np.fmax(F(1) / n, F(par.alpha_min))
    want = k[..., None] * cur["beauty"] + (F(1) - k)[..., None] * info["clamped"]
    assert_bits(c[kept], want[kept])
    changed, total = int(info["changed"].sum()), int(kept.sum())
    print(f"{w}x{h} radius {radius} motion {motion}: pixels with history {total}, a channel changed on {changed}")
    assert total > w * h // 4
    assert changed > total / 10 and total - changed > total / 10
    # the clamp matters in the output, and the unclamped stage is the older restatements'
    plain = (temporal_motion_ref.accumulate(cur, prev, cam, prev_cam, par, *tabs) if motion
             else temporal_ref.accumulate(cur, prev, cam, prev_cam, par))
    assert np.array_equal(reason, plain[3]) and np.array_equal(u32(v), u32(plain[1])) and np.array_equal(u32(n), u32(plain[2]))
    differ = (u32(c) != u32(plain[0])).any(axis=2)
    assert (differ <= info["changed"]).all() and differ.sum() > total / 10
    if motion and w * h > 100:  # (5 x 3 has 15 pixels: a resized sphere's are counted at the larger sizes)
        assert (reason == R.RESIZED).sum() >= 20


@pytest.mark.parametrize("motion", [False, True], ids=["static", "motion"])
def test_restatement_with_a_wide_box_is_the_unclamped_stage_bit_for_bit(motion):
    """gamma = 1e30 on planes without a flat window: no channel changes, and the whole restatement
    equals temporal_ref / temporal_motion_ref (which share only the camera helpers with it)."""
    w, h = 70, 37
    cur, prev, cam, prev_cam = clip_cases.planes(w, h)
    cur = dict(cur, beauty=np.random.default_rng(3).random((h, w, 3), dtype=F))
    par = clip_cases.params(w, h)
    tabs = clip_cases.tables() if motion else (None, None)
    got = R.accumulate(cur, prev, cam, prev_cam, par, clip_cases.clip(1, gamma=1e30), *tabs)
    plain = (temporal_motion_ref.accumulate(cur, prev, cam, prev_cam, par, *tabs) if motion
             else temporal_ref.accumulate(cur, prev, cam, prev_cam, par))
    lone = np.isin(got[3], (R.KEPT,)) & (got[4]["lo"] == got[4]["hi"]).all(axis=2)
    print("kept pixels alone in their window:", int(lone.sum()))
    for a, b in zip(got[:3], plain[:3]):
        assert np.array_equal(u32(a)[~lone], u32(b)[~lone])
    assert np.array_equal(got[3], plain[3])
    assert (got[3] == R.KEPT).sum() > w * h // 4


def test_a_pixel_alone_in_its_window_takes_its_own_colour():
    """Every pixel carries an id of its own, in both frames, under a static camera: each reprojects onto
    itself, its window holds only itself (n = 1, s2 = 0, lo = hi = b), and C_h becomes b exactly, so
    that the blend is k b + (1 - k) b whatever the history held."""
    w, h = 12, 7
    g = np.random.default_rng(5)
    cam = rt.Camera.default(w, h, rt.CORRECTED)
    normal = np.zeros((h, w, 3), dtype=F)
    normal[..., 1] = 1
    guides = dict(normal=normal, depth=np.full((h, w), F(0.75)), sphere_id=np.arange(w * h, dtype=np.uint32).reshape(h, w))
    cur = dict(beauty=g.random((h, w, 3), dtype=F), variance=g.random((h, w), dtype=F) * F(0.01),
               alpha=np.ones((h, w), dtype=F), **guides)
    prev = dict(color=g.random((h, w, 3), dtype=F) * F(5), variance=g.random((h, w), dtype=F) * F(0.01),
                history=np.full((h, w), F(3)), **guides)
    par = rt.temporal_params(w, h, alpha_min=0.01, max_history=64.0, normal_tol=0.1, depth_tol=0.1)
    for radius in clip_cases.RADII:
        c, v, n, reason, info = R.accumulate(cur, prev, cam, cam, par, rt.temporal_clip(radius=radius, gamma=3.0))
        assert (reason == R.KEPT).all() and np.abs(n - 4).max() < 1e-5
        assert np.array_equal(u32(info["lo"]), u32(cur["beauty"])) and np.array_equal(u32(info["hi"]), u32(cur["beauty"]))
        assert_bits(info["clamped"], cur["beauty"])
        k = np.fmax(F(1) / n, F(par.alpha_min))
        assert_bits(c, k[..., None] * cur["beauty"] + (F(1) - k)[..., None] * cur["beauty"])
        assert (u32(info["resampled"]) != u32(cur["beauty"])).any()


def test_window_box_against_float64_statistics():
    """lo and hi of the restatement, for the library's record (rt.temporal_clip), against the window's mean
    and standard deviation formed in float64 from the unshifted data (which shares nothing with the
    shifted float32 sums). The bound, per pixel and channel, with u = 2^-24, values in [0, 1] and at most
    n = 49 taps (the record's radius is at most 3):
      - a float32 sum of n terms below 1 in magnitude is off by at most (n - 1) u n, so m1 / n and m2 / n
        by E = 49 u each, and the rounding of d, d * d and the division adds less than 3 u: mean, ex2
        and mu = b + mean are each within 2 E of their exact values;
      - s2 = ex2 - mean^2: 2 E from ex2, 2 * 2 E from the square of a mean below 1, one rounding: within
        e = 8 E of the exact variance;
      - |sqrt(a) - sqrt(a')| = |a - a'| / (sqrt(a) + sqrt(a')) is at most e / sd and at most sqrt(e);
      - gamma * sqrt, and mu -+ half: three more roundings of numbers below 4, 3 * 4 u.
    So |lo - lo64| and |hi - hi64| are at most 2 E + gamma min(sqrt(e), e / sd) + 12 u: 1.3e-4 for the
    random windows here (sd about 0.29), and gamma x 4.8e-3 only where the deviation vanishes."""
    clip = rt.temporal_clip(radius=2, gamma=1.5)
    w, h, radius, gamma = 23, 11, int(clip.radius), float(clip.gamma)
    g = np.random.default_rng(8)
    b = g.random((h, w, 3), dtype=F)
    sid = (g.random((h, w)) < 0.3).astype(np.uint32)
    lo, hi = R.window_box(b, sid, radius, gamma)
    u = 2.0 ** -24
    E = 49 * u
    e = 8 * E
    worst = worst_ratio = 0.0
    for y in range(h):
        for x in range(w):
            ys, xs = slice(max(0, y - radius), min(h, y + radius + 1)), slice(max(0, x - radius), min(w, x + radius + 1))
            taps = b[ys, xs][sid[ys, xs] == sid[y, x]].astype(np.float64)
            mu, sd = taps.mean(axis=0), taps.std(axis=0)
            bound = 2 * E + gamma * np.minimum(np.sqrt(e), e / np.maximum(sd, 1e-300)) + 12 * u
            diff = np.maximum(np.abs(lo[y, x] - (mu - gamma * sd)), np.abs(hi[y, x] - (mu + gamma * sd)))
            worst, worst_ratio = max(worst, diff.max()), max(worst_ratio, (diff / bound).max())
    print(f"largest difference from the float64 box: {worst:.3e}; largest share of its bound: {worst_ratio:.3f}")
    assert worst_ratio <= 1.0
