"""The à-trous denoiser without a GPU (rt_denoise*): the records, every argument
check (all made before any device call), the properties of the CPU reference
(tests/tools/denoise_ref.py) that the GPU tests compare against, and the quality condition that
chose the default parameters.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import oracle_binding as O
import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import aov_ref  # noqa: E402
import denoise_ref  # noqa: E402
from support import assert_bits, synthetic_planes, words as u32  # noqa: E402

F = np.float32


# ---- records -------------------------------------------------------------------------------------
def test_record_sizes_and_default_record():
    assert C.sizeof(abi.RtDenoiseParams) == 36 and C.sizeof(abi.RtDenoiseBuffers) == 56
    p = abi.RtDenoiseParams()
    assert rt.lib().rt_denoise_params_default(640, 360, C.byref(p)) == abi.RT_OK
    assert (p.size, p.width, p.height, p.flags) == (36, 640, 360, 0)
    # the values the sweep of DESIGN.md §4.9 chose
    assert (p.levels, p.sigma_color, p.sigma_normal, p.sigma_depth, p.sigma_albedo) == (2, 4.0, 2.0, 1.0, 1.0)
    assert rt.lib().rt_denoise_params_default(0, 360, C.byref(p)) == abi.RT_ERR_INVALID
    assert rt.lib().rt_denoise_params_default(640, 360, None) == abi.RT_ERR_INVALID
    q = rt.denoise_params(8, 4, levels=5, sigma_depth=0.5, demodulate=True, direct=True)
    assert (q.width, q.height, q.levels, q.sigma_depth, q.sigma_color) == (8, 4, 5, 0.5, 4.0)
    assert q.flags == abi.RT_DENOISE_DEMODULATE | abi.RT_DENOISE_DIRECT
    assert rt.denoise_params(8, 4, base=q, direct=False).flags == abi.RT_DENOISE_DEMODULATE
    with pytest.raises(KeyError):
        rt.denoise_params(8, 4, sigma=1)


# ---- argument checks -------------------------------------------------------------------------------
W0, H0 = 6, 4
_PLANES = {n: np.zeros((H0, W0, 3) if ch == 3 else (H0, W0), dtype=np.float32) for n, ch in abi.DENOISE_PLANES.items()}


def _call(device, params=None, planes=("beauty", "albedo", "normal", "depth", "out", "scratch"), alias=None,
          params_size=None, buffers_size=None, **fields):
    """The status and message of rt_denoise (host) or rt_denoise_device with host addresses, which a
    call that fails its checks never touches."""
    p = rt.denoise_params(W0, H0, **fields) if params is None else params
    if params_size is not None:
        p.size = params_size
    ptr = {n: _PLANES[n].ctypes.data for n in planes}
    for a, b in (alias or {}).items():
        ptr[a] = ptr[b]
    rec = rt.render.denoise_buffers(ptr)
    if buffers_size is not None:
        rec.size = buffers_size
    L = rt.lib()
    rc = L.rt_denoise_device(C.byref(p), C.byref(rec), None) if device else L.rt_denoise(C.byref(p), C.byref(rec), None)
    return rc, L.rt_last_error().decode()


def _raw(**over):
    p = rt.denoise_params(W0, H0)
    for k, v in over.items():
        setattr(p, k, v)
    return p


BAD = [
    ("params.size", dict(params_size=32)),
    ("buffers.size", dict(buffers_size=48)),
    ("width", dict(params=_raw(width=0))),
    ("height", dict(params=_raw(height=0))),
    ("levels", dict(levels=0)),
    ("levels", dict(levels=7)),
    ("sigma_color", dict(sigma_color=-1.0)),
    ("sigma_color", dict(sigma_color=float("nan"))),
    ("sigma_normal", dict(sigma_normal=float("inf"))),
    ("sigma_normal", dict(sigma_normal=-0.5)),
    ("sigma_depth", dict(sigma_depth=float("nan"))),
    ("sigma_depth", dict(sigma_depth=-2.0)),
    ("sigma_albedo", dict(sigma_albedo=float("-inf"))),
    ("sigma_albedo", dict(sigma_albedo=-1e-3)),
    ("sigma_normal", dict(sigma_normal=0.0)),
    ("sigma_depth", dict(sigma_depth=0.0)),
    ("sigma_color", dict(sigma_color=1e-20, levels=6)),
    ("flags", dict(flags=4)),
    ("albedo", dict(demodulate=True, planes=("beauty", "normal", "depth", "out", "scratch"))),
    ("beauty", dict(planes=("albedo", "normal", "depth", "out", "scratch"))),
    ("out", dict(planes=("beauty", "albedo", "normal", "depth", "scratch"))),
    ("out", dict(alias={"out": "beauty"})),
    ("out", dict(alias={"out": "albedo"})),
    ("out", dict(alias={"out": "normal"})),
    ("out", dict(alias={"out": "depth"})),
]
BAD_DEVICE_ONLY = [
    ("scratch", dict(levels=2, planes=("beauty", "albedo", "normal", "depth", "out"))),
    ("scratch", dict(levels=2, alias={"scratch": "beauty"})),
    ("scratch", dict(levels=2, alias={"scratch": "depth"})),
    ("scratch", dict(levels=2, alias={"scratch": "out"})),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("field,kw", BAD, ids=[f"{i}-{f}" for i, (f, _) in enumerate(BAD)])
def test_argument_checks_name_the_field(field, kw, device):
    """RT_ERR_INVALID before any device call (this test runs without a GPU), the field named."""
    rc, msg = _call(device, **kw)
    assert rc == abi.RT_ERR_INVALID, (rc, msg)
    assert field in msg and msg.startswith("rt_denoise_device:" if device else "rt_denoise:"), msg


@pytest.mark.parametrize("field,kw", BAD_DEVICE_ONLY, ids=[f"{i}-{f}" for i, (f, _) in enumerate(BAD_DEVICE_ONLY)])
def test_device_call_checks_scratch(field, kw):
    rc, msg = _call(True, **kw)
    assert rc == abi.RT_ERR_INVALID and field in msg, (rc, msg)


def test_zero_sigma_is_fine_for_a_plane_that_is_not_given_and_null_arguments_fail():
    # sigma_normal = 0 without a normal plane passes the checks: the next failure is another field
    rc, msg = _call(True, sigma_normal=0.0, levels=2, planes=("beauty", "albedo", "depth", "out"))
    assert rc == abi.RT_ERR_INVALID and "scratch" in msg
    L = rt.lib()
    assert L.rt_denoise(None, None, None) == abi.RT_ERR_INVALID
    assert L.rt_denoise_device(None, None, None) == abi.RT_ERR_INVALID
    assert L.rt_denoise_level_device(None, None, 0, None) == abi.RT_ERR_INVALID
    p = rt.denoise_params(W0, H0, levels=2)
    rec = rt.render.denoise_buffers({n: _PLANES[n].ctypes.data for n in ("beauty", "out")})
    assert L.rt_denoise_level_device(C.byref(p), C.byref(rec), 2, None) == abi.RT_ERR_INVALID
    assert b"level" in L.rt_last_error()


def test_python_wrapper_checks_shapes_and_dtypes():
    b = np.zeros((H0, W0, 3), dtype=np.float32)
    with pytest.raises(ValueError):
        rt.denoise(b.astype(np.float64))
    with pytest.raises(ValueError):
        rt.denoise(b[..., 0])
    with pytest.raises(ValueError):
        rt.denoise(b, depth=np.zeros((H0, W0, 1), dtype=np.float32))
    with pytest.raises(ValueError):
        rt.denoise(b, normal=np.zeros((H0, W0 + 1, 3), dtype=np.float32))
    with pytest.raises(KeyError):
        rt.denoise(b, sigma=1.0)
    with pytest.raises(KeyError):
        rt.render.denoise_buffers({"colour": 1})


# ---- properties of the reference ---------------------------------------------------------------------
def _random_planes(w, h, seed):
    p = synthetic_planes(w, h, seed=seed)
    return tuple(p[n] for n in ("beauty", "albedo", "normal", "depth"))


def test_reference_single_pixel_is_the_centre_tap_chain():
    """1 x 1: every level sees the centre tap only, edge value 1: c -> (k c) / k with k = 9/64."""
    beauty, albedo, normal, depth = _random_planes(1, 1, 1)
    k = F(0.375) * F(0.375)
    out, census = denoise_ref.denoise(beauty, albedo, normal, depth, 3, 1.0, 1.0, 1.0, 1.0)
    c = beauty
    for _ in range(3):
        c = (k * c) / k
    assert c.dtype == np.float32 and np.array_equal(u32(out), u32(c)) and census == (0, 0, 0)
    a1 = np.maximum(albedo, F(0.0078125))
    c = beauty / a1
    for _ in range(3):
        c = (k * c) / k
    out, _ = denoise_ref.denoise(beauty, albedo, normal, depth, 3, 1.0, 1.0, 1.0, 1.0, True)
    assert_bits(out, c * a1)


def test_reference_taps_beyond_the_image_are_skipped():
    """5 x 3 at levels = 3: at step 4 every non-centre tap of columns 1..3 is outside, so there the
    last level is the centre-tap chain (k c) / k over the second level's output; columns 0 and 4
    see each other (x = 0 + 4 and 4 - 4) as their one other tap, computed here by hand in the
    contract's order: the tap with the smaller i first."""
    beauty, albedo, normal, depth = _random_planes(5, 3, 2)
    sig = (1.0, 0.5, 2.0, 0.5)
    two, c2 = denoise_ref.denoise(beauty, albedo, normal, depth, 2, *sig)
    three, c3 = denoise_ref.denoise(beauty, albedo, normal, depth, 3, *sig)
    k = F(0.375) * F(0.375)
    assert_bits(three[:, 1:4], ((k * two) / k)[:, 1:4])

    def d2(a, b):
        d = a - b
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]

    def edge(v, sigma):
        m = max(F(0), F(1) - v * (F(1) / (F(sigma) * F(sigma))))
        return m * m

    for y in range(3):
        for x, xq in ((0, 4), (4, 0)):
            w = F(0.375) * F(0.25)
            w = w * edge(d2(two[y, xq], two[y, x]), F(sig[0]) * F(0.25))
            w = w * edge(d2(normal[y, xq], normal[y, x]), sig[1])
            dz = depth[y, xq] - depth[y, x]
            w = w * edge(dz * dz, sig[2])
            w = w * edge(d2(albedo[y, xq], albedo[y, x]), sig[3])
            first, second = ((k, x), (w, xq)) if xq > x else ((w, xq), (k, x))
            sumw = (F(0) + first[0]) + second[0]
            acc = (F(0) + first[0] * two[y, first[1]]) + second[0] * two[y, second[1]]
            assert isinstance(w, np.float32) and acc.dtype == np.float32
            assert_bits(three[y, x], acc / sumw, (y, x))
    # the last level adds those 6 taps to the census and no other
    assert sum(c3) == sum(c2) + 6 and sum(c2) > 0


def _plain_b3(img, levels):
    """The à-trous B3 blur with no edge term, written pixel by pixel."""
    h, w, _ = img.shape
    taps = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))
    c = img
    for level in range(levels):
        s, d = 1 << level, np.zeros_like(img)
        for y in range(h):
            for x in range(w):
                sw, acc = F(0), [F(0), F(0), F(0)]
                for j in range(5):
                    for i in range(5):
                        qx, qy = x + (i - 2) * s, y + (j - 2) * s
                        if 0 <= qx < w and 0 <= qy < h:
                            wgt = taps[i] * taps[j]
                            sw = sw + wgt
                            acc = [acc[ch] + wgt * c[qy, qx, ch] for ch in range(3)]
                d[y, x] = [acc[ch] / sw for ch in range(3)]
        c = d
    return c


def test_reference_without_terms_is_the_plain_b3_blur():
    beauty, albedo, _, _ = _random_planes(7, 6, 3)
    out, census = denoise_ref.denoise(beauty, albedo, None, None, 2, 0.0, 0.0, 0.0, 0.0)
    assert_bits(out, _plain_b3(beauty, 2))
    assert census[0] == 0 and census[1] == 0 and census[2] > 0


@pytest.mark.parametrize("constant", [True, False], ids=["constant-halves", "random-halves"])
def test_reference_zero_weight_taps_contribute_nothing(constant):
    """A depth step between two halves with a small sigma_depth: each half's bits are those of the
    half filtered alone (where the taps across the step do not exist)."""
    h, w = 9, 16
    g = np.random.default_rng(4)
    beauty = g.random((h, w, 3), dtype=np.float32)
    if constant:
        beauty[:, :8] = (F(0.3), F(0.7), F(0.1))
        beauty[:, 8:] = (F(0.9), F(0.2), F(0.6))
    depth = np.empty((h, w), dtype=np.float32)
    depth[:, :8], depth[:, 8:] = F(1), F(5)
    kw = dict(levels=3, sigma_color=0.0, sigma_depth=0.5)
    whole, census = denoise_ref.denoise(beauty, depth=depth, **kw)
    left, _ = denoise_ref.denoise(beauty[:, :8], depth=depth[:, :8], **kw)
    right, _ = denoise_ref.denoise(beauty[:, 8:], depth=depth[:, 8:], **kw)
    assert census[0] > 0 and census[1] == 0 and census[2] > 0
    assert np.array_equal(u32(whole[:, :8]), u32(left)) and np.array_equal(u32(whole[:, 8:]), u32(right))


# ---- quality: the condition the default parameters were chosen by ---------------------------------------
@functools.lru_cache(maxsize=None)
def _quality_inputs():
    w, h, spp, seed = 64, 32, 4, 1234
    s, m = rt.simple_scene_arrays()
    cam = rt.Camera.default(w, h)
    p = rt.make_params(w, h, spp, 64, seed)
    noisy, _ = O.render_f32(s, m, cam.c, p)
    target, _ = O.render_f32(s, m, cam.c, rt.make_params(w, h, 1024, 64, seed + 1))
    return noisy, target, aov_ref.render(s, m, cam, p, spp)


def _mse(a, b):
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.parametrize("demodulate", [False, True], ids=["plain", "demodulated"])
def test_default_parameters_lower_the_error(demodulate):
    """The simple scene at 64 x 32 and 4 spp against 1024 spp: the reference denoiser with the
    library's default parameters has a lower mean squared error than the 4-spp image (the sweep of
    scripts/denoise_sweep.py, recorded in DESIGN.md §4.9: ratio 0.861 plain, 0.838 demodulated)."""
    noisy, target, g = _quality_inputs()
    p = rt.denoise_params(64, 32, demodulate=demodulate)
    out, _ = denoise_ref.denoise(noisy, g["albedo"], g["normal"], g["depth"], **denoise_ref.params_kwargs(p))
    before, after = _mse(noisy, target), _mse(out, target)
    print(f"mse 4 spp {before:.6e}, denoised {after:.6e}, ratio {after / before:.4f}")
    assert after < before
