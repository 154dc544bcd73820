"""The guided upsample and the upscaled preview session without a GPU (rt_upsample*,
rt_preview_upscale_default, rt_preview_create_upscaled): the records, every argument
check with its field named (all made before any device call: rt_upsample_device is called with
made-up non-null addresses, which a call that fails its checks never touches, and the session is
created with a null scene, which is looked at last), the Python builders against the C defaults, and
properties of the numpy restatement (tests/tools/upsample_ref.py) on the synthetic planes of
tests/tools/upsample_cases.py.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import upsample_cases  # noqa: E402
import upsample_ref  # noqa: E402
from support import assert_bits, census, words as u32  # noqa: E402

F = np.float32
W0, H0, LW0, LH0 = 70, 37, 35, 19
SIZES = [(32, 18, 64, 36), (35, 19, 70, 37), (23, 12, 67, 35), (64, 36, 64, 36), (1, 1, 5, 3)]


# ---- records -------------------------------------------------------------------------------------
def test_record_sizes_and_default_records():
    assert C.sizeof(abi.RtUpsampleParams) == 32 and C.sizeof(abi.RtUpsampleBuffers) == 96
    assert C.sizeof(abi.RtPreviewUpscale) == 24 and C.sizeof(abi.RtPreviewOutput) == 64
    assert [n for n, _ in abi.RtUpsampleBuffers._fields_[1:]] == list(abi.UPSAMPLE_PLANES)
    assert [n for n, _ in abi.RtPreviewOutput._fields_[3:]] == list(abi.PREVIEW_OUTPUT_PLANES)
    L = rt.lib()
    p = abi.RtUpsampleParams()
    assert L.rt_upsample_params_default(1280, 720, 640, 360, C.byref(p)) == abi.RT_OK
    assert (p.size, p.width, p.height, p.lo_width, p.lo_height, p.flags) == (32, 1280, 720, 640, 360, 0)
    # the defaults lie in the ranges the checks accept (their values are not pinned)
    assert p.normal_tol >= 0 and p.depth_tol >= 0 and np.isfinite(p.normal_tol) and np.isfinite(p.depth_tol)
    for bad in ((0, 720, 640, 360), (1280, 0, 640, 360), (1280, 720, 0, 360), (1280, 720, 640, 0)):
        assert L.rt_upsample_params_default(*bad, C.byref(p)) == abi.RT_ERR_INVALID
    assert L.rt_upsample_params_default(1280, 720, 640, 360, None) == abi.RT_ERR_INVALID
    rec = rt.upsample_buffers({"lo_color": 1, "out_color": 2})
    assert (rec.size, rec.lo_color, rec.out_color, rec.lo_variance) == (96, 1, 2, None)
    pp = rt.preview_params(LW0, LH0, 4)
    u = abi.RtPreviewUpscale()
    assert L.rt_preview_upscale_default(C.byref(pp), W0, H0, C.byref(u)) == abi.RT_OK
    assert (u.size, u.out_width, u.out_height, u.guide_samples) == (24, W0, H0, 0)
    q = rt.upsample_params(W0, H0, LW0, LH0)
    assert (u.normal_tol, u.depth_tol) == (q.normal_tol, q.depth_tol)
    assert L.rt_preview_upscale_default(C.byref(pp), LW0 - 1, H0, C.byref(u)) == abi.RT_ERR_INVALID
    assert L.rt_preview_upscale_default(C.byref(pp), W0, LH0 - 1, C.byref(u)) == abi.RT_ERR_INVALID
    assert L.rt_preview_upscale_default(None, W0, H0, C.byref(u)) == abi.RT_ERR_INVALID
    assert L.rt_preview_upscale_default(C.byref(pp), W0, H0, None) == abi.RT_ERR_INVALID


def test_python_builders_produce_the_c_defaults():
    L = rt.lib()
    p = abi.RtUpsampleParams()
    assert L.rt_upsample_params_default(W0, H0, LW0, LH0, C.byref(p)) == abi.RT_OK
    assert bytes(rt.upsample_params(W0, H0, LW0, LH0)) == bytes(p)
    q = rt.upsample_params(W0, H0, LW0, LH0, normal_tol=0.25, depth_tol=0.02)
    assert (q.normal_tol, q.depth_tol, q.width, q.lo_height) == (0.25, F(0.02), W0, LH0)
    r = rt.upsample_params(64, 36, 32, 18, base=q)
    assert (r.normal_tol, r.width, r.height, r.lo_width, r.lo_height, r.size) == (0.25, 64, 36, 32, 18, 32)
    with pytest.raises(KeyError):
        rt.upsample_params(W0, H0, LW0, LH0, size=3)
    with pytest.raises(KeyError):
        rt.upsample_buffers({"color": 1})
    pp = rt.preview_params(LW0, LH0, 4)
    u = abi.RtPreviewUpscale()
    assert L.rt_preview_upscale_default(C.byref(pp), W0, H0, C.byref(u)) == abi.RT_OK
    assert bytes(rt.preview_upscale(pp, W0, H0)) == bytes(u)
    v = rt.preview_upscale(pp, W0, H0, guide_samples=1, normal_tol=0.125)
    assert (v.guide_samples, v.normal_tol, v.depth_tol, v.out_width, v.out_height) == (1, 0.125, u.depth_tol, W0, H0)
    with pytest.raises(KeyError):
        rt.preview_upscale(pp, W0, H0, size=3)
    with pytest.raises(rt.RtError):
        rt.preview_upscale(pp, LW0 - 1, H0)


# ---- the stage's argument checks --------------------------------------------------------------------
# made-up, distinct, non-null addresses: a refused call never touches them
FAKE = {n: 0x10000 * (i + 1) for i, n in enumerate(abi.UPSAMPLE_PLANES)}


def _refused(drop=(), alias=None, params_size=None, buffers_size=None, raw=None):
    p = rt.upsample_params(W0, H0, LW0, LH0)
    for k, v in (raw or {}).items():
        setattr(p, k, v)
    if params_size is not None:
        p.size = params_size
    ptr = {n: a for n, a in FAKE.items() if n not in drop}
    for a, b in (alias or {}).items():
        ptr[a] = ptr[b]
    rec = rt.upsample_buffers(ptr)
    if buffers_size is not None:
        rec.size = buffers_size
    L = rt.lib()
    rc = L.rt_upsample_device(C.byref(p), C.byref(rec), None)
    return rc, L.rt_last_error().decode()


INPUTS = [n for n in abi.UPSAMPLE_PLANES if not n.startswith("out_")]
REFUSED = (
    [("params.size", dict(params_size=28)), ("buffers.size", dict(buffers_size=88))]
    + [(f, dict(raw={f: v})) for f in ("width", "height") for v in (0, 65537)]
    + [("lo_width", dict(raw=dict(lo_width=0))), ("lo_width", dict(raw=dict(lo_width=W0 + 1))),
       ("lo_height", dict(raw=dict(lo_height=0))), ("lo_height", dict(raw=dict(lo_height=H0 + 1)))]
    + [(f, dict(raw={f: v})) for f in ("normal_tol", "depth_tol") for v in (-1.0, float("inf"), float("nan"))]
    + [("flags", dict(raw=dict(flags=1))), ("flags", dict(raw=dict(flags=1 << 31)))]
    + [(n, dict(drop=(n,))) for n in abi.UPSAMPLE_PLANES if n not in ("lo_variance", "out_variance")]
    + [("lo_variance", dict(drop=("out_variance",))), ("out_variance", dict(drop=("lo_variance",)))]
    + [("out_color", dict(alias={"out_color": n})) for n in INPUTS]
    + [("out_variance", dict(alias={"out_variance": n})) for n in INPUTS]
    + [("out_variance", dict(alias={"out_variance": "out_color"}))]
)


@pytest.mark.parametrize("field,how", REFUSED, ids=[f"{i}-{f}" for i, (f, _) in enumerate(REFUSED)])
def test_upsample_device_refuses_with_the_field_named(field, how):
    rc, msg = _refused(**how)
    assert rc == abi.RT_ERR_INVALID, msg
    assert msg.startswith("rt_upsample_device: ")
    # the field's name stands alone: "width" must not be found in "lo_width"
    assert f" {field} " in msg.replace(":", " ") + " ", msg
    if "alias" in how:
        assert list(how["alias"].values())[0] in msg, msg


def test_null_records_are_refused():
    L = rt.lib()
    p, rec = rt.upsample_params(W0, H0, LW0, LH0), rt.upsample_buffers(FAKE)
    assert L.rt_upsample_device(None, C.byref(rec), None) == abi.RT_ERR_INVALID
    assert L.rt_upsample_device(C.byref(p), None, None) == abi.RT_ERR_INVALID
    assert L.rt_upsample(None, None, None) == abi.RT_ERR_INVALID


def test_the_host_call_passes_its_checks_without_the_variance_pair_and_with_it():
    """A call that is complete fails, if at all, on the device (no GPU here), never on a check."""
    lo, guides = upsample_cases.planes(LW0, LH0, W0, H0)
    for with_var in (False, True):
        low = {n: a for n, a in lo.items() if with_var or n != "variance"}
        try:
            rt.upsample(low, guides)
        except rt.RtError as e:
            assert e.status != abi.RT_ERR_INVALID, str(e)


# ---- the session's second record ------------------------------------------------------------------------
def _create(change=None, u_size=None, **fields):
    p = rt.preview_params(LW0, LH0, 4)
    if change:
        change(p)
    u = rt.preview_upscale(rt.preview_params(LW0, LH0, 4), W0, H0)
    for k, v in fields.items():
        setattr(u, k, v)
    if u_size is not None:
        u.size = u_size
    with pytest.raises(rt.RtError) as e:
        rt.Preview(None, p, u)
    assert e.value.status == abi.RT_ERR_INVALID, str(e.value)
    return str(e.value)


UPSCALE_REFUSED = [
    ("upscale.size", dict(u_size=20)), ("out_width", dict(out_width=LW0 - 1)), ("out_width", dict(out_width=65537)),
    ("out_height", dict(out_height=LH0 - 1)), ("out_height", dict(out_height=65537)),
    ("out_width * out_height", dict(out_width=65536, out_height=32768)),
    ("guide_samples", dict(guide_samples=5)),
    ("normal_tol", dict(normal_tol=-1.0)), ("normal_tol", dict(normal_tol=float("nan"))),
    ("depth_tol", dict(depth_tol=-0.5)), ("depth_tol", dict(depth_tol=float("inf"))),
]


@pytest.mark.parametrize("field,fields", UPSCALE_REFUSED, ids=[f"{i}-{f}" for i, (f, _) in enumerate(UPSCALE_REFUSED)])
def test_create_upscaled_refuses_with_the_field_named(field, fields):
    msg = _create(**fields)
    assert "rt_preview_create_upscaled: " in msg
    assert f" {field} " in msg.replace(":", " ") + " ", msg


def test_create_upscaled_checks_params_first_and_the_scene_last():
    def bad_spp(p):
        p.spp = 1
    # p is checked as rt_preview_create checks it, before u ...
    msg = _create(change=bad_spp, out_width=LW0 - 1)
    assert " spp " in msg and "out_width" not in msg
    # ... and with both records right, the null scene is what is refused
    p = rt.preview_params(LW0, LH0, 4)
    with pytest.raises(rt.RtError) as e:
        rt.Preview(None, p, rt.preview_upscale(p, W0, H0, guide_samples=4))
    assert e.value.status == abi.RT_ERR_INVALID and "scene" in str(e.value)
    h = C.c_void_p()
    assert rt.lib().rt_preview_create_upscaled(None, C.byref(p), None, C.byref(h)) == abi.RT_ERR_INVALID
    assert "upscale" in rt.lib().rt_last_error().decode()
    out = abi.RtPreviewOutput()
    assert rt.lib().rt_preview_output(None, C.byref(out)) == abi.RT_ERR_INVALID


# ---- the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("lw,lh,w,h", SIZES)
def test_restatement_shapes_positions_and_the_plain_weight(lw, lh, w, h):
    lo, guides = upsample_cases.planes(lw, lh, w, h)
    p = rt.upsample_params(w, h, lw, lh)
    color, variance, reason, outside = upsample_ref.upsample(lo, guides, p)
    assert color.shape == (h, w, 3) and variance.shape == (h, w) and reason.shape == (h, w) and outside.shape == (h, w)
    assert color.dtype == F and variance.dtype == F and np.isfinite(color).all() and np.isfinite(variance).all()
    # the colour does not depend on whether the variance pair is there
    c2, v2, r2, _ = upsample_ref.upsample({n: a for n, a in lo.items() if n != "variance"}, guides, p)
    assert v2 is None and np.array_equal(u32(c2), u32(color)) and np.array_equal(r2, reason)
    if lw < w and lh < h:
        # the image's border rows and columns have taps outside (positions below 0 or above the last centre)
        assert outside[0].all() and outside[:, 0].all() and outside[-1].all() and outside[:, -1].all()
    # a weighted mean of the taps: within the low-resolution image's range
    assert color.min() >= lo["color"].min() * F(1 - 1e-6) and color.max() <= lo["color"].max() * F(1 + 1e-6)


def test_census_every_reason_occurs_and_guided_pixels_are_a_fair_share():
    lo, guides = upsample_cases.planes(LW0, LH0, W0, H0)
    _, _, reason, outside = upsample_ref.upsample(lo, guides, rt.upsample_params(W0, H0, LW0, LH0))
    counts = census(reason, upsample_ref.REASONS)
    print("taps outside on", int(outside.sum()), "pixels")
    assert all(counts.values()), counts
    share = counts["guided"] / reason.size
    assert 0.2 <= share <= 0.8, share
    assert outside.any() and not outside.all()


def test_tight_tolerances_leave_the_id_test_and_zero_ones_reject_surfaces():
    lo, guides = upsample_cases.planes(LW0, LH0, W0, H0)
    zero = rt.upsample_params(W0, H0, LW0, LH0, normal_tol=0.0, depth_tol=0.0)
    _, _, reason, _ = upsample_ref.upsample(lo, guides, zero)
    surface = guides["alpha"] == 1
    # depths carry a jitter: with a zero tolerance no tap of a surface pixel passes the depth test
    assert (reason[surface] != upsample_ref.GUIDED).all()
    # sky and edge pixels take the id test only: the tolerances do not matter to them
    _, _, wide, _ = upsample_ref.upsample(lo, guides, rt.upsample_params(W0, H0, LW0, LH0))
    assert np.array_equal(reason[~surface], wide[~surface]) and (wide[~surface] == upsample_ref.GUIDED).any()


def test_one_low_pixel_gives_its_colour_bits_everywhere():
    """lw = lh = 1 on the module's synthetic planes: every output equals the single low pixel's
    colour bits.

    This holds for these planes and is not a property of the contract: with one tap the value is
    (wgt * c) / wgt, two roundings, which returns c for certain only where wgt * c is exact (the
    centre pixel, wgt = 1). At 1 x 1 -> 5 x 3 the weights are products of {0.6, 0.8, 1, 0.8, 0.6} and
    {2/3, 1, 2/3} as binary32 rounds them. Measured on the restatement: 0 of the 45 values differ
    with the seed the modules use (11); over the seeds 0..199 of upsample_cases.planes 944 of 9000
    values differ, each by one unit in the last place. What holds for every colour is asserted by
    test_one_low_pixel_within_one_ulp below; the GPU is held to the restatement's bits, not to this
    property (tests/test_upsample_gpu.py, 1 x 1 -> 5 x 3)."""
    lo, guides = upsample_cases.planes(1, 1, 5, 3)
    color, _, _, _ = upsample_ref.upsample(lo, guides, rt.upsample_params(5, 3, 1, 1))
    want = np.broadcast_to(lo["color"][0, 0], (3, 5, 3))
    bad = int(np.count_nonzero(u32(color) != u32(want)))
    print("values that differ from the low pixel's bits:", bad, "of", color.size)
    assert bad == 0


def test_one_low_pixel_within_one_ulp():
    """What holds for lw = lh = 1: the centre pixel (weight 1) has the low pixel's bits, every other
    one lies within one unit in the last place of them ((wgt * c) / wgt: two roundings of relative
    2^-24 each, and the quotient is rounded to nearest)."""
    differ = 0
    for seed in range(20):
        lo, guides = upsample_cases.planes(1, 1, 5, 3, seed=seed)
        color, variance, reason, outside = upsample_ref.upsample(lo, guides, rt.upsample_params(5, 3, 1, 1))
        c = lo["color"][0, 0]
        assert_bits(color[1, 2], c)
        ulps = np.abs(u32(color).astype(np.int64) - u32(np.broadcast_to(c, (3, 5, 3))).astype(np.int64))
        assert ulps.max() <= 1
        differ += int(ulps.sum())
        assert outside.all()  # ix + 1 or ix lies outside a 1 x 1 image whatever ix is
    print("values one unit in the last place away, seeds 0..19:", differ, "of", 20 * 45)
    assert differ > 0  # (the bits themselves are not a property of the contract)
