"""The guided upsample on the GPU (rt_upsample_device, rt_upsample).

Every comparison is on uint32 views with zero mismatches allowed, against the numpy restatement
(tests/tools/upsample_ref.py), which runs once per case and is shared. Synthetic planes
(tests/tools/upsample_cases.py) at an exact 2x, at a non-integer ratio with a partial wave per row
and a last row group short of four rows, at about 3x, at the same size and from a single pixel; and
planes rendered from the huge scene by the public synchronous calls at 35 x 19 and 70 x 37, 4 spp,
max_depth 8, with the preview session's corrected camera (one camera for both sizes).
"""
import functools
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import upsample_cases  # noqa: E402
import upsample_ref  # noqa: E402
from device_io import SENTINEL  # noqa: E402
from support import assert_bits as assert_same, census, orbit_camera  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(32, 18, 64, 36), (35, 19, 70, 37), (23, 12, 67, 35), (64, 36, 64, 36), (1, 1, 5, 3)]
SCENE_SEED, SPP, MAX_DEPTH = 1234, 4, 8


@functools.lru_cache(maxsize=None)
def case(lw, lh, w, h):
    """The synthetic planes of a size and the restatement's result, once."""
    lo, guides = upsample_cases.planes(lw, lh, w, h)
    ref = upsample_ref.upsample(lo, guides, rt.upsample_params(w, h, lw, lh))
    return lo, guides, ref


def run_device(lo, guides, w, h, lw, lh, with_variance):
    """rt_upsample_device on a stream of its own into sentinel-filled outputs: (color, variance or
    None), and the inputs as they are on the device afterwards."""
    import torch
    host = {**{"lo_" + n: a for n, a in lo.items() if with_variance or n != "variance"}, **guides}
    dev = {n: torch.from_numpy(np.array(a.view(np.int32) if a.dtype == np.uint32 else a)).to("cuda:0") for n, a in host.items()}
    out = {"out_color": torch.full((h, w, 3), SENTINEL, dtype=torch.float32, device="cuda:0")}
    if with_variance:
        out["out_variance"] = torch.full((h, w), SENTINEL, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    rt.upsample_device({n: t.data_ptr() for n, t in {**dev, **out}.items()}, rt.upsample_params(w, h, lw, lh), st.cuda_stream)
    st.synchronize()
    after = {n: t.cpu().numpy().view(host[n].dtype) for n, t in dev.items()}
    for n, a in host.items():
        assert_same(after[n], a, f"input plane {n} changed")
    return out["out_color"].cpu().numpy(), out["out_variance"].cpu().numpy() if with_variance else None


@pytest.mark.parametrize("lw,lh,w,h", SIZES)
def test_device_call_equals_the_restatement(lw, lh, w, h):
    lo, guides, (ref_c, ref_v, reason, _) = case(lw, lh, w, h)
    color, variance = run_device(lo, guides, w, h, lw, lh, True)
    census(reason, upsample_ref.REASONS)
    assert (color != SENTINEL).all() and (variance != SENTINEL).all()
    assert_same(color, ref_c, "colour")
    assert_same(variance, ref_v, "variance")
    # the same colour bits without the variance pair
    alone, none = run_device(lo, guides, w, h, lw, lh, False)
    assert none is None
    assert_same(alone, ref_c, "colour without the variance pair")


def test_the_census_conditions_hold_on_the_restatement():
    _, _, (_, _, reason, outside) = case(35, 19, 70, 37)
    counts = census(reason, upsample_ref.REASONS)
    assert all(counts.values()), counts
    assert 0.2 <= counts["guided"] / reason.size <= 0.8
    assert outside.any()


# ---- rendered planes --------------------------------------------------------------------------------------
def test_host_call_on_rendered_planes_equals_the_restatement():
    scene = rt.huge_scene_arrays(SCENE_SEED)
    lw, lh, w, h = 35, 19, 70, 37
    cam = orbit_camera(w, h, 0)  # the preview module's corrected camera, frame 0 of its orbit; one camera for both sizes: depths compare directly
    p_lo, p_hi = rt.make_params(lw, lh, SPP, MAX_DEPTH, 1), rt.make_params(w, h, SPP, MAX_DEPTH, 1)
    beauty, variance, _ = rt.render_var(scene, p_lo, cam)
    g_lo = rt.render_aov(scene, p_lo, cam, 0)
    g_hi = rt.render_aov(scene, p_hi, cam, 0)
    lo = dict(color=beauty, variance=variance, normal=g_lo["normal"], depth=g_lo["depth"], sphere_id=g_lo["sphere_id"])
    guides = {n: g_hi[n] for n in ("normal", "depth", "alpha", "sphere_id")}
    params = rt.upsample_params(w, h, lw, lh)
    ref_c, ref_v, reason, outside = upsample_ref.upsample(lo, guides, params)
    counts = census(reason, upsample_ref.REASONS)
    print("taps outside on", int(outside.sum()), "pixels; surface pixels:", int((guides["alpha"] == 1).sum()))
    stats = abi.RtStats()
    color, var = rt.upsample(lo, guides, stats=stats)
    assert_same(color, ref_c, "colour")
    assert_same(var, ref_v, "variance")
    assert stats.kernel_ms > 0 and stats.wall_ms >= stats.kernel_ms
    assert_same(rt.upsample({n: a for n, a in lo.items() if n != "variance"}, guides), ref_c, "colour alone")
    # both guided and fallback pixels occur with this camera
    assert counts["guided"] > 0 and reason.size - counts["guided"] > 0, counts
