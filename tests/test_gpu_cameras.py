"""GPU renders under non-default cameras and material extremes (tests/tools/camera_cases.py)
against the CPU restatement, bit for bit.

The kernels' shortcuts hold under conditions on the camera or the materials that the other GPU
suites never flip: the short root and division forms need every active lane's a = |d|^2 in
[2^-40, 2^40] (rt_trace.h ray_div: the per-wave fallback with KParams::fast_roots on runs only
where part of a wave is outside, the tiny_* and wide_* cases; in the subnormal_* cases a itself
is below 2^-126 for half the primaries, where the short forms do give other bits), the sky kernel
and the sky blocks of aov_kernel rely on rt_tile_order's proof, the always-tested-sphere gate is a function of a, and
the walk, the transposed member tests and the isolated-ball shortcut start here from inside balls,
under the ground and among the cluster boxes. tests/test_camera_cases_cpu.py fixes, from the
reference alone, that the cases are what they claim to be.

Every comparison is on uint32 views with zero mismatches allowed, and the segment count equals
the oracle's wherever it reports one. References and default renders are computed once per module.
"""
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import camera_cases as CC  # noqa: E402
from support import assert_all_bits, assert_bits, words as u32  # noqa: E402

pytestmark = pytest.mark.gpu

PLANES = tuple(abi.AOV_PLANES)
OPTION_CASES = CC.RANGE_CASES + CC.SUBNORMAL_CASES + ("in_glass", "in_bubble", "grazing", "materials")
VARIANTS = {"ieee_roots": {"ieee_roots": True}, "no_sky": {"no_sky": True}, "natural_order": {"natural_order": True},
            "transpose0": {"transpose_max": 0}, "no_shortcut": {"no_shortcut": True},
            "deep": {"deep_split": 3, "deep_min_items": 0}}
SENTINEL = 0x5a5a5a5a


_default = {}


def gpu_default(name):
    """The case's frame under the default options, rendered once (ask before changing the options)."""
    if name not in _default:
        img, st = rt.render_f32(CC.scene(name), CC.params(name), CC.case(name).camera)
        _default[name] = (img, int(st.segments), int(st.primaries))
    return _default[name]


@pytest.mark.parametrize("name", CC.NAMES)
def test_beauty_matches_oracle(name):
    """rt.render_f32 against the oracle, bits and segments; brute force (every sphere per lane, no
    cluster boxes) the same: the padded-box slab tests of the culled walk see directions of 1e-7
    (tiny) and 1e6 (wide)."""
    c = CC.case(name)
    ref, ref_seg = CC.beauty_ref(name)
    img, seg, prim = gpu_default(name)
    assert_bits(img, ref, f"{name} culled")
    assert seg == ref_seg
    assert prim == ref.shape[0] * c.W * c.spp
    brute, sb = rt.render_f32(CC.scene(name), CC.params(name, brute_force=True), c.camera)
    assert_bits(brute, ref, f"{name} brute force")
    assert sb.segments == ref_seg


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", OPTION_CASES)
def test_same_bits_under_options(name, variant, opts):
    """IEEE roots for the whole frame, no sky kernel, natural dealing order, per-lane member tests,
    no isolated-ball shortcut, and the deep launch from segment 3 on: the default render's bits."""
    img, seg, _ = gpu_default(name)
    opts.set(**VARIANTS[variant])
    got, st = rt.render_f32(CC.scene(name), CC.params(name), CC.case(name).camera)
    assert_bits(got, img, f"{name} {variant} against the default render")
    assert_bits(got, CC.beauty_ref(name)[0], f"{name} {variant} against the oracle")
    assert st.segments == seg == CC.beauty_ref(name)[1]


@pytest.mark.parametrize("name", ["tiny", "wide", "subnormal", "in_glass", "in_bubble"])
def test_wavefront_variant(name):
    ref, ref_seg = CC.beauty_ref(name)
    got, st = rt.render_f32(CC.scene(name), CC.params(name, wavefront=True), CC.case(name).camera)
    assert_bits(got, ref, f"{name} wavefront")
    assert st.segments == ref_seg


@pytest.mark.parametrize("name", CC.NAMES)
def test_feature_buffers_match_reference(name):
    """aov_kernel has its own copy of the range gate and of the sky blocks: all five planes."""
    ref = CC.aov_reference(name)
    got = rt.render_aov(CC.scene(name), CC.params(name), CC.case(name).camera)
    assert_all_bits(got, ref, name, PLANES)


def _render_device(name, p, rows, options=None, events=False):
    """The case through rt_render_device into a buffer of `rows` rows filled with an integer sentinel,
    read back as its words: the float32 references are compared as u32(ref), the same bytes."""
    import torch
    c = CC.case(name)
    out = torch.full((rows, c.W, 3), SENTINEL, dtype=torch.int32, device="cuda:0")
    ds = rt.DeviceScene(CC.scene(name), device=0, options=options)
    try:
        ds.render(c.camera, p, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ev = ds.debug_events(reset=True) if events else None
    finally:
        ds.close()
    return out.cpu().numpy().view(np.uint32), ev


def test_materials_instrumented_witness():
    """The instrumented kernel on `materials`: metals absorbed and dielectrics scattered, and its
    frame is the reference's. (A witness on the code under test; the reference-side census of
    tests/test_camera_cases_cpu.py is what guards the case.)"""
    c = CC.case("materials")
    got, ev = _render_device("materials", CC.params("materials"), c.H,
                             rt.options(rt.default_options(), stats=True), events=True)
    print("events:", {k: ev[k] for k in ("metal_absorb", "dielectric", "lambert", "hit", "sky")})
    assert ev["metal_absorb"] > 0 and ev["dielectric"] > 0, ev
    assert_bits(got, u32(CC.beauty_ref("materials")[0]), "materials instrumented")


def test_share_rows():
    """Rows 1, 4, 7, ... of the grazing frame: packed they are the oracle's rows (which are the
    whole frame's), and a full-frame buffer keeps its other rows untouched."""
    c = CC.case("share")
    ref, ref_seg = CC.beauty_ref("share")
    rows = slice(c.row_offset, c.H, c.row_stride)
    assert ref.shape[0] == 13
    assert_bits(ref, CC.beauty_ref("grazing")[0][rows], "oracle: share against the whole frame's rows")
    img, seg, _ = gpu_default("share")
    assert_bits(img, ref, "share packed")
    assert seg == ref_seg
    full, _ = _render_device("share", CC.params("share", full_frame=True), c.H)
    assert_bits(full[rows], u32(ref), "share full frame, its rows")
    other = np.ones(c.H, dtype=bool)
    other[rows] = False
    assert (full[other] == SENTINEL).all()
