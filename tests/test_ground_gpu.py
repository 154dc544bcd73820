"""The ground kernel and the redo launch on the GPU: every frame bit for bit
against the CPU restatement (tests/oracle_binding.py), on uint32 views with zero mismatches.

The huge scene at 128x72 has 20 ground tiles under the reference camera and 15 under the corrected
one (tests/test_ground_cpu.py); sample counts sit around the blocks of 4, the ring depths (4, 8) and the 32 samples of a thread.
A pass issued alone (the synchronous calls) runs the ground kernel beside the main launch when it is
split (`deep_min_items=1` here: so small a lone pass is otherwise unsplit and keeps its ground
tiles in the main launch), the `in_flight` option plans every pass as beside other renders; a small `max_workspace_bytes` cuts the
frame into several passes (sample_begin > 0). The redo camera looks at ground just outside the
sphere field, where part of the scattered rays pass the box over the clusters: some samples are
redone, not all. References are computed once per module and shared.
"""
import functools
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import golden_io as G  # noqa: E402
import ground_checks as GC  # noqa: E402
import oracle_binding as O  # noqa: E402
from support import assert_bits  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, DEPTH, SEED = 128, 72, 64, 1234
SPPS = (1, 3, 4, 5, 8, 9, 33)
CAMERAS = {"reference": lambda: rt.Camera.default(W, H), "corrected": lambda: rt.Camera.default(W, H, rt.CORRECTED),
           "redo": lambda: GC.redo_camera(W / H)}
GROUND_TILES = {"reference": 20, "corrected": 15, "redo": 85}
LONE_SPLIT = dict(deep_min_items=1)  # a lone pass of any size is split
FAST_TOL_PIX, FAST_TOL_FRAC, FAST_TOL_MEAN = 1e-4, 0.99, 1e-4  # tests/test_gpu_parity.py


@functools.lru_cache(maxsize=None)
def scene(which="huge"):
    s, m = G.scene("huge")
    return GC.metal_ground(s, m) if which == "metal" else GC.two_big(s, m) if which == "two_big" else (s, m)


@functools.lru_cache(maxsize=None)
def oracle(camera, spp, depth=DEPTH, which="huge", row_offset=0, row_stride=1):
    s, m = scene(which)
    p = rt.make_params(W, H, spp, depth, SEED, row_offset=row_offset, row_stride=row_stride)
    img, seg = O.render_f32(s, m, CAMERAS[camera]().c, p)
    img.flags.writeable = False
    return img, int(seg)


def device_frame(camera, spp, options=None, depth=DEPTH, which="huge", flags=None):
    """One frame through rt_render_device on a fresh scene with the counters: (image, segments,
    (ground samples, redone samples), usage)."""
    import torch
    p = rt.make_params(W, H, spp, depth, SEED, **(flags or {}))
    ds = rt.DeviceScene(scene(which), device=0, options=rt.options(**dict(LONE_SPLIT, **(options or {}))))
    try:
        out = torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda:0")
        seg = torch.zeros(3, dtype=torch.int64, device="cuda:0")
        ds.render(CAMERAS[camera](), p, out.data_ptr(), torch.cuda.current_stream().cuda_stream, d_segments=seg.data_ptr())
        torch.cuda.synchronize()
        return out.cpu().numpy(), int(seg[0].item()), ds.ground_counts(), ds.usage()
    finally:
        ds.close()


@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("camera", ["reference", "corrected"])
def test_frames_match_the_oracle(camera, spp, opts):
    """The synchronous call (a pass issued alone and split: the ground kernel beside the main launch)."""
    opts.set(**LONE_SPLIT)
    ref, ref_seg = oracle(camera, spp)
    img, st = rt.render_f32(scene(), rt.make_params(W, H, spp, DEPTH, SEED), CAMERAS[camera]())
    assert_bits(img, ref, f"{camera} spp {spp}")
    assert st.segments == ref_seg


@pytest.mark.parametrize("spp", (5, 33))
@pytest.mark.parametrize("camera", ["reference", "corrected", "redo"])
def test_passes_beside_other_renders(camera, spp):
    """Every pass planned as in a frame stream: the ground kernel, the main launch, the redo launch
    and the deep launch on the pass's stream. The ground samples are tiles x 64 x spp."""
    ref, ref_seg = oracle(camera, spp)
    img, seg, (ground, redone), _ = device_frame(camera, spp, dict(render_streams=3, in_flight=1))
    print(f"{camera} spp {spp}: {ground} ground samples, {redone} redone")
    assert_bits(img, ref, f"{camera} spp {spp} in flight")
    assert seg == ref_seg
    assert ground == GROUND_TILES[camera] * 64 * spp
    assert redone <= ground


def test_reference_camera_ground_samples():
    spp = 8
    img, seg, (ground, redone), _ = device_frame("reference", spp)
    assert_bits(img, oracle("reference", spp)[0], "reference spp 8, device call")
    assert seg == oracle("reference", spp)[1]
    assert ground == 20 * 64 * spp and redone <= ground


@pytest.mark.parametrize("options", [dict(), dict(render_streams=3, in_flight=1)], ids=["lone", "in_flight"])
def test_redo_camera_redoes_some_samples(options):
    spp = 9
    ref, ref_seg = oracle("redo", spp)
    img, seg, (ground, redone), _ = device_frame("redo", spp, options)
    print(f"redo camera: {ground} ground samples, {redone} redone ({100.0 * redone / max(ground, 1):.1f}%)")
    assert_bits(img, ref, "redo camera")
    assert seg == ref_seg
    assert ground == GROUND_TILES["redo"] * 64 * spp
    assert 0 < redone < ground


def test_several_passes():
    """max_workspace_bytes for 8-sample passes: the later passes start at sample_begin > 0. (Single
    samples: under a cap the ring's passes would take sample pairs first, which have no tile classes.)"""
    spp = 33
    cap = 3 * (8 * W * H * 12 + (256 << 10)) + 2 * W * H * 12
    img, seg, (ground, _), usage = device_frame("reference", spp, dict(render_streams=3, max_workspace_bytes=cap, no_pairs=1))
    print("usage", usage)
    assert usage["pass_samples"] < spp and usage["pair_passes"] == 0
    assert_bits(img, oracle("reference", spp)[0], "reference spp 33 in several passes")
    assert seg == oracle("reference", spp)[1]
    assert ground == 20 * 64 * spp


def test_row_share_not_a_multiple_of_8(opts):
    """Rows 1, 3, 5, ... (36 rows: four tile rows and four untiled rows, 7 ground tiles) and rows
    1, 5, 9, ... (18 rows: two tile rows and two untiled rows, 5 ground tiles): the untiled blocks
    stay in the main launch, in a group of their own behind the ground range."""
    spp = 5
    opts.set(**LONE_SPLIT)
    for ro, rs in ((1, 2), (1, 4)):
        p = rt.make_params(W, H, spp, DEPTH, SEED, row_offset=ro, row_stride=rs)
        ref = oracle("reference", spp)[0][ro::rs]
        n_ground = rt.tile_ground(scene(), p, CAMERAS["reference"]())
        print(f"rows {ro}::{rs}: {n_ground} ground tiles")
        assert n_ground > 0
        got, st = rt.render_f32(scene(), p, CAMERAS["reference"]())
        assert_bits(got, ref, f"rows {ro}::{rs}")
        assert st.segments == oracle("reference", spp, row_offset=ro, row_stride=rs)[1]


@pytest.mark.parametrize("what", ["metal ground", "max_depth 0", "max_depth 1", "no_sky"])
def test_fallbacks_are_exact(what, opts):
    spp = 5
    depth = {"max_depth 0": 0, "max_depth 1": 1}.get(what, DEPTH)
    which = "metal" if what == "metal ground" else "huge"
    if what == "no_sky":
        opts.set(no_sky=True)
    ref, ref_seg = oracle("reference", spp, depth, which)
    img, st = rt.render_f32(scene(which), rt.make_params(W, H, spp, depth, SEED), CAMERAS["reference"]())
    assert_bits(img, ref, what)
    assert st.segments == ref_seg
    ds_opts = dict(no_sky=1) if what == "no_sky" else {}
    _, _, (ground, redone), _ = device_frame("reference", spp, ds_opts, depth, which)
    assert (ground, redone) == (0, 0)


def test_fast_variant_within_its_tolerance(opts):
    """The tolerance of tests/test_gpu_parity.py's fast-variant test, on a frame with ground tiles."""
    spp = 33
    opts.set(**LONE_SPLIT)
    ref = oracle("reference", spp)[0]
    img, _ = rt.render_f32(scene(), rt.make_params(W, H, spp, DEPTH, SEED, fast_math=True), CAMERAS["reference"]())
    d = np.abs(img - ref)
    frac = float((d.max(axis=-1) <= FAST_TOL_PIX).mean())
    print(f"fast variant: {frac:.4%} of pixels within {FAST_TOL_PIX}, mean |d| {d.mean():.3g}")
    assert frac >= FAST_TOL_FRAC and float(d.mean()) <= FAST_TOL_MEAN and np.isfinite(img).all()


def test_device_order_gives_the_same_ground_range():
    """tile_classes = 1: the order computed by the device's kernels."""
    spp = 5
    img, seg, (ground, redone), _ = device_frame("redo", spp, dict(tile_classes=1))
    assert_bits(img, oracle("redo", spp)[0], "redo camera, the device's order")
    assert seg == oracle("redo", spp)[1]
    assert ground == GROUND_TILES["redo"] * 64 * spp and 0 < redone < ground


@pytest.mark.parametrize("which,camera,depth", [("two_big", "reference", DEPTH), ("two_big", "reference", 2),
                                                 ("huge", "redo", 2)])
def test_two_spheres_in_the_list_and_the_depth_limit(which, camera, depth):
    """An always-tested list of two spheres (the list's loop, the lookup of the hit sphere's shading
    record), and max_depth 2, the smallest depth with the class: a punted sample whose second
    segment hits ends at the limit with colour 0 in the redo launch. (A pass is split only when the
    split depth is below max_depth: deep_split=1 for the depth-2 frames.)"""
    spp = 5
    ref, ref_seg = oracle(camera, spp, depth, which)
    options = dict(render_streams=3, in_flight=1, deep_split=1 if depth == 2 else 8)
    img, seg, (ground, redone), _ = device_frame(camera, spp, options, depth, which)
    print(f"{which} {camera} depth {depth}: {ground} ground samples, {redone} redone")
    assert_bits(img, ref, f"{which} {camera} depth {depth}")
    assert seg == ref_seg
    assert 0 < redone < ground


def test_unsplit_lone_pass_keeps_its_ground_tiles():
    """A lone pass below deep_min_items (the default 2^25 samples) is not split: no ground kernel."""
    spp = 5
    import torch
    ds = rt.DeviceScene(scene(), device=0)
    try:
        out = torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda:0")
        ds.render(CAMERAS["reference"](), rt.make_params(W, H, spp, DEPTH, SEED), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert_bits(out.cpu().numpy(), oracle("reference", spp)[0], "unsplit lone pass")
        assert ds.ground_counts() == (0, 0)
    finally:
        ds.close()
