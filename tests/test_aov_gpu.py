"""First-hit feature buffers on the GPU (rt_render_aov / rt_render_aov_device)
against the per-sample CPU reference (tests/tools/aov_ref.cpp over oracle/rt_oracle.cpp).

Every comparison is on uint32 views (signed zeros count), over all five planes, with zero
mismatches allowed. The references are computed once per module and shared.
"""
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
from support import assert_all_bits, assert_bits, words as u32  # noqa: E402

pytestmark = pytest.mark.gpu

PLANES = tuple(abi.AOV_PLANES)
SEED = 1234


def assert_same(got, ref, planes=PLANES):
    assert_all_bits(got, ref, "planes", planes)


@functools.lru_cache(maxsize=None)
def simple():
    return rt.simple_scene_arrays()


@functools.lru_cache(maxsize=None)
def huge():
    return rt.huge_scene_arrays(SEED)


def bubble_camera(mode):
    return rt.Camera((-2, 1, 0), (0, 1, 0), (0, 1, 0), 2.0, 90.0, .0625, 1.0, mode)


# the two culled cases: (scene, W, H, camera mode, spp, samples)
CASES = {4: (64, 36, rt.REFERENCE, 4, 4), 5: (128, 72, rt.CORRECTED, 8, 5)}


def case_args(n, **params):
    W, H, mode, spp, samples = CASES[n]
    return rt.make_params(W, H, spp, 64, SEED, **params), rt.Camera.default(W, H, mode), samples


@functools.lru_cache(maxsize=None)
def case_ref(n):
    p, cam, samples = case_args(n)
    return aov_ref.render(*huge(), cam, p, samples, sample_ids=True)


@pytest.fixture(scope="module")
def case_gpu():
    """The culled cases rendered under the default options, once (requested before a test changes
    the options)."""
    out = {}
    for n in CASES:
        p, cam, samples = case_args(n)
        out[n] = rt.render_aov(huge(), p, cam, samples)
    return out


# ---- 1-3: the simple scene (brute force: no clusters) -----------------------------------------
@pytest.mark.parametrize("mode", [rt.REFERENCE, rt.CORRECTED])
@pytest.mark.parametrize("spp,samples", [(1, 1), (4, 4), (7, 7), (7, 3)])
def test_simple_scene_blocked_sum(spp, samples, mode):
    """Full blocks of 4, the tail, and samples < spp (keys over the frame's spp)."""
    W, H = 64, 32
    p, cam = rt.make_params(W, H, spp, 64, SEED), rt.Camera.default(W, H, mode)
    got = rt.render_aov(simple(), p, cam, samples)
    ref = aov_ref.render(*simple(), cam, p, samples)
    assert got["albedo"].shape == (H, W, 3) and got["depth"].shape == (H, W) and got["sphere_id"].dtype == np.uint32
    assert_same(got, ref)
    assert (ref["sphere_id"] != 0xffffffff).any() and (ref["sphere_id"] == 0xffffffff).any()


def test_partial_last_block():
    """37 x 19: 703 pixels, no multiple of 64: natural order, a partial last wave."""
    W, H, spp = 37, 19, 7
    p, cam = rt.make_params(W, H, spp, 64, SEED), rt.Camera.default(W, H)
    assert_same(rt.render_aov(simple(), p, cam), aov_ref.render(*simple(), cam, p))


@pytest.mark.parametrize("mode", [rt.REFERENCE, rt.CORRECTED])
def test_bubble_camera(mode):
    """From inside the hollow glass ball: negative radius (flipped normal), far root."""
    W, H, spp = 64, 32, 4
    p, cam = rt.make_params(W, H, spp, 64, SEED), bubble_camera(mode)
    got = rt.render_aov(simple(), p, cam)
    ref = aov_ref.render(*simple(), cam, p)
    assert (ref["sphere_id"] == 4).all() and (ref["alpha"] == 1).all()
    assert_same(got, ref)


# ---- 4-5: the huge scene (culled walk, tile classes, sky blocks) -------------------------------
def test_huge_scene_reference_camera(case_gpu):
    """64 x 36: 8x8 tiles and leftover rows; sky blocks; every material kind among the first hits."""
    p, cam, _ = case_args(4)
    perm, _, n_sky = rt.tile_order(huge(), p, cam)
    assert len(perm) == 36 and n_sky > 0
    ref = case_ref(4)
    ids = ref["sample_ids"]
    s, m = huge()
    kinds = set(m["kind"][s["material"][ids[ids != 0xffffffff]]].tolist())
    assert kinds == {abi.RT_LAMBERT, abi.RT_METAL, abi.RT_DIELECTRIC}
    partial = int(np.count_nonzero((ref["alpha"] > 0) & (ref["alpha"] < 1)))
    print("pixels with 0 < alpha < 1:", partial)
    assert partial > 0
    assert_same(case_gpu[4], ref)


def test_huge_scene_corrected_camera_sample_prefix(case_gpu):
    """128 x 72, corrected camera, samples 5 of spp 8."""
    p, cam, _ = case_args(5)
    perm, _, n_sky = rt.tile_order(huge(), p, cam)
    assert len(perm) == 144 and n_sky > 0
    ref = case_ref(5)
    distinct = np.unique(ref["sphere_id"][ref["sphere_id"] != 0xffffffff])
    print("distinct first-hit spheres:", len(distinct))
    assert len(distinct) > 100
    assert_same(case_gpu[5], ref)


# ---- 6: same bits under options ----------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(CASES))
@pytest.mark.parametrize("variant", ["brute_force", "natural_order", "no_sky", "ieee_roots", "shade_global"])
def test_same_bits_under_options(n, variant, case_gpu, opts):
    p, cam, samples = case_args(n, brute_force=True) if variant == "brute_force" else case_args(n)
    if variant != "brute_force":
        opts.set(**{variant: True})
    got = rt.render_aov(huge(), p, cam, samples)
    assert_same(got, case_gpu[n])
    assert_same(got, case_ref(n))


# ---- 7: rows and planes ------------------------------------------------------------------------
def test_row_fields_packed(case_gpu):
    p, cam, samples = case_args(4, row_offset=1, row_stride=2)
    got = rt.render_aov(huge(), p, cam, samples)
    assert got["albedo"].shape == (18, 64, 3)
    assert_same(got, {n: case_gpu[4][n][1::2] for n in PLANES})


def _device_planes(torch, rows, W, fill):
    """One device buffer holding the five planes with a guard region before, between and after
    them, every word set to `fill`: (buffer, {plane: word offset}, {plane: words})."""
    guard, at, words, total = 256, {}, {}, 256
    for n, (ch, _, _) in abi.AOV_PLANES.items():
        at[n], words[n] = total, rows * W * ch
        total += words[n] + guard
    buf = torch.full((total,), fill, dtype=torch.int32, device="cuda:0")
    return buf, at, words


def _plane(buf_np, at, words, n, rows, W):
    ch, dt, _ = abi.AOV_PLANES[n]
    a = buf_np[at[n]:at[n] + words[n]].view(dt)
    return a.reshape((rows, W, ch) if ch > 1 else (rows, W))


SENTINEL = 0x5a5a5a5a


def test_row_fields_full_frame_keeps_untouched_rows(case_gpu):
    import torch
    p, cam, samples = case_args(4, row_offset=1, row_stride=2, full_frame=True)
    W, H = p.width, p.height
    buf, at, words = _device_planes(torch, H, W, SENTINEL)
    ds = rt.DeviceScene(huge(), device=0)
    try:
        ds.render_aov(cam, p, {n: buf.data_ptr() + 4 * at[n] for n in PLANES}, samples,
                      torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        ds.close()
    host = buf.cpu().numpy().view(np.uint32)
    got = {n: _plane(host, at, words, n, H, W) for n in PLANES}
    assert_same({n: got[n][1::2] for n in PLANES}, {n: case_gpu[4][n][1::2] for n in PLANES})
    for n in PLANES:
        assert (u32(got[n][0::2]) == SENTINEL).all(), n
    written = np.zeros(host.size, dtype=bool)
    for n in PLANES:
        written[at[n]:at[n] + words[n]] = True
    assert (host[~written] == SENTINEL).all()  # the guard regions


def test_only_requested_planes_are_written(case_gpu):
    import torch
    p, cam, samples = case_args(4)
    W, H = p.width, p.height
    buf, at, words = _device_planes(torch, H, W, SENTINEL)
    wanted = ("depth", "sphere_id")
    ds = rt.DeviceScene(huge(), device=0)
    try:
        ds.render_aov(cam, p, {n: buf.data_ptr() + 4 * at[n] for n in wanted}, samples,
                      torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        ds.close()
    host = buf.cpu().numpy().view(np.uint32)
    assert_same({n: _plane(host, at, words, n, H, W) for n in wanted}, case_gpu[4], wanted)
    written = np.zeros(host.size, dtype=bool)
    for n in wanted:
        written[at[n]:at[n] + words[n]] = True
    assert (host[~written] == SENTINEL).all()


# ---- 8: against the beauty on the GPU -------------------------------------------------------------
def test_miss_albedo_is_the_gpu_beauty(case_gpu):
    p, cam, _ = case_args(4)
    beauty, _ = rt.render_f32(huge(), p, cam)
    miss = case_gpu[4]["alpha"] == 0
    assert int(miss.sum()) >= 1000
    assert np.array_equal(u32(case_gpu[4]["albedo"])[miss], u32(beauty)[miss])


# ---- 9: ordering with frames in flight --------------------------------------------------------------
def test_ordered_between_beauty_frames_in_flight(case_gpu):
    """Beauty frame, feature buffers, beauty frame on one scene and one stream, no host sync between
    them: each equals its stand-alone result."""
    import torch
    p, cam, samples = case_args(4)
    W, H = p.width, p.height
    p2 = rt.make_params(W, H, p.spp, 64, SEED + 1)
    alone = [rt.render_f32(huge(), q, cam)[0] for q in (p, p2)]
    st = torch.cuda.Stream()
    buf, at, words = _device_planes(torch, H, W, SENTINEL)
    frames = [torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    ds = rt.DeviceScene(huge(), device=0)
    try:
        ds.render(cam, p, frames[0].data_ptr(), st.cuda_stream)
        ds.render_aov(cam, p, {n: buf.data_ptr() + 4 * at[n] for n in PLANES}, samples, st.cuda_stream)
        ds.render(cam, p2, frames[1].data_ptr(), st.cuda_stream)
        st.synchronize()
    finally:
        ds.close()
    host = buf.cpu().numpy().view(np.uint32)
    assert_same({n: _plane(host, at, words, n, H, W) for n in PLANES}, case_gpu[4])
    for f, ref in zip(frames, alone):
        assert_bits(f.cpu().numpy(), ref)


def test_stats_of_the_host_call():
    import ctypes as C
    s, m = simple()
    W, H, spp, samples = 64, 32, 7, 3
    p, cam = rt.make_params(W, H, spp, 64, SEED, row_offset=2, row_stride=3), rt.Camera.default(W, H).c
    rows = abi.rows_of(p)
    depth = np.zeros((rows, W), dtype=np.float32)
    rec = rt.render.aov_buffers({"depth": depth.ctypes.data}, samples)
    st = abi.RtStats()
    rt.render.check(rt.lib().rt_render_aov(abi.ptr(s, C.POINTER(abi.RtSphere)), len(s),
                                           abi.ptr(m, C.POINTER(abi.RtMaterial)), len(m), C.byref(cam), C.byref(p),
                                           C.byref(rec), C.byref(st)))
    assert st.primaries == st.segments == W * rows * samples
    assert st.sphere_tests == 0 and st.box_tests == 0 and st.kernel_ms > 0 and st.wall_ms >= st.kernel_ms
    ref = aov_ref.render(s, m, cam, p, samples)
    assert_bits(depth, ref["depth"])
