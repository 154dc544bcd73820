"""64-bit seeds and stream keys past 2^32 in every kernel (cases: tests/tools/wide_cases.py).

Each sample's two PCG32 streams are seeded from key = (y W + x) spp + s with increments made of the
64-bit seed; the kernels restate that arithmetic in several places (render_kernel's fresh samples
and rejection loop, sky_kernel's stepped products, the wavefront generator, aov_kernel, the moments
accumulation, ground_kernel's sums cd1, cd2, cd3 and steps M, M^2, M^3 from its own key0, and
render_list_kernel's key rebuilt from a slot word of the redo list) and carry a path's 64-bit state
through the deep queue and the wavefront ray queues.
The other GPU suites keep the key, both increments' high words and the pixel index's top bit at
zero. Here bands of a 8192 x 524280 frame (keys 2^33.4 .. 2^34.0, every pixel index >= 2^31) with
seed 1234 + 2^32, and the small frame with seeds up to 2^64 - 1, are rendered through every path and
compared with the CPU restatement, which tests/test_oracle_golden.py pins to the reference itself
on such words; tests/test_wide_words_cpu.py fixes that the cases reach what they are meant to.

Every comparison is on uint32 views with zero mismatches allowed, and the segment count equals the
restatement's wherever the render reports one. A render is at most 16 x 8192 x 5 samples.

The ground kernel and the redo launch run in split passes with ground tiles only,
which none of the cases above has: section 8 renders the `ground` band (817 ground tiles beside lead
and sky tiles), the small frame (4 ground tiles) and the redo frame (85 ground tiles, a tenth of
their samples redone, under the wide seeds) in flight and as a lone split pass, and asserts
the scene's ground counts, so that a frame that fell back to the main launch fails.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi
from raytracinginoneweekend_amd import render as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import wide_cases as WC  # noqa: E402
from support import assert_all_bits, assert_bits, words as u32  # noqa: E402

pytestmark = pytest.mark.gpu

PLANES = tuple(abi.AOV_PLANES)
SENTINEL = 0x5a5a5a5a

# name -> (scene, camera, params(**kw), reference (image, segments), options every variant starts from).
# The deep band's passes are far smaller than rt_options.deep_min_items, below which a pass issued
# alone is not split: 0 there, so that its long paths go through the deep queue and the deep launch.
CASES = {}
for _band, _mode in WC.BAND_MODES:
    if _band != "ground":  # (section 8's)
        CASES[f"{_band}-{_mode}"] = dict(band=_band, mode=_mode, base=dict(deep_min_items=0) if _band == "deep" else {})
for _name in WC.SEEDS:
    CASES[f"small-{_name}"] = dict(seed=WC.SEEDS[_name], base={})


def case_camera(name):
    c = CASES[name]
    return WC.camera(c["mode"]) if "band" in c else WC.small_camera()


def case_params(name, **kw):
    c = CASES[name]
    return WC.params(c["band"], **kw) if "band" in c else WC.small_params(c["seed"], **kw)


def case_ref(name):
    c = CASES[name]
    return WC.band_ref(c["band"], c["mode"])[:2] if "band" in c else WC.small_ref(c["seed"])


# options of the variant (rt_options fields and diag bits); _flags: rt_params flags; _count: with the
# segment counters (the counting instantiation); _passes: a max_pass_bytes that cuts the samples
VARIANTS = {
    "default": {},
    "counting": dict(_count=True),
    "wavefront": dict(_flags=dict(wavefront=True), _count=True),
    "brute_force": dict(_flags=dict(brute_force=True), _count=True),
    "scalar_scene": dict(_flags=dict(scalar_scene=True), _count=True),
    "instrumented": dict(stats=True, _count=True),
    "natural_order": dict(natural_order=True),
    "no_sky": dict(no_sky=True),
    "two_passes": dict(_passes=True, _count=True),
    "pairs": dict(pairs=True, in_flight=True),
    "one_stream": dict(render_streams=1),
    "tile_classes": dict(tile_classes=1),
}


def render_device(scene, cam, p, count=False, out=None, out_ptr=None):
    """One rt_render_device call on a fresh scene made with the process-default options (the opts
    fixture's): (frame as uint32 (rows, W, 3), segments or None, rt_scene_usage, word [15] of
    rt_scene_debug_counters: the instrumented kernel's first bounds violation, 0 = none). The frame
    comes back as the words of a buffer filled with an integer sentinel; the float32 references are
    compared as u32(ref), the same bytes under that dtype."""
    import torch
    rows = p.height if p.flags & abi.RT_FLAG_FULL_FRAME else abi.rows_of(p)
    if out is None:
        out = torch.full((rows, p.width, 3), SENTINEL, dtype=torch.int32, device="cuda:0")
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda:0") if count else None
    ds = rt.DeviceScene(scene, device=0)
    try:
        ds.render(cam, p, out_ptr or out.data_ptr(), torch.cuda.current_stream().cuda_stream,
                  cnt.data_ptr() if count else None)
        torch.cuda.synchronize()
        usage = ds.usage()
        dbg = (C.c_uint64 * 16)()
        R.check(rt.lib().rt_scene_debug_counters(ds.handle, dbg, 1))
    finally:
        ds.close()
    return out.cpu().numpy().view(np.uint32), int(cnt[0]) if count else None, usage, int(dbg[15])


# ---- 1. the beauty through every path ----------------------------------------------------------
# (a pass holds at least 4 samples: the small frame's 4 spp cannot be cut, the bands' 5 spp can)
BEAUTY = [(n, v) for n in CASES for v in VARIANTS if not (v == "two_passes" and n.startswith("small-"))]


@pytest.mark.parametrize("name,variant", BEAUTY)
def test_beauty_matches_restatement(name, variant, opts):
    v = dict(VARIANTS[variant])
    flags, count, passes = v.pop("_flags", {}), v.pop("_count", False), v.pop("_passes", False)
    p, cam = case_params(name, **flags), case_camera(name)
    n_pixels = abi.rows_of(p) * p.width
    if passes:  # a pass of 4 samples, then one of the fifth: sample_begin = 4 there
        v["max_pass_bytes"] = n_pixels * 12 * 4
    opts.set(**CASES[name]["base"], **v)
    ref, ref_seg = case_ref(name)
    got, seg, usage, violation = render_device(WC.scene(), cam, p, count)
    assert_bits(got, u32(ref), f"{name} {variant}")
    if count:
        assert seg == ref_seg
    assert violation == 0
    if passes:
        assert 0 < usage["pass_samples"] < p.spp, usage
    if variant == "pairs":
        assert usage["pair_passes"] >= 1, usage
    if variant in ("default", "tile_classes") and name == "split-reference":
        assert usage["lead_tiles"] > 0 and usage["sky_tiles"] > 0, usage  # the tile classes split this band
    if variant in ("default", "counting") and name == "deep-corrected":
        assert usage["split_passes"] >= 1 and usage["deep_launch"] != 0, usage


def test_lone_split_pass_of_the_deep_band_takes_the_deep_launch(opts):
    """As tests/test_gpu_trap.py::test_lone_split_pass_takes_the_deep_launch: shading records in
    global memory, split after 2 segments: the 8-wave deep launch, the restatement's frame and
    segments."""
    opts.set(deep_min_items=0, shade_global=True, deep_split=2)
    ref, ref_seg = case_ref("deep-corrected")
    got, seg, usage, _ = render_device(WC.scene(), case_camera("deep-corrected"), case_params("deep-corrected"), True)
    assert usage["deep_launch"] == 8 | 16 and usage["split_passes"] >= 1, usage
    assert_bits(got, u32(ref), "deep band, lone split pass")
    assert seg == ref_seg


# ---- 2. the other stages -------------------------------------------------------------------------
def _stage_case(which):
    if which == "split":
        return (WC.camera("reference"), WC.params("split"), WC.band_aov_ref("split", "reference"),
                WC.band_moments_ref("split", "reference"))
    return WC.small_camera(), WC.small_params(WC.SEED), WC.small_aov_ref(WC.SEED), WC.small_moments_ref(WC.SEED)


@pytest.mark.parametrize("which", ["split", "small", "deep"])
def test_feature_buffers_match_reference(which):
    """aov_kernel seeds its own copy of the streams: all five planes against tests/tools/aov_ref, on
    the split band, the small frame and (no sky blocks: every pixel a surface) the deep band under
    the corrected camera."""
    if which == "deep":
        cam, p, ref = WC.camera("corrected"), WC.params("deep"), WC.band_aov_ref("deep", "corrected")
        assert (ref["alpha"] == 1).all()
    else:
        cam, p, ref, _ = _stage_case(which)
        assert (ref["alpha"] == 0).any() and (ref["alpha"] == 1).any()
    got = rt.render_aov(WC.scene(), p, cam)
    assert_all_bits(got, ref, which, PLANES)


@pytest.mark.parametrize("which", ["split", "small"])
def test_variance_render_matches_reference(which):
    """rt_render_var (the moments build of the accumulation) against tests/tools/moments_ref."""
    cam, p, _, (ref_rgb, ref_var) = _stage_case(which)
    rgb, var, _ = rt.render_var(WC.scene(), p, cam)
    assert_bits(rgb, ref_rgb, f"{which} render_var rgb")
    assert_bits(var, ref_var, f"{which} render_var variance")
    assert (ref_var > 0).any()


# ---- 3. row partitions of the deep band --------------------------------------------------------------
def test_row_partitions_of_the_deep_band(opts):
    """The deep band (corrected camera) as one call, as two calls of half its rows, packed and with
    RT_FLAG_FULL_FRAME: the same bits at those keys. A full-frame buffer of this frame would be 51 GB;
    the full-frame calls get the address the frame's row 0 would have if the band's rows lay where the
    buffer is (the kernel writes the rendered rows only, each at ((size_t)y W + x) 3 floats from the
    base, an offset past 2^32 floats), with guard rows around the band."""
    import torch
    opts.set(deep_min_items=0)
    name = "deep-corrected"
    ref, _ = case_ref(name)
    cam, scene = case_camera(name), WC.scene()
    n = WC.BANDS["deep"]["num_rows"]
    halves = [(0, n // 2), (n // 2, n - n // 2)]
    whole, _, usage, _ = render_device(scene, cam, case_params(name))
    assert usage["split_passes"] >= 1
    assert_bits(whole, u32(ref), "one call")
    parts = [render_device(scene, cam, case_params(name, rows=h))[0] for h in halves]
    assert_bits(np.concatenate(parts), u32(ref), "two calls of half the rows")
    guard, y0 = 2, WC.BANDS["deep"]["row_offset"]
    row_bytes = WC.W * 12
    for calls in ([(0, n)], halves):
        buf = torch.full((n + 2 * guard, WC.W, 3), SENTINEL, dtype=torch.int32, device="cuda:0")
        base = buf.data_ptr() + guard * row_bytes - y0 * row_bytes
        assert base > 0
        for h in calls:
            got = render_device(scene, cam, case_params(name, rows=h, full_frame=True), out=buf, out_ptr=base)[0]
        assert_bits(got[guard:guard + n], u32(ref), f"full frame, {len(calls)} call(s)")
        assert (got[:guard] == SENTINEL).all() and (got[guard + n:] == SENTINEL).all()


# ---- 4. seeds equal modulo 2^62 ------------------------------------------------------------------
@pytest.mark.parametrize("seed", [WC.BASE_SEED, WC.SEED])
def test_seed_aliases_render_equal_bits(seed):
    """Seed s and s + 2^62 (and s + 2^63) give equal bits: include/rt_api.h rt_params.seed."""
    cam = WC.small_camera()
    a = render_device(WC.scene(), cam, WC.small_params(seed))[0]
    for k in (62, 63):
        b = render_device(WC.scene(), cam, WC.small_params((seed + 2 ** k) % 2 ** 64))[0]
        assert_bits(b, a, f"seed {seed} + 2^{k}")
    cam, p = WC.camera("reference"), WC.params("split", seed=WC.SEED + 2 ** 62)
    assert_bits(render_device(WC.scene(), cam, p)[0], u32(WC.band_ref("split", "reference")[0]), "split band, SEED + 2^62")


# ---- 5. the reference's CUDA variant: a 32-bit engine ------------------------------------------------
def test_cuda_compat_seed_is_taken_modulo_2_32():
    s, m = WC.compat_scene()
    cam = rt.Camera.cuda(64, 36)
    a, sa = rt.render_f32((s, m), rt.make_params(64, 36, 4, 32, 7, cuda_compat=True), cam)
    b, sb = rt.render_f32((s, m), rt.make_params(64, 36, 4, 32, 7 + 2 ** 32, cuda_compat=True), cam)
    assert_bits(b, a, "seed 7 + 2^32 against seed 7")
    assert sa.segments == sb.segments and a.any()


def test_cuda_compat_state_wraps_inside_the_band():
    """The last 8 rows of the frame with seed 100000: x + y W + seed passes 2^32 in the band."""
    ref, ref_seg = WC.compat_ref()
    got, st = rt.render_f32(WC.compat_scene(), WC.compat_params(), rt.Camera.cuda(WC.W, WC.H))
    assert_bits(got, ref, "cuda-compat band")
    assert st.segments == ref_seg


# ---- 6. the preview session ------------------------------------------------------------------------
def test_preview_frame_is_the_stage_calls_with_a_wide_seed():
    """One rt.Preview frame with seed 1234 + 2^32 equals the five stage calls made by hand with that
    seed (tests/test_preview_gpu.py::test_chain_equality at its smallest size, first frame)."""
    import torch
    w, h, spp = WC.SMALL
    depth, seed = 8, WC.SEED
    cam = WC.small_camera("corrected")
    pp = rt.preview_params(w, h, spp, flags=0, max_depth=depth, denoise=dict(levels=2))

    def plane(ch, dtype=torch.float32):
        return torch.full((h, w, ch) if ch > 1 else (h, w), -7.0, dtype=dtype, device="cuda:0")

    ds = rt.DeviceScene(WC.scene(), device=0)
    try:
        st = torch.cuda.Stream()
        rgb, rgb8 = plane(3), torch.full((h, w, 3), 77, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        pv = ds.preview(pp)
        pv.frame(cam, seed, rgb.data_ptr(), rgb8.data_ptr(), st.cuda_stream)
        st.synchronize()
        pv.close()
        beauty, variance, albedo, alpha = plane(3), plane(1), plane(3), plane(1)
        g = dict(normal=plane(3), depth=plane(1), sphere_id=plane(1, torch.int32))
        hist = dict(color=plane(3), variance=plane(1), history=plane(1))
        out, scratch, var_scratch = plane(3), plane(3), plane(2)
        tex = torch.full((h, w, 3), 77, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        rp = rt.make_params(w, h, spp, depth, seed)
        ds.render_var(cam, rp, beauty.data_ptr(), variance.data_ptr(), st.cuda_stream)
        ds.render_aov(cam, rp, dict(albedo=albedo.data_ptr(), alpha=alpha.data_ptr(), **{n: a.data_ptr() for n, a in g.items()}),
                      0, st.cuda_stream)
        ptrs = dict(beauty=beauty, variance=variance, alpha=alpha, **g, out_color=hist["color"],
                    out_variance=hist["variance"], out_history=hist["history"])
        rt.temporal_device({n: a.data_ptr() for n, a in ptrs.items()}, pp.temporal, cam, None, st.cuda_stream)
        rt.denoise_var_device(dict(beauty=hist["color"].data_ptr(), albedo=albedo.data_ptr(), normal=g["normal"].data_ptr(),
                                   depth=g["depth"].data_ptr(), out=out.data_ptr(), scratch=scratch.data_ptr()), pp.denoise,
                              R.denoise_var_buffers(dict(variance=hist["variance"].data_ptr(),
                                                         var_scratch=var_scratch.data_ptr()), pp.var_floor), st.cuda_stream)
        rt.epilogue_rgb8_device(out.data_ptr(), tex.data_ptr(), w * h, st.cuda_stream)
        st.synchronize()
    finally:
        ds.close()
    assert_bits(rgb.cpu().numpy(), out.cpu().numpy(), "preview rgb")
    assert np.array_equal(rgb8.cpu().numpy(), tex.cpu().numpy())
    # the hand-made chain started from this seed's streams: its beauty is the public call's, which
    # differs from seed 1234's
    want, _, _ = rt.render_var(WC.scene(), rt.make_params(w, h, spp, depth, seed), cam)
    assert_bits(beauty.cpu().numpy(), want, "beauty of the chain")
    other, _, _ = rt.render_var(WC.scene(), rt.make_params(w, h, spp, depth, WC.BASE_SEED), cam)
    assert np.count_nonzero(u32(other) != u32(want)) > want.size // 2


# ---- 7. the dealing order of the split band ------------------------------------------------------------
@pytest.mark.parametrize("tile_classes", [0, 1])
def test_tile_order_of_the_split_band(tile_classes):
    """DeviceScene.tile_order gives the host's permutation and counts at rows 270000 .. 417000 of a
    524280-row frame."""
    cam, p = WC.camera("reference"), WC.params("split")
    want, wl, ws = rt.tile_order(WC.scene(), p, cam)
    ds = rt.DeviceScene(WC.scene(), device=0, options=rt.options(rt.default_options(), tile_classes=tile_classes))
    try:
        got, gl, gs = ds.tile_order(cam, p)
    finally:
        ds.close()
    print("blocks", len(want), "lead", wl, "sky", ws, "| device lead", gl, "sky", gs)
    assert wl > 0 and ws > 0 and (gl, gs) == (wl, ws)
    assert got.dtype == np.uint32 and got.shape == want.shape and np.array_equal(got, want)


# ---- 8. the ground kernel and the redo launch ------------------------------------------------------------
IN_FLIGHT = dict(render_streams=3, in_flight=1)  # every launch of a pass on the pass's stream
LONE_SPLIT = dict(deep_min_items=1)              # a pass issued alone is split: the ground kernel on a stream of its own
# _count, _passes as in VARIANTS; _seed: another seed than the band's
GROUND_VARIANTS = {
    "in_flight": dict(IN_FLIGHT),
    "lone_split": dict(LONE_SPLIT),
    "counting": dict(IN_FLIGHT, _count=True),
    "instrumented": dict(LONE_SPLIT, stats=True, _count=True),
    "two_passes": dict(IN_FLIGHT, _passes=True, _count=True),
    "tile_classes": dict(IN_FLIGHT, tile_classes=1),
    "seed_alias": dict(IN_FLIGHT, _seed=WC.SEED + 2 ** 62),
}


def render_ground(scene, cam, p, options, count=False):
    """One rt_render_device call on a fresh scene with `options`: (frame as uint32, segments or None,
    rt_scene_usage, the instrumented kernels' first bounds violation, (ground samples, redone))."""
    import torch
    out = torch.full((abi.rows_of(p), p.width, 3), SENTINEL, dtype=torch.int32, device="cuda:0")
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda:0") if count else None
    ds = rt.DeviceScene(scene, device=0, options=rt.options(rt.default_options(), **options))
    try:
        ds.render(cam, p, out.data_ptr(), torch.cuda.current_stream().cuda_stream, cnt.data_ptr() if count else None)
        torch.cuda.synchronize()
        usage, counts = ds.usage(), ds.ground_counts()
        dbg = (C.c_uint64 * 16)()
        R.check(rt.lib().rt_scene_debug_counters(ds.handle, dbg, 1))
    finally:
        ds.close()
    return out.cpu().numpy().view(np.uint32), int(cnt[0]) if count else None, usage, int(dbg[15]), counts


@pytest.mark.parametrize("variant", list(GROUND_VARIANTS))
def test_ground_band_matches_restatement(variant):
    """The ground band under the reference camera: 817 tiles x 64 pixels x 5 samples through
    ground_kernel at keys past 2^33 and pixel indices past 2^31, part of them redone by
    render_list_kernel (scattered rays that pass the box over the field), part not (the ground
    tiles' sky samples never are: tests/test_wide_words_cpu.py::test_ground_band_census)."""
    v = dict(GROUND_VARIANTS[variant])
    count, passes, seed = v.pop("_count", False), v.pop("_passes", False), v.pop("_seed", WC.SEED)
    p, cam = WC.params("ground", seed=seed), WC.camera("reference")
    if passes:  # a pass of 4 samples, then one of the fifth: sample_begin = 4 there
        v["max_pass_bytes"] = abi.rows_of(p) * p.width * 12 * 4
    ref, ref_seg, _ = WC.band_ref("ground", "reference")
    n_ground = WC.band_tiles("ground", "reference")[2]
    got, seg, usage, violation, (ground, redone) = render_ground(WC.scene(), cam, p, v, count)
    print(f"ground band, {variant}: {ground} ground samples, {redone} redone, usage {usage}")
    assert_bits(got, u32(ref), f"ground band, {variant}")
    if count:
        assert seg == ref_seg
    assert violation == 0
    if passes:
        assert 0 < usage["pass_samples"] < p.spp, usage
    assert usage["lead_tiles"] > 0 and usage["sky_tiles"] > 0 and usage["split_passes"] >= 1, usage
    assert n_ground >= 64 and ground == n_ground * 64 * WC.SPP
    assert 0 < redone < ground


@pytest.mark.parametrize("name", ["hi32", "max", "bit63", "alias62"])
def test_small_frame_ground_tiles_with_wide_seeds(name):
    """The small frame's 4 ground tiles in flight: the increments' high words (hi32), every bit set
    (max), bit 63 of an increment (bit63), and a seed past 2^62 that names seed 1234's streams."""
    seed = WC.SEEDS[name]
    ref, ref_seg = WC.small_ref(seed)
    got, seg, _, _, (ground, redone) = render_ground(WC.scene(), WC.small_camera(), WC.small_params(seed), IN_FLIGHT, True)
    print(f"small frame, seed {name}: {ground} ground samples, {redone} redone")
    assert_bits(got, u32(ref), f"small frame, seed {name}, in flight")
    assert seg == ref_seg
    assert WC.small_ground_tiles() == 4 and ground == 4 * 64 * WC.SMALL[2]
    assert redone <= ground


@pytest.mark.parametrize("name", WC.WIDE_SEEDS)
def test_redo_frame_with_wide_seeds(name):
    """The redo frame in flight: 85 ground tiles, part of whose samples render_list_kernel redoes
    under each wide seed (tests/test_wide_words_cpu.py shows ground samples of three segments and
    more for each), its key rebuilt from the slot word with that seed's increments."""
    seed = WC.SEEDS[name]
    ref, ref_seg = WC.redo_ref(seed)
    got, seg, _, _, (ground, redone) = render_ground(WC.scene(), WC.redo_camera(), WC.redo_params(seed), IN_FLIGHT, True)
    print(f"redo frame, seed {name}: {ground} ground samples, {redone} redone")
    assert_bits(got, u32(ref), f"redo frame, seed {name}, in flight")
    assert seg == ref_seg
    assert ground == 85 * 64 * WC.REDO[2]
    assert 0 < redone < ground
