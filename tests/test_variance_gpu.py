"""The variance render and the variance-guided denoiser on the GPU (rt_render_var*,
rt_denoise_var*) against their CPU references (tests/tools/moments_ref.py,
tests/tools/denoise_var_ref.py).

Every comparison is on uint32 views with zero mismatches allowed. The references are computed once
per module and shared.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import denoise_var_ref  # noqa: E402
import moments_ref  # noqa: E402
from device_io import SENTINEL  # noqa: E402  (other modules read it from here too)
from support import assert_bits as assert_same, frame_planes, synthetic_planes  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SEED = 1234
GUIDES = ("albedo", "normal", "depth")
CAMERAS = {"reference": rt.REFERENCE, "corrected": rt.CORRECTED}


# ---- the render ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "huge":
        return rt.huge_scene_arrays(SEED)
    # glass: small glass balls on the ground in front of the camera (paths trapped in them run deep),
    # a big glass sphere, lambert and metal balls
    rng = np.random.default_rng(5)
    n = 160
    s = np.zeros(n, dtype=abi.SPHERE_DTYPE)
    m = np.zeros(4, dtype=abi.MATERIAL_DTYPE)
    m[0] = (0, [0.5, 0.5, 0.5], 0.0)
    m[1] = (1, [0.7, 0.6, 0.5], 0.05)
    m[2] = (2, [1.0, 1.0, 1.0], 1.5)
    m[3] = (0, [0.8, 0.3, 0.2], 0.0)
    r = rng.choice([0.2, 0.3, 0.15], n).astype(np.float32)
    c = np.zeros((n, 3), dtype=np.float32)
    c[:, 0] = rng.uniform(-6, 6, n)
    c[:, 2] = rng.uniform(-6, 6, n)
    c[:, 1] = r
    s["center"], s["radius"], s["material"] = c, r, rng.choice([2, 2, 2, 0, 1, 3], n)
    s["center"][0], s["radius"][0], s["material"][0] = (0, -1000, 0), 1000.0, 0
    s["center"][1], s["radius"][1], s["material"][1] = (0, 1, 0), 1.0, 2
    return s, m


def params(w, h, spp, seed=SEED, **kw):
    return rt.make_params(w, h, spp, 64, seed, **kw)


_REFS = {}


def reference(scene_name, w, h, spp, mode, seed=SEED, **kw):
    """moments_ref's (rgb, var) of the frame, once; rows the call does not render hold SENTINEL."""
    key = (scene_name, w, h, spp, mode, seed, tuple(sorted(kw.items())))
    if key not in _REFS:
        kw_ref = {k: v for k, v in kw.items() if k != "brute_force"}  # same bits by contract
        p = params(w, h, spp, seed, **kw_ref)
        s, m = scene(scene_name)
        rgb, var, _ = moments_ref.render(s, m, rt.Camera.default(w, h, mode), p)
        if p.flags & abi.RT_FLAG_FULL_FRAME:
            rest = np.ones(h, dtype=bool)
            rest[p.row_offset::p.row_stride or 1] = False
            rgb[rest], var[rest] = F(SENTINEL), F(SENTINEL)
        _REFS[key] = (rgb, var)
    return _REFS[key]


def device_render(scene_name, p, mode, opts=None, plain=False):
    """One frame through DeviceScene.render_var (plain: DeviceScene.render) into buffers filled with
    SENTINEL, on a scene with options `opts`: (rgb, var, rt_scene_usage after the call)."""
    import torch
    rows = p.height if p.flags & abi.RT_FLAG_FULL_FRAME else abi.rows_of(p)
    rgb = torch.full((rows, p.width, 3), SENTINEL, dtype=torch.float32, device="cuda:0")
    var = torch.full((rows, p.width), SENTINEL, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ds = rt.DeviceScene(scene(scene_name), device=0, options=rt.options(**opts) if opts else None)
    try:
        cam = rt.Camera.default(p.width, p.height, mode)
        st = torch.cuda.current_stream().cuda_stream
        if plain:
            ds.render(cam, p, rgb.data_ptr(), st)
        else:
            ds.render_var(cam, p, rgb.data_ptr(), var.data_ptr(), st)
        usage = ds.usage()
        torch.cuda.synchronize()
    finally:
        ds.close()
    return rgb.cpu().numpy(), var.cpu().numpy(), usage


def check_render(scene_name, w, h, spp, mode, opts=None, seed=SEED, **kw):
    ref_rgb, ref_var = reference(scene_name, w, h, spp, mode, seed, **kw)
    rgb, var, usage = device_render(scene_name, params(w, h, spp, seed, **kw), mode, opts)
    print("usage:", usage)
    assert_same(rgb, ref_rgb, "rgb")
    assert_same(var, ref_var, "var")
    assert usage["pair_passes"] == 0 and usage["sky_tiles"] == 0, usage
    return usage


@pytest.mark.parametrize("spp", [2, 7, 16])
@pytest.mark.parametrize("camera", sorted(CAMERAS))
def test_render_matches_the_plain_render_and_the_reference_variance(camera, spp):
    """The huge scene at 64 x 36 through the host call: rgb is rt.render_f32's bit for bit, var is
    moments_ref's."""
    w, h, mode = 64, 36, CAMERAS[camera]
    p, cam = params(w, h, spp), rt.Camera.default(w, h, mode)
    ref_rgb, ref_var = reference("huge", w, h, spp, mode)
    rgb, var, st = rt.render_var(scene("huge"), p, cam)
    plain, plain_st = rt.render_f32(scene("huge"), p, cam)
    assert_same(rgb, plain, "rgb against render_f32")
    assert_same(rgb, ref_rgb, "rgb against the oracle")
    assert_same(var, ref_var, "var")
    assert st.primaries == w * h * spp and st.segments == plain_st.segments and st.kernel_ms > 0
    assert (var > 0).any()


def test_the_sky_path_is_the_one_replaced():
    """The 64 x 36 frame's plain render takes the sky kernel (sky_tiles > 0, no pairs); the variance
    render of the same frame deals those tiles to the main launch."""
    p = params(64, 36, 16)
    _, _, plain = device_render("huge", p, rt.REFERENCE, plain=True)
    assert plain["sky_tiles"] > 0 and plain["pair_passes"] == 0, plain
    usage = check_render("huge", 64, 36, 16, rt.REFERENCE)
    assert usage["lead_tiles"] > 0, usage  # tile classes still order the dealing


# 64 x 36: 27648 slot bytes per sample. PAIRS_CAP: three streams' 16-sample workspaces of single
# samples with their deep queues take 2071296 bytes; under a cap below that the plain render turns to
# pairs (passes of 12 samples), the variance render to shorter passes of single samples.
PAIRS_CAP = dict(render_streams=3, max_workspace_bytes=2000000, in_flight=True)
VARIANTS = {
    "four-passes": ("huge", dict(max_pass_bytes=64 * 36 * 12 * 4), {}),
    "workspace-cap": ("huge", PAIRS_CAP, {}),
    "in-flight": ("huge", dict(in_flight=True), {}),
    "deep-lone": ("glass", dict(deep_min_items=0, deep_split=1), {}),
    "deep-in-flight": ("glass", dict(deep_min_items=0, deep_split=1, in_flight=True), {}),
    "deep-one-stream": ("glass", dict(deep_min_items=0, deep_split=1, render_streams=1), {}),
    "deep-four-passes": ("glass", dict(deep_min_items=0, deep_split=1, max_pass_bytes=64 * 36 * 12 * 4), {}),
    "brute-force": ("huge", None, dict(brute_force=True)),
    "one-stream": ("huge", dict(render_streams=1), {}),
    "one-stream-four-passes": ("huge", dict(render_streams=1, max_pass_bytes=64 * 36 * 12 * 4), {}),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_pass_and_plan_variants(variant):
    """The render check under every cut of the frame: `mom` carried over four passes, a workspace cap
    under which the plain render takes pairs, passes planned as in flight, the deep split at one
    segment on a glass-heavy scene (two-part accumulation for a lone pass, one part otherwise), brute
    force, and everything on the caller's stream."""
    scene_name, opts, kw = VARIANTS[variant]
    usage = check_render(scene_name, 64, 36, 16, rt.REFERENCE, opts, **kw)
    if "four-passes" in variant:
        assert usage["pass_samples"] == 4, usage
    if variant == "workspace-cap":
        assert usage["pass_samples"] < 16 and usage["workspace_bytes"] <= PAIRS_CAP["max_workspace_bytes"], usage
        _, _, plain = device_render("huge", params(64, 36, 16), rt.REFERENCE, opts, plain=True)
        assert plain["pair_passes"] > 0, plain
    if variant.startswith("deep"):
        assert usage["split_passes"] >= 1, usage
    if "one-stream" in variant:
        assert usage["render_streams"] == 1, usage


def test_the_moments_buffer_is_accounted_and_allocated_on_demand():
    """rt_scene_usage: a multi-pass plain frame holds the running sums, the first multi-pass variance
    frame adds as many bytes for the moments; a one-pass variance frame adds none."""
    import torch
    w, h, spp = 64, 36, 16
    px = w * h * 12
    ds = rt.DeviceScene(scene("huge"), device=0, options=rt.options(render_streams=1, max_pass_bytes=px * 4))
    one = rt.DeviceScene(scene("huge"), device=0, options=rt.options(render_streams=1))
    try:
        rgb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        var = torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
        cam, p = rt.Camera.default(w, h), params(w, h, spp)
        ds.render(cam, p, rgb.data_ptr())
        before = ds.usage()
        ds.render_var(cam, p, rgb.data_ptr(), var.data_ptr())
        after = ds.usage()
        one.render(cam, p, rgb.data_ptr())
        one_before = one.usage()
        one.render_var(cam, p, rgb.data_ptr(), var.data_ptr())
        one_after = one.usage()
        torch.cuda.synchronize()
    finally:
        ds.close()
        one.close()
    assert after["workspace_bytes"] == before["workspace_bytes"] + px, (before, after)
    assert after["device_bytes"] == before["device_bytes"] + px
    assert one_after["workspace_bytes"] == one_before["workspace_bytes"], (one_before, one_after)


LAYOUTS = {
    "packed-rows": (64, 36, dict(row_offset=1, row_stride=3)),
    "full-frame-rows": (64, 36, dict(row_offset=1, row_stride=3, full_frame=True)),
    "untiled-37x19": (37, 19, {}),
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_rows_and_layout(layout):
    """Strided rows packed and at their global position (rows not rendered keep their sentinel), and
    a width that is no multiple of the tile (natural order)."""
    w, h, kw = LAYOUTS[layout]
    check_render("huge", w, h, 7, rt.REFERENCE, **kw)
    if layout == "full-frame-rows":
        # the host call writes the rendered rows only
        p, cam = params(w, h, 7, **kw), rt.Camera.default(w, h)
        rgb, var, _ = rt.render_var(scene("huge"), p, cam)
        ref_rgb, ref_var = reference("huge", w, h, 7, rt.REFERENCE, **kw)
        assert_same(rgb[1::3], ref_rgb[1::3], "host rgb")
        assert_same(var[1::3], ref_var[1::3], "host var")
        rest = np.ones(h, dtype=bool)
        rest[1::3] = False
        assert (rgb[rest] == 0).all() and (var[rest] == 0).all()


def test_frames_in_stream_order():
    """Three variance frames with different seeds and a plain frame between them, issued back to
    back on one stream without host synchronisation."""
    import torch
    w, h, spp = 64, 36, 7
    seeds = (SEED, SEED + 1, SEED + 2)
    cam = rt.Camera.default(w, h)
    plain_ref = reference("huge", w, h, spp, rt.REFERENCE, SEED + 3)[0]
    rgb = [torch.full((h, w, 3), SENTINEL, dtype=torch.float32, device="cuda:0") for _ in range(4)]
    var = [torch.full((h, w), SENTINEL, dtype=torch.float32, device="cuda:0") for _ in range(3)]
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    ds = rt.DeviceScene(scene("huge"), device=0)
    try:
        with torch.cuda.stream(st):
            for i, seed in enumerate(seeds):
                ds.render_var(cam, params(w, h, spp, seed), rgb[i].data_ptr(), var[i].data_ptr(), st.cuda_stream)
                if i == 1:
                    ds.render(cam, params(w, h, spp, SEED + 3), rgb[3].data_ptr(), st.cuda_stream)
        st.synchronize()
    finally:
        ds.close()
    for i, seed in enumerate(seeds):
        ref_rgb, ref_var = reference("huge", w, h, spp, rt.REFERENCE, seed)
        assert_same(rgb[i].cpu().numpy(), ref_rgb, f"frame {i} rgb")
        assert_same(var[i].cpu().numpy(), ref_var, f"frame {i} var")
    assert_same(rgb[3].cpu().numpy(), plain_ref, "the plain frame between them")


# ---- the denoiser ------------------------------------------------------------------------------------------
VAR_SCALE = 0.02  # synthetic variances lie in [0, VAR_SCALE)


@functools.lru_cache(maxsize=None)
def synthetic(w, h, block=False):
    """support.synthetic_planes with a variance in [0, VAR_SCALE), once per module."""
    return synthetic_planes(w, h, block, VAR_SCALE)


_DREFS = {}


def dreference(name, planes, use, kw):
    """denoise_var_ref over planes[use], once per (name, use, kw)."""
    key = (name, use, tuple(sorted(kw.items())))
    if key not in _DREFS:
        _DREFS[key] = denoise_var_ref.denoise(planes["beauty"], planes["variance"], **{n: planes[n] for n in use}, **kw)
    return _DREFS[key]


def dcheck(name, planes, use=GUIDES, **kw):
    """The host call with and without variance_out against the reference; returns the census."""
    ref, ref_v, census = dreference(name, planes, use, kw)
    guides = {n: planes[n] for n in use}
    got, got_v = rt.denoise_var(planes["beauty"], planes["variance"], variance_out=True, **guides, **kw)
    assert_same(got, ref, "out")
    assert_same(got_v, ref_v, "variance_out")
    assert_same(rt.denoise_var(planes["beauty"], planes["variance"], **guides, **kw), ref, "out alone")
    return census


ALL = dict(sigma_color=8.0, sigma_normal=2.0, sigma_depth=2.0, sigma_albedo=1.0, var_floor=1e-4)


@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3)])
def test_tiny_images(w, h, levels):
    dcheck(f"tiny{w}x{h}", synthetic(w, h), levels=levels, **ALL)


# 37 x 19: the synthetic variance's scale (VAR_SCALE) and these sigmas were chosen on the CPU
# reference's census (the assertion below) so that no class of tap weight is rare
CENSUS = dict(sigma_color=12.0,sigma_normal=1.5, sigma_depth=1.5, sigma_albedo=1.0, var_floor=1e-4)


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
def test_no_multiple_of_the_block(levels):
    """37 x 19, levels 1..5: a partial block of lanes in x and y, and at levels = 5 taps 32 pixels
    away in an image 19 high."""
    census = dcheck("odd", synthetic(37, 19, True), levels=levels, **CENSUS)
    if levels == 5:
        zero, between, one = census
        total = zero + between + one
        print("tap census: zero %d, between %d, one %d of %d" % (zero, between, one, total))
        # the case cannot pass with every weight zero or every weight one
        assert min(zero, between, one) * 10 >= total


TERMS = {
    "colour": (GUIDES, dict(sigma_color=8.0, sigma_normal=1e6, sigma_depth=1e6, sigma_albedo=0.0, var_floor=1e-4)),
    "colour-no-guides": ((), dict(sigma_color=8.0, var_floor=1e-3)),
    "normal": (("normal",), dict(sigma_color=0.0, sigma_normal=1.0)),
    "depth": (("depth",), dict(sigma_color=0.0, sigma_depth=2.0)),
    "albedo": (("albedo",), dict(sigma_color=0.0, sigma_albedo=1.0)),
    "none": ((), dict(sigma_color=0.0)),
    "all": (GUIDES, ALL),
}


@pytest.mark.parametrize("terms", sorted(TERMS))
def test_each_term_alone_and_all_together(terms):
    """70 x 41 at 3 levels: two blocks of 64 lanes in x, eleven of 4 rows in y."""
    use, kw = TERMS[terms]
    census = dcheck("terms", synthetic(70, 41), use=use, levels=3, **kw)
    if terms == "none":
        assert census[0] == 0 and census[1] == 0
    else:
        assert census[0] > 0 and census[1] > 0


REAL = {"64x36": (64, 36, rt.REFERENCE, 4), "128x72": (128, 72, rt.CORRECTED, 8)}


@functools.lru_cache(maxsize=None)
def real(name):
    """Beauty and variance from rt.render_var, guides from rt.render_aov with 4 samples (the huge scene)."""
    w, h, mode, spp = REAL[name]
    return frame_planes(scene("huge"), params(w, h, spp), rt.Camera.default(w, h, mode), 4, GUIDES)


@pytest.mark.parametrize("name", sorted(REAL))
def test_rendered_inputs_default_parameters(name):
    planes = real(name)
    p, v = rt.denoise_var_params(*REAL[name][:2])
    kw = denoise_var_ref.params_kwargs(p, v)
    ref, ref_v, census = dreference(name, planes, GUIDES, kw)
    print("tap census (zero, between, one):", census)
    assert np.isfinite(ref).all() and np.isfinite(ref_v).all() and min(census) > 0
    got, got_v = rt.denoise_var(planes["beauty"], planes["variance"], planes["albedo"], planes["normal"],
                                planes["depth"], variance_out=True)
    assert_same(got, ref, "out")
    assert_same(got_v, ref_v, "variance_out")


def test_render_denoise_render_on_one_stream():
    """render_var, render_aov, denoise_var_device, then the next frame into the same buffers, on one
    stream with no host synchronisation: the denoised frame and its variance are the host path's over
    the first frame's arrays, and the denoise call leaves its inputs as they were."""
    import torch
    w, h, mode, spp = REAL["64x36"]
    host = real("64x36")
    p, p2 = params(w, h, spp), params(w, h, spp, SEED + 1)
    cam = rt.Camera.default(w, h, mode)
    expect, expect_v = rt.denoise_var(host["beauty"], host["variance"], host["albedo"], host["normal"], host["depth"],
                                      variance_out=True, levels=5)
    second, second_v, _ = rt.render_var(scene("huge"), p2, cam)
    dp, dv = rt.denoise_var_params(w, h, levels=5)
    nan = float("nan")
    t = {n: torch.full((h, w, 3) if ch == 3 else (h, w), nan, dtype=torch.float32, device="cuda:0")
         for n, ch in abi.DENOISE_PLANES.items()}
    t.update({n: torch.full((h, w, ch) if ch > 1 else (h, w), nan, dtype=torch.float32, device="cuda:0")
              for n, ch in abi.DENOISE_VAR_PLANES.items()})
    inputs = ("beauty", "variance") + GUIDES
    before = {n: torch.empty_like(t[n]) for n in inputs}
    after = {n: torch.empty_like(t[n]) for n in inputs}
    vrec = rt.render.denoise_var_buffers({n: t[n].data_ptr() for n in abi.DENOISE_VAR_PLANES}, dv.var_floor)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    ds = rt.DeviceScene(scene("huge"), device=0)
    try:
        with torch.cuda.stream(st):
            ds.render_var(cam, p, t["beauty"].data_ptr(), t["variance"].data_ptr(), st.cuda_stream)
            ds.render_aov(cam, p, {n: t[n].data_ptr() for n in GUIDES}, 4, st.cuda_stream)
            for n in before:
                before[n].copy_(t[n], non_blocking=True)
            rt.denoise_var_device({n: t[n].data_ptr() for n in abi.DENOISE_PLANES}, dp, vrec, st.cuda_stream)
            for n in after:
                after[n].copy_(t[n], non_blocking=True)
            out, out_v = t["out"].clone(), t["variance_out"].clone()
            ds.render_var(cam, p2, t["beauty"].data_ptr(), t["variance"].data_ptr(), st.cuda_stream)
        st.synchronize()
    finally:
        ds.close()
    assert_same(out.cpu().numpy(), expect, "out")
    assert_same(out_v.cpu().numpy(), expect_v, "variance_out")
    for n in inputs:
        assert_same(before[n].cpu().numpy(), host[n], n + " before")
        assert_same(after[n].cpu().numpy(), host[n], n + " after")
    assert_same(t["beauty"].cpu().numpy(), second, "next frame rgb")
    assert_same(t["variance"].cpu().numpy(), second_v, "next frame var")


def test_aliased_outputs_are_refused_and_inputs_left_intact():
    import torch
    planes = synthetic(37, 19, True)
    t = {n: torch.from_numpy(np.array(a)).to("cuda:0") for n, a in planes.items()}
    t["out"], t["scratch"] = torch.zeros_like(t["beauty"]), torch.zeros_like(t["beauty"])
    t["variance_out"] = torch.zeros_like(t["variance"])
    t["var_scratch"] = torch.zeros((19, 37, 2), dtype=torch.float32, device="cuda:0")
    keep = {n: a.clone() for n, a in t.items()}
    dp, dv = rt.denoise_var_params(37, 19, levels=2)
    ptr = {n: a.data_ptr() for n, a in t.items()}
    for field, other in (("variance_out", "variance"), ("variance_out", "depth"), ("var_scratch", "variance"),
                         ("var_scratch", "out"), ("var_scratch", "variance_out"), ("out", "beauty")):
        q = dict(ptr)
        q[field] = ptr[other]
        vrec = rt.render.denoise_var_buffers({n: q[n] for n in abi.DENOISE_VAR_PLANES}, dv.var_floor)
        with pytest.raises(rt.RtError) as e:
            rt.denoise_var_device({n: q[n] for n in abi.DENOISE_PLANES}, dp, vrec)
        assert e.value.status == abi.RT_ERR_INVALID and field in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for n in t:
        assert torch.equal(t[n], keep[n]), n
    v = np.array(planes["variance"])
    b = np.array(planes["beauty"])
    o = np.zeros_like(b)
    rec = rt.render.denoise_buffers({"beauty": b.ctypes.data, "out": o.ctypes.data})
    vrec = rt.render.denoise_var_buffers({"variance": v.ctypes.data, "variance_out": v.ctypes.data}, dv.var_floor)
    assert rt.lib().rt_denoise_var(C.byref(dp), C.byref(rec), C.byref(vrec), None) == abi.RT_ERR_INVALID
