"""The à-trous denoiser on the GPU (rt_denoise / rt_denoise_device) against its
CPU restatement (tests/tools/denoise_ref.py).

Every comparison is on uint32 views with zero mismatches allowed, and every case runs twice: with
the library's choice of kernel per level (tiled for the small steps) and with RT_DENOISE_DIRECT.
The references are computed once per module and shared.
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
import denoise_ref  # noqa: E402
from support import assert_bits as assert_same, synthetic_planes  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SEED = 1234
KERNELS = pytest.mark.parametrize("direct", [False, True], ids=["tiled", "direct"])
GUIDES = ("albedo", "normal", "depth")


synthetic = functools.lru_cache(maxsize=None)(synthetic_planes)  # (w, h, block=False), once per module


_REFS = {}


def reference(name, planes, use, kw):
    """denoise_ref over planes[use], once per (name, use, kw)."""
    key = (name, use, tuple(sorted(kw.items())))
    if key not in _REFS:
        _REFS[key] = denoise_ref.denoise(planes["beauty"], **{n: planes[n] for n in use}, **kw)
    return _REFS[key]


def run_gpu(planes, use, direct, kw):
    # a sigma the case does not set is the library's default: its plane is absent
    return rt.denoise(planes["beauty"], **{n: planes[n] for n in use}, direct=direct, **kw)


def check(name, planes, direct, use=GUIDES, **kw):
    ref, census = reference(name, planes, use, kw)
    assert_same(run_gpu(planes, use, direct, kw), ref)
    return census


ALL = dict(sigma_color=1.0, sigma_normal=2.0, sigma_depth=2.0, sigma_albedo=1.0)


# ---- synthetic shapes ----------------------------------------------------------------------------------
@KERNELS
@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3)])
def test_tiny_images(w, h, levels, direct):
    check(f"tiny{w}x{h}", synthetic(w, h), direct, levels=levels, **ALL)
    check(f"tiny{w}x{h}", synthetic(w, h), direct, levels=levels, demodulate=True, **ALL)


# 37 x 19: sigmas chosen on the reference's census (the assertion below) so that no class is rare
CENSUS = dict(sigma_color=1.0, sigma_normal=1.5, sigma_depth=1.5, sigma_albedo=1.0)


@KERNELS
@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
def test_no_multiple_of_any_tile(levels, direct):
    """37 x 19, levels 1..5: a partial tile in x and y, and at levels = 5 a halo (32) larger than
    the image's height."""
    census = check("odd", synthetic(37, 19, True), direct, levels=levels, **CENSUS)
    if levels == 5:
        zero, between, one = census
        total = zero + between + one
        print("tap census: zero %d, between %d, one %d of %d" % (zero, between, one, total))
        # the case cannot pass with every weight zero or every weight one
        assert min(zero, between, one) * 10 >= total


@KERNELS
def test_tile_seams(direct):
    """70 x 41: two full 32 x 16 tiles and a partial one each way; steps 1 and 2 are tiled, so
    every seam is crossed by taps of both, and step 4 follows them with the direct kernel."""
    check("seams", synthetic(70, 41), direct, levels=3, **ALL)
    check("seams", synthetic(70, 41), direct, levels=3, demodulate=True, **ALL)


TERMS = {
    "colour": (GUIDES, dict(sigma_color=0.5, sigma_normal=1e6, sigma_depth=1e6, sigma_albedo=0.0)),
    "colour-no-guides": ((), dict(sigma_color=0.5)),
    "normal": (("normal",), dict(sigma_color=0.0, sigma_normal=1.0)),
    "depth": (("depth",), dict(sigma_color=0.0, sigma_depth=2.0)),
    "albedo": (("albedo",), dict(sigma_color=0.0, sigma_albedo=1.0)),
    "none": ((), dict(sigma_color=0.0)),
    "all": (GUIDES, ALL),
    "demodulate-albedo-off": (("albedo",), dict(sigma_color=1.0, sigma_albedo=0.0, demodulate=True)),
    "demodulate-all": (GUIDES, dict(demodulate=True, **ALL)),
}


@KERNELS
@pytest.mark.parametrize("terms", sorted(TERMS))
def test_each_term_alone_and_all_together(terms, direct):
    use, kw = TERMS[terms]
    census = check("terms", synthetic(70, 41), direct, use=use, levels=3, **kw)
    if terms == "none":
        assert census[0] == 0 and census[1] == 0
    elif terms not in ("colour",):
        assert census[0] > 0 and census[1] > 0


# ---- real inputs ----------------------------------------------------------------------------------------
REAL = {"64x36": (64, 36, rt.REFERENCE, 4), "128x72": (128, 72, rt.CORRECTED, 8)}


@functools.lru_cache(maxsize=None)
def real(name):
    """Beauty from rt.render_f32, guides from rt.render_aov with 4 samples (the huge scene)."""
    w, h, mode, spp = REAL[name]
    scene = rt.huge_scene_arrays(SEED)
    p, cam = rt.make_params(w, h, spp, 64, SEED), rt.Camera.default(w, h, mode)
    beauty, _ = rt.render_f32(scene, p, cam)
    g = rt.render_aov(scene, p, cam, 4, GUIDES)
    return dict(beauty=beauty, **g)


@KERNELS
@pytest.mark.parametrize("demodulate", [False, True], ids=["plain", "demodulated"])
@pytest.mark.parametrize("name", sorted(REAL))
def test_rendered_inputs_default_parameters(name, demodulate, direct):
    planes = real(name)
    d = rt.denoise_params(*REAL[name][:2])
    kw = dict(levels=5, sigma_color=d.sigma_color, sigma_normal=d.sigma_normal, sigma_depth=d.sigma_depth,
              sigma_albedo=d.sigma_albedo, demodulate=demodulate)
    ref, census = reference(name, planes, GUIDES, kw)
    print("tap census (zero, between, one):", census)
    assert np.isfinite(ref).all() and min(census) > 0
    got = rt.denoise(planes["beauty"], planes["albedo"], planes["normal"], planes["depth"], levels=5,
                     demodulate=demodulate, direct=direct)
    assert_same(got, ref)


def test_inputs_need_not_be_contiguous():
    planes = synthetic(70, 41)
    wide = np.zeros((41, 70, 4), dtype=np.float32)
    wide[..., :3] = planes["beauty"]
    ref, _ = reference("seams", planes, GUIDES, dict(levels=3, **ALL))
    got = rt.denoise(wide[..., :3], planes["albedo"], planes["normal"], np.asfortranarray(planes["depth"]),
                     levels=3, **ALL)
    assert_same(got, ref)


def test_stats_of_the_host_call():
    planes = synthetic(37, 19, True)
    st = abi.RtStats()
    rt.denoise(planes["beauty"], depth=planes["depth"], levels=2, stats=st)
    assert st.kernel_ms > 0 and st.wall_ms >= st.kernel_ms
    assert (st.primaries, st.segments, st.sphere_tests, st.box_tests) == (0, 0, 0, 0)


# ---- the device call ---------------------------------------------------------------------------------------
def _dev(torch, a):
    return torch.from_numpy(np.array(a)).to("cuda:0")  # a writable copy: the shared planes are read-only


@KERNELS
def test_device_call_in_stream_order(direct):
    """Beauty frame, feature buffers, denoise, then another beauty frame into the same buffer, on
    one stream with no host synchronisation between them: the denoised frame is rt.denoise of the
    first frame's host arrays, and the denoise call leaves beauty and the guides as they were."""
    import torch
    w, h, mode, spp = REAL["64x36"]
    scene = rt.huge_scene_arrays(SEED)
    p, p2 = rt.make_params(w, h, spp, 64, SEED), rt.make_params(w, h, spp, 64, SEED + 1)
    cam = rt.Camera.default(w, h, mode)
    host = real("64x36")
    expect = rt.denoise(host["beauty"], host["albedo"], host["normal"], host["depth"], levels=5, demodulate=True,
                        direct=direct)
    second, _ = rt.render_f32(scene, p2, cam)
    dp = rt.denoise_params(w, h, levels=5, demodulate=True, direct=direct)
    nan = float("nan")
    t = {n: torch.full((h, w, 3) if ch == 3 else (h, w), nan, dtype=torch.float32, device="cuda:0")
         for n, ch in abi.DENOISE_PLANES.items()}
    before = {n: torch.empty_like(t[n]) for n in ("beauty",) + GUIDES}
    after = {n: torch.empty_like(t[n]) for n in ("beauty",) + GUIDES}
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    ds = rt.DeviceScene(scene, device=0)
    try:
        with torch.cuda.stream(st):
            ds.render(cam, p, t["beauty"].data_ptr(), st.cuda_stream)
            ds.render_aov(cam, p, {n: t[n].data_ptr() for n in GUIDES}, 4, st.cuda_stream)
            for n in before:
                before[n].copy_(t[n], non_blocking=True)
            rt.denoise_device({n: a.data_ptr() for n, a in t.items()}, dp, st.cuda_stream)
            for n in after:
                after[n].copy_(t[n], non_blocking=True)
            ds.render(cam, p2, t["beauty"].data_ptr(), st.cuda_stream)
        st.synchronize()
    finally:
        ds.close()
    assert_same(t["out"].cpu().numpy(), expect)
    for n in before:
        assert_same(before[n].cpu().numpy(), host[n])
        assert_same(after[n].cpu().numpy(), host[n])
    assert_same(t["beauty"].cpu().numpy(), second)


@KERNELS
def test_one_level_needs_no_scratch(direct):
    import torch
    planes = synthetic(37, 19, True)
    ref, _ = reference("odd", planes, GUIDES, dict(levels=1, **CENSUS))
    t = {n: _dev(torch, planes[n]) for n in planes}
    t["out"] = torch.zeros((19, 37, 3), dtype=torch.float32, device="cuda:0")
    dp = rt.denoise_params(37, 19, levels=1, direct=direct, **CENSUS)
    rt.denoise_device({n: a.data_ptr() for n, a in t.items()}, dp, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert_same(t["out"].cpu().numpy(), ref)


@KERNELS
def test_single_level_call_is_that_level_of_the_run(direct):
    """rt_denoise_level_device (the timing script's call): level 2 of a 3-level run over the
    2-level result is the 3-level result; without RT_DENOISE_DIRECT it is the tiled kernel at step
    4, which the library itself leaves to the direct one."""
    import torch
    planes = synthetic(70, 41)
    two, _ = reference("seams", planes, GUIDES, dict(levels=2, **ALL))
    three, _ = reference("seams", planes, GUIDES, dict(levels=3, **ALL))
    t = {n: _dev(torch, planes[n]) for n in GUIDES}
    t["beauty"] = _dev(torch, two)
    t["out"] = torch.zeros((41, 70, 3), dtype=torch.float32, device="cuda:0")
    dp = rt.denoise_params(70, 41, levels=3, direct=direct, **ALL)
    rec = rt.render.denoise_buffers({n: a.data_ptr() for n, a in t.items()})
    rt.render.check(rt.lib().rt_denoise_level_device(C.byref(dp), C.byref(rec), 2,
                                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert_same(t["out"].cpu().numpy(), three)


def test_aliased_output_is_refused():
    import torch
    planes = synthetic(37, 19, True)
    t = {n: _dev(torch, planes[n]) for n in planes}
    keep = t["beauty"].clone()
    scratch = torch.zeros_like(keep)
    dp = rt.denoise_params(37, 19, levels=2)
    ptr = {n: a.data_ptr() for n, a in t.items()}
    with pytest.raises(rt.RtError) as e:
        rt.denoise_device(dict(ptr, out=ptr["beauty"], scratch=scratch.data_ptr()), dp)
    assert e.value.status == abi.RT_ERR_INVALID and "out" in str(e.value)
    torch.cuda.synchronize()
    assert torch.equal(t["beauty"], keep)
    b = np.array(planes["beauty"])
    rec = rt.render.denoise_buffers({"beauty": b.ctypes.data, "out": b.ctypes.data})
    assert rt.lib().rt_denoise(C.byref(dp), C.byref(rec), None) == abi.RT_ERR_INVALID
