"""The preview session at rest on the GPU (rt_preview_refine_device): every refine
call against the stage calls made by hand (step -> preview_split_device -> denoise_var_device ->
preview_merge_device) and against the restatements (preview_ref / denoise_var_ref over
progressive_ref's planes); the completing call and one more against render_f32; what restarts a
refinement; the frame call after one; the refusal of upscaled sessions.

Every comparison is on uint32 (or uint8) views with zero mismatches allowed. 64 x 36, the huge scene,
a frame of 16 samples refined in calls of 4, 4 and 8; references are computed once and shared.
"""
import functools
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi
from raytracinginoneweekend_amd import render

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import denoise_var_ref  # noqa: E402
import moments_ref  # noqa: E402
import preview_ref  # noqa: E402
import progressive_ref  # noqa: E402
from motion_cases import huge_a_b  # noqa: E402
import device_io  # noqa: E402
from device_io import Outputs  # noqa: E402
from support import assert_bits as assert_same, words as u32  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, MAX_DEPTH, TOTAL = 64, 36, 4, 8, 16
CALLS = (4, 4, 8)
DEMOD, FEEDBACK = abi.RT_PREVIEW_DEMODULATE, abi.RT_PREVIEW_FEEDBACK
MODES = {"plain": 0, "demodulate": DEMOD, "both": DEMOD | FEEDBACK}


@functools.lru_cache(maxsize=None)
def records(which="a"):
    a, b = huge_a_b()
    return a if which == "a" else b


def camera(mode=rt.CORRECTED):
    return rt.Camera.default(W, H, mode)


def params(flags):
    return rt.preview_params(W, H, SPP, flags=flags, max_depth=MAX_DEPTH, denoise=dict(levels=2))


def frame_params(seed, total=TOTAL):
    return rt.make_params(W, H, total, MAX_DEPTH, seed)


@functools.lru_cache(maxsize=None)
def estimates(seed, mode=rt.CORRECTED, total=TOTAL, calls=CALLS, which="a"):
    """progressive_ref's estimates after each call, and the guides of the refinement."""
    s, m = records(which)
    rp, cam = frame_params(seed, total), camera(mode)
    _, _, samples = moments_ref.render(s, m, cam, rp)
    guides = rt.render_aov((s, m), rp, cam, min(total, SPP))
    return progressive_ref.run(samples, calls), guides


@functools.lru_cache(maxsize=None)
def expected(flags, seed, mode=rt.CORRECTED, total=TOTAL, calls=CALLS, which="a"):
    """What each refine call stores, by the restatements: [float32 (H, W, 3)]."""
    est, g = estimates(seed, mode, total, calls, which)
    p = params(flags)
    kw = dict(sigma_color=p.denoise.sigma_color, sigma_normal=p.denoise.sigma_normal, sigma_depth=p.denoise.sigma_depth,
              sigma_albedo=p.denoise.sigma_albedo, var_floor=p.var_floor)
    out, done = [], 0
    for n, e in zip(calls, est):
        done += n
        if done >= total:
            out.append(e["rgb"])
            continue
        color, variance = e["rgb"], e["var"]
        if flags & DEMOD:
            color, variance = preview_ref.split(color, variance, g["albedo"])
        filtered = denoise_var_ref.denoise(color, variance, g["albedo"], g["normal"], g["depth"], levels=p.denoise.levels, **kw)[0]
        out.append(preview_ref.merge(filtered, g["albedo"] if flags & DEMOD else None))
    return out


@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_call_is_the_stages_by_hand_and_the_restatement(mode):
    import torch
    flags, seed, cam = MODES[mode], 5, camera()
    want = expected(flags, seed)
    p, rp = params(flags), frame_params(seed)
    exact, _ = rt.render_f32(records(), rp, cam)
    ds = rt.DeviceScene(records(), device=0)
    plane = functools.partial(device_io.plane, W, H)
    try:
        pv = ds.preview(p)
        before = pv.usage()
        out = Outputs(W, H)
        # the chain by hand: a progressive session and planes of the caller's
        st = torch.cuda.Stream()
        pg = ds.progressive(cam, rp)
        beauty, variance, illum, ivar = plane(3), plane(1), plane(3), plane(1)
        g = dict(albedo=plane(3), normal=plane(3), depth=plane(1), alpha=plane(1), sphere_id=plane(1, torch.int32))
        filtered, scratch, var_scratch, hand = plane(3), plane(3), plane(2), plane(3)
        hand8 = torch.full((H, W, 3), 77, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ds.render_aov(cam, rp, {n: a.data_ptr() for n, a in g.items()}, min(TOTAL, SPP), st.cuda_stream)
        done = 0
        for i, n in enumerate(CALLS + (4,)):  # (one call past the end)
            rgb, rgb8 = out.refine(pv, cam, seed, TOTAL, n)
            done = min(TOTAL, done + n)
            assert pv.refine_info() == (done, TOTAL)
            if done == TOTAL:
                assert_same(rgb, exact, f"call {i}: the frame itself against render_f32")
                assert np.array_equal(rgb8, progressive_ref.texel(exact)), f"call {i}: its texels"
                continue
            pg.step(n, rgb_ptr=beauty.data_ptr(), variance_ptr=variance.data_ptr(), stream=st.cuda_stream)
            color, var = beauty, variance
            if flags & DEMOD:
                rt.preview_split_device(W, H, beauty.data_ptr(), variance.data_ptr(), g["albedo"].data_ptr(), illum.data_ptr(),
                                        ivar.data_ptr(), st.cuda_stream)
                color, var = illum, ivar
            rt.denoise_var_device(dict(beauty=color.data_ptr(), albedo=g["albedo"].data_ptr(), normal=g["normal"].data_ptr(),
                                       depth=g["depth"].data_ptr(), out=filtered.data_ptr(), scratch=scratch.data_ptr()), p.denoise,
                                  render.denoise_var_buffers(dict(variance=var.data_ptr(), var_scratch=var_scratch.data_ptr()),
                                                             p.var_floor), st.cuda_stream)
            rt.preview_merge_device(W, H, filtered.data_ptr(), g["albedo"].data_ptr() if flags & DEMOD else None, hand.data_ptr(),
                                    hand8.data_ptr(), st.cuda_stream)
            st.synchronize()
            assert_same(rgb, hand.cpu().numpy(), f"call {i} against the stages by hand")
            assert np.array_equal(rgb8, hand8.cpu().numpy()), f"call {i} rgb8 against the stages by hand"
            assert_same(rgb, want[i], f"call {i} against the restatement")
            assert int(np.count_nonzero(u32(rgb) != u32(exact))) > 1000  # (a filtered estimate, not the frame)
        assert pv.usage() == before + 24 * W * H  # the session's own progressive session is counted
        pg.close()
        pv.close()
    finally:
        ds.close()


def test_what_restarts_a_refinement():
    """Another seed, camera, total or scene epoch, and a frame call in between: the call is the first
    of a new refinement (done = its own samples, the output the new arguments' first estimate)."""
    flags = DEMOD
    ds = rt.DeviceScene(records(), device=0)
    try:
        pv = ds.preview(params(flags))
        out = Outputs(W, H)
        cam, other = camera(), camera(rt.REFERENCE)
        rgb, _ = out.refine(pv, cam, 5, TOTAL, 4)
        assert_same(rgb, expected(flags, 5)[0], "the first call")
        rgb, _ = out.refine(pv, cam, 5, TOTAL, 4)
        assert pv.refine_info() == (8, TOTAL)
        assert_same(rgb, expected(flags, 5)[1], "the second call goes on")
        rgb, _ = out.refine(pv, cam, 6, TOTAL, 4)
        assert pv.refine_info() == (4, TOTAL)
        assert_same(rgb, expected(flags, 6, calls=(4,))[0], "another seed")
        rgb, _ = out.refine(pv, other, 6, TOTAL, 4)
        assert pv.refine_info() == (4, TOTAL)
        assert_same(rgb, expected(flags, 6, rt.REFERENCE, calls=(4,))[0], "another camera")
        rgb, _ = out.refine(pv, other, 6, 8, 4)
        assert pv.refine_info() == (4, 8)
        assert_same(rgb, expected(flags, 6, rt.REFERENCE, 8, (4,))[0], "another total")
        # a frame call in between: the refinement starts again, and that frame had no history
        rgb, _ = out.refine(pv, cam, 5, TOTAL, 4)
        frame = Outputs(W, H)
        pv.frame(cam, 9, frame.rgb.data_ptr(), frame.rgb8.data_ptr(), frame.stream.cuda_stream)
        frame.stream.synchronize()
        assert pv.planes()["frames"] == 1 and pv.refine_info() == (0, 0)
        pv.frame(cam, 10, frame.rgb.data_ptr(), frame.rgb8.data_ptr(), frame.stream.cuda_stream)
        frame.stream.synchronize()
        assert pv.planes()["frames"] == 2
        rgb, _ = out.refine(pv, cam, 5, TOTAL, 4)
        assert pv.refine_info() == (4, TOTAL)
        assert_same(rgb, expected(flags, 5)[0], "after a frame call")
        pv.frame(cam, 11, frame.rgb.data_ptr(), frame.rgb8.data_ptr(), frame.stream.cuda_stream)
        frame.stream.synchronize()
        assert pv.planes()["frames"] == 1  # no history after a refinement
        # the scene's epoch
        rgb, _ = out.refine(pv, cam, 5, TOTAL, 4)
        ds.update(records("b"))
        rgb, _ = out.refine(pv, cam, 5, TOTAL, 4)
        assert pv.refine_info() == (4, TOTAL)
        assert_same(rgb, expected(flags, 5, calls=(4,), which="b")[0], "after a scene update")
        # refusals leave the refinement as it is
        for args, word in (((cam, 5, TOTAL, 3), "n_samples"), ((cam, 5, 1, 4), "total_spp"), ((None, 5, TOTAL, 4), "camera")):
            with pytest.raises(rt.RtError) as e:
                pv.refine(*args, out.rgb.data_ptr(), None, out.stream.cuda_stream)
            assert e.value.status == abi.RT_ERR_INVALID and word in str(e.value), str(e.value)
        with pytest.raises(rt.RtError) as e:
            pv.refine(cam, 5, TOTAL, 4, None, None, out.stream.cuda_stream)
        assert e.value.status == abi.RT_ERR_INVALID and "d_rgb" in str(e.value)
        assert pv.refine_info() == (4, TOTAL)
        pv.close()
    finally:
        ds.close()


def test_an_upscaled_session_does_not_refine():
    ds = rt.DeviceScene(records(), device=0)
    try:
        p = rt.preview_params(32, 18, SPP, max_depth=MAX_DEPTH)
        pv = ds.preview(p, rt.preview_upscale(p, W, H))
        out = Outputs(W, H)
        with pytest.raises(rt.RtError) as e:
            pv.refine(camera(), 5, TOTAL, 4, out.rgb.data_ptr(), None, out.stream.cuda_stream)
        assert e.value.status == abi.RT_ERR_UNSUPPORTED and "upscaled" in str(e.value)
        pv.close()
    finally:
        ds.close()
