"""The preview session on the GPU (rt_preview_*).

Every comparison is on uint32 (or uint8) views with zero mismatches allowed. The huge scene, the
corrected camera on an orbit around its look-at point, 4 spp, max_depth 8, three frames with seeds
1..3, at 64 x 36 and at 70 x 37 (a partial wave per row, a last row short of the 4-row group). The
restatement (tests/tools/preview_ref.py) starts from each frame's planes as the public rt_render_var
and rt_render_aov calls give them on the same GPU (their own modules prove those); it runs once per
mode and is shared. The session's planes are read back with hipMemcpy from the addresses
rt_preview_planes reports.
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
import preview_ref  # noqa: E402
import temporal_ref  # noqa: E402
import device_io  # noqa: E402
from device_io import SENTINEL, Outputs, read_planes  # noqa: E402
from support import assert_bits as assert_same, frame_planes, orbit_camera as camera, words as u32  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SCENE_SEED, SPP, MAX_DEPTH, FRAMES = 1234, 4, 8, 3
SIZES = [(64, 36), (70, 37)]
DEMOD, FEEDBACK, NO_TEMPORAL = abi.RT_PREVIEW_DEMODULATE, abi.RT_PREVIEW_FEEDBACK, abi.RT_PREVIEW_NO_TEMPORAL
MODES = {"plain": 0, "demodulate": DEMOD, "feedback": FEEDBACK, "both": DEMOD | FEEDBACK, "no-temporal": NO_TEMPORAL,
         "no-temporal-demodulate": NO_TEMPORAL | DEMOD}


@functools.lru_cache(maxsize=None)
def scene():
    return rt.huge_scene_arrays(SCENE_SEED)


@functools.lru_cache(maxsize=None)
def device_scene():
    return rt.DeviceScene(scene(), device=0)


@functools.lru_cache(maxsize=None)
def frame(w, h, i):
    """Frame i's planes (seed 1 + i) from the public synchronous calls."""
    return frame_planes(scene(), rt.make_params(w, h, SPP, MAX_DEPTH, 1 + i), camera(w, h, i))


def params(w, h, flags, levels=2):
    return rt.preview_params(w, h, SPP, flags=flags, max_depth=MAX_DEPTH, denoise=dict(levels=levels))


@functools.lru_cache(maxsize=None)
def reference(w, h, flags, levels):
    """The restatement's three frames of a mode, once."""
    s = preview_ref.Session(params(w, h, flags, levels))
    return tuple(s.frame(frame(w, h, i), camera(w, h, i)) for i in range(FRAMES))


def session_frames(w, h, flags, levels, order=range(FRAMES), f32=True, u8=True):
    """A fresh session's frames for the cameras / seeds of `order`: [(rgb, rgb8, planes)]."""
    pv = device_scene().preview(params(w, h, flags, levels))
    out = Outputs(w, h, f32, u8)
    got = []
    for i in order:
        rgb, rgb8 = out.frame(pv, camera(w, h, i), 1 + i)
        got.append((rgb, rgb8, read_planes(pv, w, h)))
    pv.close()
    return got


def expected_usage(w, h, flags, levels):
    """The planes the contract needs, floats per pixel, each rounded up to 256 bytes."""
    temporal, feedback, demod = not flags & NO_TEMPORAL, bool(flags & FEEDBACK), bool(flags & DEMOD)
    planes = [3, 1, 3, 1] + [3, 1] * demod + [3, 1, 1] * (2 if temporal else 1) + [3, 1, 1] * (2 * temporal)
    planes += [3, 1] * feedback + [3] + [3, 2] * (levels > (2 if feedback else 1))
    return sum((4 * w * h * c + 255) // 256 * 256 for c in planes)


# ---- 1: with the flags 0 a frame is the five stage calls made by hand --------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_chain_equality(w, h):
    import torch
    got = session_frames(w, h, 0, 2)
    ds, p = device_scene(), params(w, h, 0, 2)
    plane = functools.partial(device_io.plane, w, h)
    beauty, variance, albedo, alpha = plane(3), plane(1), plane(3), plane(1)
    g = [dict(normal=plane(3), depth=plane(1), sphere_id=plane(1, torch.int32)) for _ in range(2)]
    hist = [dict(color=plane(3), variance=plane(1), history=plane(1)) for _ in range(2)]
    out, scratch, var_scratch = plane(3), plane(3), plane(2)
    rgb8 = torch.full((h, w, 3), 77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for i in range(FRAMES):
        c, o = i % 2, 1 - i % 2
        cam, rp = camera(w, h, i), rt.make_params(w, h, SPP, MAX_DEPTH, 1 + i)
        ds.render_var(cam, rp, beauty.data_ptr(), variance.data_ptr(), st.cuda_stream)
        ds.render_aov(cam, rp, dict(albedo=albedo.data_ptr(), alpha=alpha.data_ptr(), **{n: a.data_ptr() for n, a in g[c].items()}),
                      0, st.cuda_stream)
        ptrs = dict(beauty=beauty, variance=variance, alpha=alpha, **g[c], out_color=hist[c]["color"],
                    out_variance=hist[c]["variance"], out_history=hist[c]["history"])
        if i:
            ptrs.update({"prev_" + n: a for n, a in {**hist[o], **g[o]}.items()})
        rt.temporal_device({n: a.data_ptr() for n, a in ptrs.items()}, p.temporal, cam, camera(w, h, i - 1) if i else None,
                           st.cuda_stream)
        rt.denoise_var_device(dict(beauty=hist[c]["color"].data_ptr(), albedo=albedo.data_ptr(), normal=g[c]["normal"].data_ptr(),
                                   depth=g[c]["depth"].data_ptr(), out=out.data_ptr(), scratch=scratch.data_ptr()), p.denoise,
                              render.denoise_var_buffers(dict(variance=hist[c]["variance"].data_ptr(),
                                                          var_scratch=var_scratch.data_ptr()), p.var_floor), st.cuda_stream)
        rt.epilogue_rgb8_device(out.data_ptr(), rgb8.data_ptr(), w * h, st.cuda_stream)
        st.synchronize()
        rgb, tex, pl = got[i]
        assert_same(rgb, out.cpu().numpy(), f"frame {i} rgb")
        assert np.array_equal(tex, rgb8.cpu().numpy()), f"frame {i} rgb8"
        for n in ("color", "variance", "history"):
            assert_same(pl["out_" + n], hist[c][n].cpu().numpy(), f"frame {i} out_{n}")
            assert_same(pl["prev_" + n], hist[c][n].cpu().numpy(), f"frame {i} prev_{n}")
        for n, a in dict(albedo=albedo, alpha=alpha, **g[c]).items():
            assert_same(pl[n], a.cpu().numpy().view(abi.PREVIEW_PLANES[n][1]), f"frame {i} {n}")
            if "prev_" + n in pl:
                assert_same(pl["prev_" + n], pl[n], f"frame {i} prev_{n}")
        # ... and those planes are what the public synchronous calls give (the restatement's inputs)
        for n in ("albedo", "normal", "depth", "alpha", "sphere_id"):
            assert_same(pl[n], frame(w, h, i)[n], f"frame {i} {n} against rt_render_aov")
        assert_same(beauty.cpu().numpy(), frame(w, h, i)["beauty"], f"frame {i} beauty against rt_render_var")


# ---- 2: every mode against the restatement -------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("w,h", SIZES)
def test_modes_against_the_restatement(w, h, mode, levels):
    flags = MODES[mode]
    ref = reference(w, h, flags, levels)
    got = session_frames(w, h, flags, levels)
    for i, ((rgb, rgb8, pl), r) in enumerate(zip(got, ref)):
        assert pl is not None and (rgb != SENTINEL).all()
        assert_same(rgb, r["out"], f"frame {i} out")
        assert_same(pl["out_color"], r["color"], f"frame {i} accumulated colour")
        assert_same(pl["out_variance"], r["variance"], f"frame {i} accumulated variance")
        if flags & NO_TEMPORAL:
            assert pl["out_history"] is None and r["history"] is None and pl["prev_color"] is None
        else:
            assert_same(pl["out_history"], r["history"], f"frame {i} history")
    if not flags & NO_TEMPORAL:
        # the planes the next frame would reproject are the restatement's (under FEEDBACK: C_1, V_1)
        pl, want = got[-1][2], final_state(w, h, flags, levels).prev
        for n in ("color", "variance", "history"):
            assert_same(pl["prev_" + n], want[n], f"prev_{n} after the last frame")
    # the rgb8 texels are the epilogue's of the f32 output (checked on the device in test_floor and
    # test_chain_equality); here: both outputs were written
    assert (got[-1][1] != 77).any()


@functools.lru_cache(maxsize=None)
def final_state(w, h, flags, levels):
    """The restatement's session after the three frames (s.prev: what a fourth would reproject)."""
    s = preview_ref.Session(params(w, h, flags, levels))
    for i in range(FRAMES):
        s.frame(frame(w, h, i), camera(w, h, i))
    return s


@pytest.mark.parametrize("mode", sorted(MODES))
def test_usage_is_the_planes_the_mode_needs(mode):
    for levels in (1, 2, 3):
        pv = device_scene().preview(params(70, 37, MODES[mode], levels))
        assert pv.usage() == expected_usage(70, 37, MODES[mode], levels), (mode, levels)
        assert pv.planes()["frames"] == 0 and pv.planes()["out_color"] is None
        pv.close()


def test_three_levels_with_feedback_use_the_scratch_planes():
    """levels = 3: level 1 writes the scratch planes (with the flag: after level 0 wrote the history)."""
    w, h = 70, 37
    for flags in (FEEDBACK | DEMOD, 0):
        ref = reference(w, h, flags, 3)
        for i, ((rgb, _, pl), r) in enumerate(zip(session_frames(w, h, flags, 3), ref)):
            assert_same(rgb, r["out"], f"flags {flags} frame {i} out")
            assert_same(pl["out_history"], r["history"], f"flags {flags} frame {i} history")


# ---- 3: reset and ordering ------------------------------------------------------------------------------
def test_reset_and_camera_order():
    w, h, flags = 70, 37, DEMOD | FEEDBACK
    pv = device_scene().preview(params(w, h, flags, 2))
    out = Outputs(w, h)
    a0 = out.frame(pv, camera(w, h, 0), 1)[0]          # A
    ab = out.frame(pv, camera(w, h, 1), 2)[0]          # A, B
    hist_ab = read_planes(pv, w, h)["out_history"]
    assert pv.planes()["frames"] == 2
    pv.reset()
    assert pv.planes()["frames"] == 0
    b = out.frame(pv, camera(w, h, 1), 2)[0]           # B after a reset
    hist_b = read_planes(pv, w, h)["out_history"]
    first = session_frames(w, h, flags, 2, order=[1])[0]
    assert_same(b, first[0], "a frame after reset against a first frame")
    assert (hist_b == 1).all()
    assert_same(a0, reference(w, h, flags, 2)[0]["out"], "A")
    assert_same(ab, reference(w, h, flags, 2)[1]["out"], "A, B")
    had = hist_ab > 1
    differ = (u32(ab) != u32(b)).any(axis=2)
    print("pixels with history in A, B:", int(had.sum()), "of those that differ from B alone:", int((differ & had).sum()),
          "others that differ:", int((differ & ~had).sum()))
    assert had.sum() > w * h // 4 and (differ & had).sum() > had.sum() // 2
    pv.close()


def test_one_output_gives_the_bits_of_both():
    w, h, flags = 70, 37, DEMOD
    both = session_frames(w, h, flags, 2)
    only_f32 = session_frames(w, h, flags, 2, f32=True, u8=False)
    only_u8 = session_frames(w, h, flags, 2, f32=False, u8=True)
    for i in range(FRAMES):
        assert_same(only_f32[i][0], both[i][0], f"frame {i} f32 alone")
        assert only_f32[i][1] is None and only_u8[i][0] is None
        assert np.array_equal(only_u8[i][1], both[i][1]), f"frame {i} rgb8 alone"
        assert_same(only_u8[i][2]["out_history"], both[i][2]["out_history"], f"frame {i} history, rgb8 alone")


def test_two_sessions_on_one_scene_do_not_disturb_each_other():
    w, h = 64, 36
    fa, fb = DEMOD | FEEDBACK, 0
    a, b = device_scene().preview(params(w, h, fa, 2)), device_scene().preview(params(w, h, fb, 2))
    oa, ob = Outputs(w, h), Outputs(w, h)
    for i in range(FRAMES):
        # b runs one frame behind a, with another camera and seed in between a's frames
        got_a = oa.frame(a, camera(w, h, i), 1 + i)[0]
        assert_same(got_a, reference(w, h, fa, 2)[i]["out"], f"session a frame {i}")
        if i:
            got_b = ob.frame(b, camera(w, h, i - 1), i)[0]
            assert_same(got_b, reference(w, h, fb, 2)[i - 1]["out"], f"session b frame {i - 1}")
    a.close()
    b.close()


def test_frame_call_refusals_leave_the_session_usable():
    w, h = 64, 36
    pv = device_scene().preview(params(w, h, 0, 2))
    out = Outputs(w, h)
    with pytest.raises(rt.RtError) as e:
        pv.frame(camera(w, h, 0), 1, None, None)
    assert e.value.status == abi.RT_ERR_INVALID and "d_rgb" in str(e.value)
    with pytest.raises(rt.RtError) as e:
        pv.frame(None, 1, out.rgb.data_ptr(), None)
    assert e.value.status == abi.RT_ERR_INVALID and "camera" in str(e.value)
    assert pv.planes()["frames"] == 0
    assert_same(out.frame(pv, camera(w, h, 0), 1)[0], reference(w, h, 0, 2)[0]["out"], "the frame after the refusals")
    pv.close()


# ---- 4: the cases are not vacuous -------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_the_orbit_keeps_and_loses_history(w, h):
    for mode in ("plain", "both"):
        ref = reference(w, h, MODES[mode], 2)
        for i in (1, 2):
            hist, reason = ref[i]["history"], ref[i]["reason"]
            kept, none = float((hist > 1).mean()), float((reason != temporal_ref.KEPT).mean())
            print(f"{w}x{h} {mode} frame {i + 1}: history > 1 on {kept:.1%}, no history on {none:.1%}")
            assert kept >= 0.25 and none >= 0.01
            assert ((hist > 1) == (reason == temporal_ref.KEPT)).all()


# ---- 5: the floor, through the two kernels' own entry points ----------------------------------------------
def test_floor():
    import torch
    w, h = 70, 37
    g = np.random.default_rng(5)
    albedo = g.uniform(0.05, 1.0, (h, w, 3)).astype(F)
    albedo[..., 1][g.random((h, w)) < 0.3] = F(0.001)      # below the floor in one channel
    albedo[0, 0] = (0.0, 0.0078125, 0.5)
    beauty = albedo.copy()                                  # sky pixels: the albedo is the beauty's own bits
    variance = (g.random((h, w), dtype=F) * F(0.02)).astype(F)
    want_i, want_v = preview_ref.split(beauty, variance, albedo)
    low = albedo < preview_ref.FLOOR
    assert low.any() and (want_i[~low] == 1).all() and (want_i[low] == albedo[low] * F(128)).all()
    d = {n: torch.from_numpy(a).to("cuda:0") for n, a in dict(beauty=beauty, variance=variance, albedo=albedo).items()}
    illum = torch.full((h, w, 3), SENTINEL, dtype=torch.float32, device="cuda:0")
    ivar = torch.full((h, w), SENTINEL, dtype=torch.float32, device="cuda:0")
    back = torch.full((h, w, 3), SENTINEL, dtype=torch.float32, device="cuda:0")
    tex, tex_ref, tex_copy = (torch.full((h, w, 3), 77, dtype=torch.uint8, device="cuda:0") for _ in range(3))
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    rt.preview_split_device(w, h, d["beauty"].data_ptr(), d["variance"].data_ptr(), d["albedo"].data_ptr(), illum.data_ptr(),
                            ivar.data_ptr(), st.cuda_stream)
    rt.preview_merge_device(w, h, illum.data_ptr(), d["albedo"].data_ptr(), back.data_ptr(), tex.data_ptr(), st.cuda_stream)
    rt.epilogue_rgb8_device(back.data_ptr(), tex_ref.data_ptr(), w * h, st.cuda_stream)
    rt.preview_merge_device(w, h, illum.data_ptr(), None, None, tex_copy.data_ptr(), st.cuda_stream)
    st.synchronize()
    assert_same(illum.cpu().numpy(), want_i, "illumination")
    assert_same(ivar.cpu().numpy(), want_v, "its variance")
    assert_same(back.cpu().numpy(), preview_ref.merge(want_i, albedo), "merged")
    assert_same(back.cpu().numpy(), beauty, "merged against the beauty (1 * a and (a * 128) / 128 are exact)")
    assert torch.equal(tex, tex_ref)
    # without an albedo the texels are those of the filter's own bits: 255 where I = 1
    copy = tex_copy.cpu().numpy()
    assert (copy[~low] == 255).all() and (copy[low] < 255).all()
