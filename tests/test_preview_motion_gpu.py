"""The preview session on a scene whose spheres move (rt_scene_update under rt_preview_frame_device,
DESIGN.md §4.16): a session's frames against the stage calls made by hand, with
rt_temporal_motion_device where the scene's geometry epoch stepped by one; the frames without history
after two updates or an appearance update; the session's bytes; a scene that is never updated.

64 x 36, 4 spp, 2 levels, max_depth 8, a static corrected camera, the huge scene with spheres 2, 3 and
4 moving. Every comparison is on uint32 (or uint8) views with zero mismatches allowed.
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
import device_io  # noqa: E402
from device_io import SENTINEL, read_planes  # noqa: E402
from support import assert_bits as assert_same  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, MAX_DEPTH, LEVELS = 64, 36, 4, 8, 2
DEMOD = abi.RT_PREVIEW_DEMODULATE
MOVED_IDS = (2, 3, 4)
GUIDES = ("normal", "depth", "alpha", "sphere_id")


@functools.lru_cache(maxsize=None)
def records(step, painted=False):
    """The huge scene with spheres 2, 3 and 4 moved by `step` x (0, 0, 0.15); painted: sphere 0's albedo changed."""
    s, m = rt.huge_scene_arrays(1234)
    s, m = s.copy(), m.copy()
    for i in MOVED_IDS:
        s["center"][i, 2] = s["center"][i, 2] + F(0.15) * F(step)
    if painted:
        m["albedo"][s["material"][0]] = (F(0.9), F(0.1), F(0.1))
    return s, m


def camera(w=W, h=H):
    return rt.Camera.default(w, h, rt.CORRECTED)


def params(flags, w=W, h=H):
    return rt.preview_params(w, h, SPP, flags=flags, max_depth=MAX_DEPTH, denoise=dict(levels=LEVELS))


def plane(ch, dtype=None, w=W, h=H):
    return device_io.plane(w, h, ch, dtype)


def Images(w=W, h=H):
    """Sentinel-filled device images; the caller brings the stream."""
    return device_io.Outputs(w, h, own_stream=False)


class HandChain:
    """The five (with DEMODULATE seven) stage calls of a frame on planes of the test's own, with the
    session's bookkeeping restated: history iff a previous frame exists and the scene's appearance epoch
    is that frame's and its geometry epoch that frame's or one more; the motion call iff one more."""

    def __init__(self, ds, flags):
        import torch
        self.ds, self.p, self.demod = ds, params(flags), bool(flags & DEMOD)
        self.beauty, self.variance, self.albedo, self.alpha = plane(3), plane(1), plane(3), plane(1)
        self.illum, self.illum_var = plane(3), plane(1)
        self.g = [dict(normal=plane(3), depth=plane(1), sphere_id=plane(1, torch.int32)) for _ in range(2)]
        self.hist = [dict(color=plane(3), variance=plane(1), history=plane(1)) for _ in range(2)]
        self.filtered, self.scratch, self.var_scratch = plane(3), plane(3), plane(2)
        self.img = Images()
        self.frames, self.cur, self.epochs = 0, 0, None
        self.calls = []
        torch.cuda.synchronize()
        self.st = torch.cuda.Stream()

    def reset(self):
        self.frames = 0

    def frame(self, seed):
        st, p, c, o = self.st.cuda_stream, self.p, self.cur, 1 - self.cur
        cam, rp = camera(), rt.make_params(W, H, SPP, MAX_DEPTH, seed)
        mo = self.ds.motion()
        now = (mo["geometry_epoch"], mo["appearance_epoch"])
        history = self.frames > 0 and now[1] == self.epochs[1] and now[0] - self.epochs[0] <= 1
        moved = history and now[0] != self.epochs[0]
        g, hist = self.g[c], self.hist[c]
        self.ds.render_var(cam, rp, self.beauty.data_ptr(), self.variance.data_ptr(), st)
        self.ds.render_aov(cam, rp, dict(albedo=self.albedo.data_ptr(), alpha=self.alpha.data_ptr(),
                                         **{n: a.data_ptr() for n, a in g.items()}), 0, st)
        color, variance = self.beauty, self.variance
        if self.demod:
            rt.preview_split_device(W, H, self.beauty.data_ptr(), self.variance.data_ptr(), self.albedo.data_ptr(),
                                    self.illum.data_ptr(), self.illum_var.data_ptr(), st)
            color, variance = self.illum, self.illum_var
        ptrs = dict(beauty=color, variance=variance, alpha=self.alpha, **g, out_color=hist["color"],
                    out_variance=hist["variance"], out_history=hist["history"])
        if history:
            ptrs.update({"prev_" + n: a for n, a in {**self.hist[o], **self.g[o]}.items()})
        rt.temporal_device({n: a.data_ptr() for n, a in ptrs.items()}, p.temporal, cam, cam if history else None, st,
                           motion=(mo["centres"], mo["prev_centres"], mo["n_spheres"]) if moved else None)
        self.calls.append("motion" if moved else "static" if history else "none")
        rt.denoise_var_device(dict(beauty=hist["color"].data_ptr(), albedo=self.albedo.data_ptr(), normal=g["normal"].data_ptr(),
                                   depth=g["depth"].data_ptr(), out=self.filtered.data_ptr(), scratch=self.scratch.data_ptr()),
                              p.denoise, render.denoise_var_buffers(dict(variance=hist["variance"].data_ptr(),
                                                                         var_scratch=self.var_scratch.data_ptr()), p.var_floor), st)
        rt.preview_merge_device(W, H, self.filtered.data_ptr(), self.albedo.data_ptr() if self.demod else None,
                                self.img.rgb.data_ptr(), self.img.rgb8.data_ptr(), st)
        self.st.synchronize()
        self.frames = self.frames + 1 if history else 1
        self.cur, self.epochs = o, now
        planes = {"out_" + n: a.cpu().numpy() for n, a in hist.items()}
        planes.update({"prev_" + n: a.cpu().numpy() for n, a in hist.items()})
        planes.update(albedo=self.albedo.cpu().numpy(), alpha=self.alpha.cpu().numpy())
        for n, a in g.items():
            planes[n] = planes["prev_" + n] = a.cpu().numpy().view(abi.PREVIEW_PLANES[n][1])
        return (*self.img.host(), planes)


def session_frame(pv, img, seed, stream):
    pv.frame(camera(), seed, img.rgb.data_ptr(), img.rgb8.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return (*img.host(), read_planes(pv, W, H))


def assert_frame(got, want, what):
    rgb, rgb8, pl = got
    assert (rgb != SENTINEL).all()
    assert_same(rgb, want[0], f"{what} rgb")
    assert np.array_equal(rgb8, want[1]), f"{what} rgb8"
    for n, a in want[2].items():
        assert_same(pl[n], a, f"{what} plane {n}")


# the updates before frames 0..3: none, none, to B after frame 2 (index 1), a further shift after frame 3
SCHEDULE = (None, None, 1, 2)


# ---- 1: four frames with two updates -----------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, DEMOD], ids=["plain", "demodulate"])
def test_session_equals_the_stage_calls_made_by_hand(flags):
    import torch
    ds_s, ds_h = rt.DeviceScene(records(0)), rt.DeviceScene(records(0))
    pv, hand, img = ds_s.preview(params(flags)), HandChain(ds_h, flags), Images()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    changed = 0
    for i, step in enumerate(SCHEDULE):
        if step is not None:
            ds_s.update(records(step))
            ds_h.update(records(step))
        want = hand.frame(1 + i)
        got = session_frame(pv, img, 1 + i, st)
        assert_frame(got, want, f"frame {i}")
        assert pv.planes()["frames"] == i + 1
        if hand.calls[-1] == "motion":
            # ... and the motion mattered: the static stage on the same planes gives another history
            on_moved = np.isin(want[2]["sphere_id"], MOVED_IDS)
            changed += int((want[2]["out_history"][on_moved] > 1).sum())
    assert hand.calls == ["none", "static", "motion", "motion"]
    print("pixels on a moved sphere that kept their history in the motion frames:", changed)
    assert changed >= 20
    pv.close()
    ds_s.close()
    ds_h.close()


def test_upscaled_session_follows_the_scene():
    """Render 32 x 18 -> 64 x 36: the render-size planes are an ordinary session's on a scene updated the
    same way (the test above ties those to the stage calls), and the output is the guided upsample and the
    merge made by hand over them with output-size guides from the updated scene."""
    import torch
    lw, lh = 32, 18
    flags = DEMOD
    p = rt.preview_params(lw, lh, SPP, flags=flags, max_depth=MAX_DEPTH, denoise=dict(levels=LEVELS))
    u = rt.preview_upscale(p, W, H)
    ds_o, ds_u = rt.DeviceScene(records(0)), rt.DeviceScene(records(0))
    ordinary, upscaled = ds_o.preview(p), ds_u.preview(p, u)
    usage = upscaled.usage()
    lo_img, own, hand = Images(lw, lh), Images(), Images()
    filtered, scratch, var_scratch = plane(3, w=lw, h=lh), plane(3, w=lw, h=lh), plane(2, w=lw, h=lh)
    g = dict(albedo=plane(3), normal=plane(3), depth=plane(1), alpha=plane(1), sphere_id=plane(1, torch.int32))
    upsampled = plane(3)
    up_params = rt.upsample_params(W, H, lw, lh, normal_tol=u.normal_tol, depth_tol=u.depth_tol)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    cam = camera()
    for i, step in enumerate(SCHEDULE):
        if step is not None:
            ds_o.update(records(step))
            ds_u.update(records(step))
        seed = 1 + i
        ordinary.frame(cam, seed, lo_img.rgb.data_ptr(), lo_img.rgb8.data_ptr(), st.cuda_stream)
        pl = ordinary.planes()
        rt.denoise_var_device(dict(beauty=pl["out_color"], albedo=pl["albedo"], normal=pl["normal"], depth=pl["depth"],
                                   out=filtered.data_ptr(), scratch=scratch.data_ptr()), p.denoise,
                              render.denoise_var_buffers(dict(variance=pl["out_variance"], var_scratch=var_scratch.data_ptr()),
                                                         p.var_floor), st.cuda_stream)
        ds_o.render_aov(cam, rt.make_params(W, H, SPP, MAX_DEPTH, seed), {n: t.data_ptr() for n, t in g.items()}, 0,
                        st.cuda_stream)
        rt.upsample_device(dict(lo_color=filtered.data_ptr(), lo_normal=pl["normal"], lo_depth=pl["depth"],
                                lo_sphere_id=pl["sphere_id"], out_color=upsampled.data_ptr(),
                                **{n: g[n].data_ptr() for n in GUIDES}), up_params, st.cuda_stream)
        rt.preview_merge_device(W, H, upsampled.data_ptr(), g["albedo"].data_ptr(), hand.rgb.data_ptr(), hand.rgb8.data_ptr(),
                                st.cuda_stream)
        st.synchronize()
        want_planes = read_planes(ordinary, lw, lh)
        upscaled.frame(cam, seed, own.rgb.data_ptr(), own.rgb8.data_ptr(), st.cuda_stream)
        st.synchronize()
        (rgb, rgb8), (want, want8) = own.host(), hand.host()
        assert (rgb != SENTINEL).all()
        assert_same(rgb, want, f"frame {i} d_rgb")
        assert np.array_equal(rgb8, want8), f"frame {i} d_rgb8"
        got_planes = read_planes(upscaled, lw, lh)
        for n, a in want_planes.items():
            assert_same(got_planes[n], a, f"frame {i} render-size plane {n}")
    assert upscaled.usage() == usage
    for x in (ordinary, upscaled, ds_o, ds_u):
        x.close()


# ---- 2: frames without history ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["two-updates", "albedo-only"])
def test_frames_that_restart_equal_the_first_frame_after_a_reset(case):
    import torch
    ds_a, ds_b = rt.DeviceScene(records(0)), rt.DeviceScene(records(0))
    pa, pb, ia, ib = ds_a.preview(params(DEMOD)), ds_b.preview(params(DEMOD)), Images(), Images()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for seed in (1, 2):
        session_frame(pa, ia, seed, st)
        session_frame(pb, ib, seed, st)
    final = records(2) if case == "two-updates" else records(0, painted=True)
    if case == "two-updates":
        ds_a.update(records(1))
    ds_a.update(final)
    ds_b.update(final)
    pb.reset()
    got, want = session_frame(pa, ia, 3, st), session_frame(pb, ib, 3, st)
    assert_frame(got, want, case)
    assert (got[2]["out_history"] == 1).all()
    assert pa.planes()["frames"] == pb.planes()["frames"] == 1
    # the frame after it has a history again, in both sessions alike
    got, want = session_frame(pa, ia, 4, st), session_frame(pb, ib, 4, st)
    assert_frame(got, want, case + ", the next frame")
    assert (got[2]["out_history"] > 1).sum() > 100
    for x in (pa, pb, ds_a, ds_b):
        x.close()


# ---- 3: usage, and a scene that is never updated ------------------------------------------------------------------
def test_usage_is_unchanged_and_a_static_scene_gives_the_static_chain():
    import torch
    ds_s, ds_h = rt.DeviceScene(records(0)), rt.DeviceScene(records(0))
    pv, hand, img = ds_s.preview(params(DEMOD)), HandChain(ds_h, DEMOD), Images()
    usage = pv.usage()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for i in range(3):
        assert_frame(session_frame(pv, img, 1 + i, st), hand.frame(1 + i), f"frame {i}")
    assert hand.calls == ["none", "static", "static"]
    ds_s.update(records(1))
    session_frame(pv, img, 9, st)
    assert pv.usage() == usage
    for x in (pv, ds_s, ds_h):
        x.close()
