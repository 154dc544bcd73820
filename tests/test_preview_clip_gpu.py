"""The preview session with the history clamp on the GPU (rt_preview_set_clip).

Every comparison is on uint32 (or uint8) views with zero mismatches allowed. The huge scene at 70 x 37
(a partial column of 64 x 4 workgroups, a ragged last row), RT_PREVIEW_DEMODULATE, 4 spp, max_depth 8,
two filter levels, three frames with seeds 1..3 on the preview module's 1.5 degree orbit. A session's
frames are compared with the stage calls made by hand (rt_temporal_clip_device, through
rt.temporal_device(clip=...), in the temporal stage's place on the frames the clip is set for) and with
the restatement (tests/tools/preview_clip_ref.py), which starts from each frame's planes as the public
rt_render_var and rt_render_aov calls give them.
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
import preview_clip_ref  # noqa: E402
import device_io  # noqa: E402
from device_io import SENTINEL, read_planes  # noqa: E402
from support import assert_bits as assert_same, frame_planes, orbit_camera, words as u32  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, MAX_DEPTH, LEVELS, FRAMES = 70, 37, 4, 8, 2, 3
OUT_W, OUT_H = 105, 56
DEMOD, NO_TEMPORAL = abi.RT_PREVIEW_DEMODULATE, abi.RT_PREVIEW_NO_TEMPORAL
MOVED_IDS = (2, 3, 4)
GUIDES = ("normal", "depth", "alpha", "sphere_id")


def clip():
    return rt.temporal_clip(radius=2, gamma=1.0)


@functools.lru_cache(maxsize=None)
def records(step=0):
    """The huge scene with spheres 2, 3 and 4 moved by `step` x (0, 0, 0.15)."""
    s, m = rt.huge_scene_arrays(1234)
    s = s.copy()
    for i in MOVED_IDS:
        s["center"][i, 2] = s["center"][i, 2] + F(0.15) * F(step)
    return s, m


@functools.lru_cache(maxsize=None)
def device_scene():
    return rt.DeviceScene(records(), device=0)


def camera(i, w=W, h=H):
    return orbit_camera(w, h, i)


@functools.lru_cache(maxsize=None)
def frame(i):
    """Frame i's planes (seed 1 + i) from the public synchronous calls."""
    return frame_planes(records(), rt.make_params(W, H, SPP, MAX_DEPTH, 1 + i), camera(i))


def params(flags=DEMOD, w=W, h=H):
    return rt.preview_params(w, h, SPP, flags=flags, max_depth=MAX_DEPTH, denoise=dict(levels=LEVELS))


@functools.lru_cache(maxsize=None)
def reference(schedule):
    """The restatement's frames with the clip set (True) or off (False) before each frame, once."""
    s = preview_clip_ref.Session(params())
    out = []
    for i, on in enumerate(schedule):
        s.set_clip(clip() if on else None)
        out.append(s.frame(frame(i), camera(i)))
    return tuple(out)


def plane(ch, dtype=None, w=W, h=H):
    return device_io.plane(w, h, ch, dtype)


def Images(w=W, h=H):
    """Sentinel-filled device images; the caller brings the stream."""
    return device_io.Outputs(w, h, own_stream=False)


class HandChain:
    """The seven stage calls of a DEMODULATE frame on planes of the test's own, with the session's
    bookkeeping restated (history iff a previous frame exists and the scene's geometry epoch is that
    frame's or one more; the motion tables iff one more) and the clip record of the frame, if any,
    passed to the temporal call."""

    def __init__(self, ds):
        import torch
        self.ds, self.p = ds, params()
        self.beauty, self.variance, self.albedo, self.alpha = plane(3), plane(1), plane(3), plane(1)
        self.illum, self.illum_var = plane(3), plane(1)
        self.g = [dict(normal=plane(3), depth=plane(1), sphere_id=plane(1, torch.int32)) for _ in range(2)]
        self.hist = [dict(color=plane(3), variance=plane(1), history=plane(1)) for _ in range(2)]
        self.filtered, self.scratch, self.var_scratch = plane(3), plane(3), plane(2)
        self.img = Images()
        self.frames, self.cur, self.epoch, self.prev_cam = 0, 0, None, None
        self.calls = []
        torch.cuda.synchronize()
        self.st = torch.cuda.Stream()

    def frame(self, cam, seed, clip_record):
        st, p, c, o = self.st.cuda_stream, self.p, self.cur, 1 - self.cur
        rp = rt.make_params(W, H, SPP, MAX_DEPTH, seed)
        mo = self.ds.motion()
        history = self.frames > 0 and mo["geometry_epoch"] - self.epoch <= 1
        moved = history and mo["geometry_epoch"] != self.epoch
        g, hist = self.g[c], self.hist[c]
        self.ds.render_var(cam, rp, self.beauty.data_ptr(), self.variance.data_ptr(), st)
        self.ds.render_aov(cam, rp, dict(albedo=self.albedo.data_ptr(), alpha=self.alpha.data_ptr(),
                                         **{n: a.data_ptr() for n, a in g.items()}), 0, st)
        rt.preview_split_device(W, H, self.beauty.data_ptr(), self.variance.data_ptr(), self.albedo.data_ptr(),
                                self.illum.data_ptr(), self.illum_var.data_ptr(), st)
        ptrs = dict(beauty=self.illum, variance=self.illum_var, alpha=self.alpha, **g, out_color=hist["color"],
                    out_variance=hist["variance"], out_history=hist["history"])
        if history:
            ptrs.update({"prev_" + n: a for n, a in {**self.hist[o], **self.g[o]}.items()})
        rt.temporal_device({n: a.data_ptr() for n, a in ptrs.items()}, p.temporal, cam, self.prev_cam if history else None, st,
                           motion=(mo["centres"], mo["prev_centres"], mo["n_spheres"]) if moved else None, clip=clip_record)
        self.calls.append(("motion" if moved else "static" if history else "none") + ("+clip" if clip_record is not None else ""))
        rt.denoise_var_device(dict(beauty=hist["color"].data_ptr(), albedo=self.albedo.data_ptr(), normal=g["normal"].data_ptr(),
                                   depth=g["depth"].data_ptr(), out=self.filtered.data_ptr(), scratch=self.scratch.data_ptr()),
                              p.denoise, render.denoise_var_buffers(dict(variance=hist["variance"].data_ptr(),
                                                                         var_scratch=self.var_scratch.data_ptr()), p.var_floor), st)
        rt.preview_merge_device(W, H, self.filtered.data_ptr(), self.albedo.data_ptr(), self.img.rgb.data_ptr(),
                                self.img.rgb8.data_ptr(), st)
        self.st.synchronize()
        self.frames = self.frames + 1 if history else 1
        self.cur, self.epoch, self.prev_cam = o, mo["geometry_epoch"], cam
        planes = {"out_" + n: a.cpu().numpy() for n, a in hist.items()}
        planes.update({"prev_" + n: a.cpu().numpy() for n, a in hist.items()})
        planes.update(albedo=self.albedo.cpu().numpy(), alpha=self.alpha.cpu().numpy())
        for n, a in g.items():
            planes[n] = planes["prev_" + n] = a.cpu().numpy().view(abi.PREVIEW_PLANES[n][1])
        return (*self.img.host(), planes)


def session_frame(pv, img, cam, seed, stream, w=W, h=H):
    pv.frame(cam, seed, img.rgb.data_ptr(), img.rgb8.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return (*img.host(), read_planes(pv, w, h))


def assert_frame(got, want, what):
    rgb, rgb8, pl = got
    assert (rgb != SENTINEL).all()
    assert_same(rgb, want[0], f"{what} rgb")
    assert np.array_equal(rgb8, want[1]), f"{what} rgb8"
    for n, a in want[2].items():
        assert_same(pl[n], a, f"{what} plane {n}")


# ---- 1: an ordinary session, the clip set or cleared between frames ----------------------------------------
# always on; turned off after two clipped frames (the third is the plain call on the clipped history);
# turned on after a plain frame and off again
SCHEDULES = {"on-on-on": (True, True, True), "on-on-off": (True, True, False), "off-on-off": (False, True, False)}


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_session_equals_the_hand_chain_and_the_restatement(name):
    import torch
    schedule = SCHEDULES[name]
    pv, hand, img = device_scene().preview(params()), HandChain(device_scene()), Images()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    ref, plain = reference(schedule), reference((False,) * FRAMES)
    for i, on in enumerate(schedule):
        pv.set_clip(clip() if on else None)
        want = hand.frame(camera(i), 1 + i, clip() if on else None)
        got = session_frame(pv, img, camera(i), 1 + i, st)
        assert_frame(got, want, f"frame {i}")
        assert pv.planes()["frames"] == i + 1
        r = ref[i]
        assert_same(got[0], r["out"], f"frame {i} out against the restatement")
        for n in ("color", "variance", "history"):
            assert_same(got[2]["out_" + n], r[n], f"frame {i} out_{n} against the restatement")
        if on and i:
            # the case says something: the clamp changed pixels with history and left others alone (the
            # sky's illumination is 1 everywhere: its box is a point that holds the history)
            kept, changed = int((r["history"] > 1).sum()), int(r["info"]["changed"].sum())
            print(f"frame {i}: pixels with history {kept}, a channel changed by the clamp on {changed}")
            assert kept > W * H // 4 and changed >= 100 and kept - changed >= 100
    assert hand.calls == ["none" + ("+clip" if schedule[0] else "")] + ["static" + ("+clip" if on else "") for on in schedule[1:]]
    # the last frame differs from the session that never had a clip
    assert (u32(ref[-1]["out"]) != u32(plain[-1]["out"])).any()
    pv.close()


# ---- 2: an upscaled session ---------------------------------------------------------------------------------
def test_upscaled_session_with_clip():
    """Render 70 x 37, shown at 105 x 56, under the output's camera: the render-size planes are those of
    the stage calls made by hand at that camera (HandChain, rt_temporal_clip_device in the temporal
    stage's place), and the image is the guided upsample and the merge made by hand over the chain's
    filter output with output-size guides."""
    import torch
    p = params()
    u = rt.preview_upscale(p, OUT_W, OUT_H)
    ds = device_scene()
    upscaled, chain = ds.preview(p, u), HandChain(ds)
    upscaled.set_clip(clip())
    own, hand = Images(OUT_W, OUT_H), Images(OUT_W, OUT_H)
    g = dict(albedo=plane(3, w=OUT_W, h=OUT_H), normal=plane(3, w=OUT_W, h=OUT_H), depth=plane(1, w=OUT_W, h=OUT_H),
             alpha=plane(1, w=OUT_W, h=OUT_H), sphere_id=plane(1, torch.int32, w=OUT_W, h=OUT_H))
    upsampled = plane(3, w=OUT_W, h=OUT_H)
    up_params = rt.upsample_params(OUT_W, OUT_H, W, H, normal_tol=u.normal_tol, depth_tol=u.depth_tol)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for i in range(FRAMES):
        cam, seed = camera(i, OUT_W, OUT_H), 1 + i
        lo = chain.g[chain.cur]  # the guides this frame's chain writes (the chain flips after the frame)
        _, _, want_planes = chain.frame(cam, seed, clip())
        ds.render_aov(cam, rt.make_params(OUT_W, OUT_H, SPP, MAX_DEPTH, seed), {n: t.data_ptr() for n, t in g.items()}, 0,
                      st.cuda_stream)
        rt.upsample_device(dict(lo_color=chain.filtered.data_ptr(), lo_normal=lo["normal"].data_ptr(),
                                lo_depth=lo["depth"].data_ptr(), lo_sphere_id=lo["sphere_id"].data_ptr(),
                                out_color=upsampled.data_ptr(), **{n: g[n].data_ptr() for n in GUIDES}), up_params,
                           st.cuda_stream)
        rt.preview_merge_device(OUT_W, OUT_H, upsampled.data_ptr(), g["albedo"].data_ptr(), hand.rgb.data_ptr(),
                                hand.rgb8.data_ptr(), st.cuda_stream)
        st.synchronize()
        rgb, rgb8, got_planes = session_frame(upscaled, own, cam, seed, st)
        assert (rgb != SENTINEL).all()
        assert_same(rgb, hand.host()[0], f"frame {i} d_rgb")
        assert np.array_equal(rgb8, hand.host()[1]), f"frame {i} d_rgb8"
        for n, a in want_planes.items():
            assert_same(got_planes[n], a, f"frame {i} render-size plane {n}")
    assert chain.calls == ["none+clip", "static+clip", "static+clip"]
    upscaled.close()


def test_upscaled_render_size_planes_are_the_restatement():
    """(The orbit camera of the render size's own aspect, as the restatement's frames have it.)"""
    import torch
    p = params()
    pv = device_scene().preview(p, rt.preview_upscale(p, OUT_W, OUT_H))
    pv.set_clip(clip())
    img = Images(OUT_W, OUT_H)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    ref = reference((True,) * FRAMES)
    for i in range(FRAMES):
        _, _, pl = session_frame(pv, img, camera(i), 1 + i, st)
        for n in ("color", "variance", "history"):
            assert_same(pl["out_" + n], ref[i][n], f"frame {i} out_{n}")
    pv.close()


# ---- 3: moving spheres: the session passes its tables as before ----------------------------------------------
def test_clip_under_moving_spheres():
    import torch
    ds_s, ds_h = rt.DeviceScene(records(0)), rt.DeviceScene(records(0))
    pv, hand, img = ds_s.preview(params()), HandChain(ds_h), Images()
    pv.set_clip(clip())
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    cam = camera(0)
    for i, step in enumerate((None, None, 1)):
        if step is not None:
            ds_s.update(records(step))
            ds_h.update(records(step))
        want = hand.frame(cam, 1 + i, clip())
        assert_frame(session_frame(pv, img, cam, 1 + i, st), want, f"frame {i}")
    assert hand.calls == ["none+clip", "static+clip", "motion+clip"]
    on_moved = np.isin(want[2]["sphere_id"], MOVED_IDS)
    kept = int((want[2]["out_history"][on_moved] > 1).sum())
    print("pixels on a moved sphere that kept their history:", kept)
    assert kept >= 20
    pv.close()
    ds_s.close()
    ds_h.close()


# ---- 4: refusals ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_session_as_it_was():
    import torch
    no_temporal = device_scene().preview(params(NO_TEMPORAL | DEMOD))
    for record in (clip(), None):
        with pytest.raises(rt.RtError) as e:
            no_temporal.set_clip(record)
        assert e.value.status == abi.RT_ERR_INVALID and "NO_TEMPORAL" in str(e.value)
    no_temporal.close()
    pv, img = device_scene().preview(params()), Images()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    pv.set_clip(clip())
    for field, value in (("radius", 0), ("radius", 4), ("gamma", -1.0), ("gamma", float("nan")), ("flags", 2), ("size", 8)):
        bad = clip()
        setattr(bad, field, value)
        with pytest.raises(rt.RtError) as e:
            pv.set_clip(bad)
        assert e.value.status == abi.RT_ERR_INVALID and "clip." + field in str(e.value) and "rt_preview_set_clip" in str(e.value)
    # the good record set before is still the session's
    ref = reference((True,) * FRAMES)
    for i in range(2):
        rgb, _, _ = session_frame(pv, img, camera(i), 1 + i, st)
        assert_same(rgb, ref[i]["out"], f"frame {i} after the refusals")
    pv.close()
