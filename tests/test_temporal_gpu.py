"""Temporal accumulation on the GPU (rt_temporal, rt_temporal_device) against its
numpy restatement (tests/tools/temporal_ref.py).

Every comparison is on uint32 views with zero mismatches allowed. Frames are rendered once per
module (rt.render_var and rt.render_aov, whose bits other modules check) and shared; the conditions
that make a case meaningful (which reasons occur, how many pixels keep their history) are checked on
the restatement's result alone. The camera moves were chosen on the CPU so that they hold.
"""
import functools
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import denoise_var_ref  # noqa: E402
import temporal_ref as T  # noqa: E402
from device_io import SENTINEL  # noqa: E402
from support import LOOK, POS, frame_planes, shifted_camera as camera  # noqa: E402
from support import assert_all_bits as assert_all_same, assert_bits as assert_same  # noqa: E402
from support import census as reason_census  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SCENE_SEED = 1234
SPP = 4
MODES = {"reference": rt.REFERENCE, "corrected": rt.CORRECTED}
# (position shift, look-at shift) after which part of the previous frame has left the screen. In
# REFERENCE mode a ray's direction is the image-plane point itself, so the picture depends on the
# camera's position far more strongly and the move is smaller.
MOVES = {"reference": ((0.1, 0.05, -0.05), (0.15, 0.05, 0.0)), "corrected": ((0.6, 0.1, -0.3), (1.0, 0.2, 0.0))}
CUR = ("beauty", "variance", "normal", "depth", "alpha", "sphere_id")
PREV = ("color", "variance", "history", "normal", "depth", "sphere_id")


@functools.lru_cache(maxsize=None)
def scene():
    return rt.huge_scene_arrays(SCENE_SEED)


AWAY = ((0.0, 0.0, 0.0), tuple(2 * (np.array(POS) - np.array(LOOK))))  # looks along -w of the default camera


@functools.lru_cache(maxsize=None)
def frame(w, h, mode, seed, shift=((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), albedo=False):
    """The planes of one frame of the huge scene: beauty and variance of SPP samples, the guides of
    the same samples."""
    return frame_planes(scene(), rt.make_params(w, h, SPP, 64, seed), camera(w, h, mode, shift), SPP,
                        ("normal", "depth", "alpha", "sphere_id") + (("albedo",) if albedo else ()))


def cur_of(f):
    return {n: f[n] for n in CUR}


def prev_of(f, color=None, variance=None, history=None):
    """A frame as the previous one: its own beauty and variance with a history of 1, or the
    accumulated planes given."""
    h, w = f["variance"].shape
    return dict(color=f["beauty"] if color is None else color, variance=f["variance"] if variance is None else variance,
                history=np.ones((h, w), dtype=F) if history is None else history,
                normal=f["normal"], depth=f["depth"], sphere_id=f["sphere_id"])


census = functools.partial(reason_census, reasons=T.REASONS)


def device_call(cur, prev, cam, prev_cam, par):
    """rt_temporal_device on a torch stream of its own into sentinel-filled outputs."""
    import torch
    h, w = cur["variance"].shape

    def up(a):
        a = np.array(a)  # a writable copy (the shared frames are read-only)
        return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")

    t = {n: up(cur[n]) for n in CUR}
    if prev is not None:
        t.update({"prev_" + n: up(prev[n]) for n in PREV})
    out = {n: torch.full((h, w, 3) if n == "out_color" else (h, w), SENTINEL, dtype=torch.float32, device="cuda:0")
           for n in ("out_color", "out_variance", "out_history")}
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        rt.temporal_device({n: a.data_ptr() for n, a in {**t, **out}.items()}, par, cam, prev_cam, st.cuda_stream)
    st.synchronize()
    return tuple(out[n].cpu().numpy() for n in ("out_color", "out_variance", "out_history"))


# ---- 1: no history ---------------------------------------------------------------------------------
def test_no_history_copies_the_current_frame():
    w, h = 64, 36
    f = frame(w, h, rt.REFERENCE, 1)
    par = rt.temporal_params(w, h)
    for got in (rt.temporal(cur_of(f), None, camera(w, h, rt.REFERENCE), None, par),
                device_call(cur_of(f), None, camera(w, h, rt.REFERENCE), None, par)):
        assert_same(got[0], f["beauty"], "color")
        assert_same(got[1], f["variance"], "variance")
        assert (got[2] == 1.0).all()
    ref = T.accumulate(cur_of(f), None, camera(w, h, rt.REFERENCE), None, par)
    assert (ref[3] == T.NO_PREV).all()
    assert_all_same(got, ref[:3])


# ---- 2: static camera, two seeds ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_static_camera_two_seeds(mode):
    w, h, m = 64, 36, MODES[mode]
    f1, f2, cam = frame(w, h, m, 1), frame(w, h, m, 2), camera(w, h, m)
    par = rt.temporal_params(w, h, alpha_min=0.2, max_history=32.0, normal_tol=0.1, depth_tol=0.1)
    ref = T.accumulate(cur_of(f2), prev_of(f1), cam, cam, par)
    census(ref[3])
    both = (f1["alpha"] == 1) & (f2["alpha"] == 1)
    kept2 = both & (ref[3] == T.KEPT) & (ref[2] == 2.0)
    print("alpha == 1 in both frames:", int(both.sum()), "of those kept with history 2:", int(kept2.sum()))
    assert both.sum() > 100 and 2 * kept2.sum() >= both.sum()
    assert_all_same(rt.temporal(cur_of(f2), prev_of(f1), cam, cam, par), ref[:3], "host")
    assert_all_same(device_call(cur_of(f2), prev_of(f1), cam, cam, par), ref[:3], "device")


# ---- 3: moved camera, 7: the chain into the filter ----------------------------------------------------
MOVED = [(mode, w, h) for mode in sorted(MODES) for w, h in ((64, 36), (48, 27))]


@functools.lru_cache(maxsize=None)
def moved(mode, w, h):
    """The moved-camera case's inputs and the restatement's result, once."""
    m = MODES[mode]
    f1, f2 = frame(w, h, m, 1), frame(w, h, m, 2, MOVES[mode], albedo=True)
    cam, prev_cam = camera(w, h, m, MOVES[mode]), camera(w, h, m)
    par = rt.temporal_params(w, h, alpha_min=0.2, max_history=32.0, normal_tol=0.1, depth_tol=0.1)
    return f1, f2, cam, prev_cam, par, T.accumulate(cur_of(f2), prev_of(f1), cam, prev_cam, par)


@pytest.mark.parametrize("mode,w,h", MOVED)
def test_moved_camera(mode, w, h):
    f1, f2, cam, prev_cam, par, ref = moved(mode, w, h)
    c = census(ref[3])
    assert min(c["kept"], c["all taps rejected"], c["off-screen"], c["edge"]) >= 1
    assert c["kept"] >= 100  # (the CPU census when the move was chosen: 753 at the least)
    assert_all_same(rt.temporal(cur_of(f2), prev_of(f1), cam, prev_cam, par), ref[:3], "host")
    assert_all_same(device_call(cur_of(f2), prev_of(f1), cam, prev_cam, par), ref[:3], "device")


@pytest.mark.parametrize("mode", sorted(MODES))
def test_chain_into_the_variance_guided_filter(mode):
    """The moved-camera case's outputs through rt.denoise_var are denoise_var_ref over the
    restatement's outputs, bit for bit: the two stages compose."""
    w, h = 64, 36
    f1, f2, cam, prev_cam, par, ref = moved(mode, w, h)
    color, variance, _ = rt.temporal(cur_of(f2), prev_of(f1), cam, prev_cam, par)
    got, got_v = rt.denoise_var(color, variance, f2["albedo"], f2["normal"], f2["depth"], variance_out=True)
    dp, dv = rt.denoise_var_params(w, h)
    want, want_v, _ = denoise_var_ref.denoise(ref[0], ref[1], f2["albedo"], f2["normal"], f2["depth"],
                                              **denoise_var_ref.params_kwargs(dp, dv))
    assert_same(got, want, "denoised")
    assert_same(got_v, want_v, "variance after the filter")


# ---- 4: behind the previous camera -------------------------------------------------------------------
# corrected: the previous camera looks along -w of the current one. In REFERENCE mode "looking away"
# has no such meaning (the directions are image-plane points); there the corrected mode's move of
# case 3 puts most of the frame behind the previous camera.
BEHIND = {"corrected": AWAY, "reference": MOVES["corrected"]}


@pytest.mark.parametrize("mode", sorted(BEHIND))
def test_points_behind_the_previous_camera(mode):
    w, h, m = 64, 36, MODES[mode]
    f_prev, f_cur = frame(w, h, m, 1, BEHIND[mode]), frame(w, h, m, 2)
    cam, prev_cam = camera(w, h, m), camera(w, h, m, BEHIND[mode])
    par = rt.temporal_params(w, h)
    ref = T.accumulate(cur_of(f_cur), prev_of(f_prev), cam, prev_cam, par)
    assert census(ref[3])["behind"] >= 100
    got = rt.temporal(cur_of(f_cur), prev_of(f_prev), cam, prev_cam, par)
    assert all(np.isfinite(a).all() for a in got)
    assert_all_same(got, ref[:3])


# ---- 5: synthetic planes -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synthetic(w, h):
    """Seeded random planes: ids from {0, 1, 2, 0xffffffff}, alpha from {0, 1, 0.5}, depth in [1, 20],
    normals from four directions (so that the normal test passes and fails), everything else
    uniform; the cameras are the default one and the corrected mode's move of case 3."""
    g = np.random.default_rng(w * 1000 + h)
    ids = np.array([0, 1, 2, 0xffffffff], dtype=np.uint32)
    dirs = np.array([[0, 1, 0], [0, 0.96, 0.28], [1, 0, 0], [0, 0, 0]], dtype=F)

    def guides():
        return dict(normal=dirs[g.integers(0, 4, (h, w))], depth=g.uniform(1, 20, (h, w)).astype(F),
                    sphere_id=ids[g.integers(0, 4, (h, w))])

    cur = dict(beauty=g.random((h, w, 3), dtype=F), variance=g.random((h, w), dtype=F) * F(0.02),
               alpha=np.array([0, 1, 0.5], dtype=F)[g.integers(0, 3, (h, w))], **guides())
    prev = dict(color=g.random((h, w, 3), dtype=F), variance=g.random((h, w), dtype=F) * F(0.02),
                history=g.integers(1, 40, (h, w)).astype(F), **guides())
    return cur, prev


SYNTHETIC = {
    "loose": dict(alpha_min=0.1, max_history=32.0, normal_tol=0.5, depth_tol=1.0),
    "zero-tolerances": dict(alpha_min=0.1, max_history=32.0, normal_tol=0.0, depth_tol=0.0),
    "max-history-1": dict(alpha_min=0.1, max_history=1.0, normal_tol=0.5, depth_tol=1.0),
}


@pytest.mark.parametrize("variant", sorted(SYNTHETIC))
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (67, 35)])
def test_synthetic_planes(w, h, variant):
    """67 x 35 is no multiple of the 64 x 4 workgroup in either axis (two blocks in x, nine in y)."""
    cur, prev = synthetic(w, h)
    cam, prev_cam = camera(w, h, rt.CORRECTED, MOVES["corrected"]), camera(w, h, rt.CORRECTED)
    par = rt.temporal_params(w, h, **SYNTHETIC[variant])
    ref = T.accumulate(cur, prev, cam, prev_cam, par)
    c = census(ref[3])
    if (w, h) == (67, 35) and variant != "zero-tolerances":
        assert min(c["kept"], c["all taps rejected"], c["edge"]) >= 20
    got = rt.temporal(cur, prev, cam, prev_cam, par)
    assert_all_same(got, ref[:3], "host")
    if (w, h) == (67, 35):
        assert_all_same(device_call(cur, prev, cam, prev_cam, par), ref[:3], "device")
    if variant == "max-history-1":
        # every k = 1: the colour is the current beauty on kept pixels too
        assert_same(got[0], cur["beauty"], "color")
        assert (got[2] == 1.0).all()


# ---- 6: a sequence -----------------------------------------------------------------------------------
def test_sequence_static_camera_eight_frames():
    """Eight frames of 4 spp (seeds 1..8) from a static camera, accumulated with alpha_min small
    enough that k = 1 / N throughout, each frame's outputs fed back as prev. The GPU's sequence is the
    restatement's bit for bit. On the pixels kept in every frame the history is the frame count (to
    7e-3: the reprojected position lies within 1e-3 of the pixel's own centre, so a neighbour's
    history, different by at most 7, enters with a weight below 1e-3), and the accumulated colour's
    MSE against a 256-spp render is below the 8th frame's own. Independent frames predict a ratio of
    about 1/8; the ratio is printed (DESIGN.md §4.11 records it)."""
    w, h, m, frames = 64, 36, rt.CORRECTED, 8
    cam = camera(w, h, m)
    par = rt.temporal_params(w, h, alpha_min=0.01, max_history=64.0, normal_tol=0.1, depth_tol=0.1)
    got = ref = None
    always = np.ones((h, w), dtype=bool)
    for i in range(frames):
        f = frame(w, h, m, 1 + i)
        if i == 0:
            got = rt.temporal(cur_of(f), None, cam, None, par)
            ref = T.accumulate(cur_of(f), None, cam, None, par)
        else:
            last = frame(w, h, m, i)
            got = rt.temporal(cur_of(f), prev_of(last, *got), cam, cam, par)
            ref = T.accumulate(cur_of(f), prev_of(last, *ref[:3]), cam, cam, par)
            always &= ref[3] == T.KEPT
        assert_all_same(got, ref[:3], f"frame {i + 1}")
    print("pixels kept in every frame:", int(always.sum()), "of", w * h)
    assert always.sum() > w * h // 4
    assert np.abs(got[2][always] - frames).max() < 7e-3
    target, _ = rt.render_f32(scene(), rt.make_params(w, h, 256, 64, 99), cam)
    last = frame(w, h, m, frames)["beauty"]

    def mse(a):
        return float(np.mean((a[always].astype(np.float64) - target[always].astype(np.float64)) ** 2))

    acc, one = mse(got[0]), mse(last)
    print(f"mse over the kept pixels: accumulated {acc:.6e}, the 8th frame alone {one:.6e}, ratio {acc / one:.4f}")
    assert acc < one


# ---- 8: aliasing ---------------------------------------------------------------------------------------
def test_aliased_outputs_are_refused_and_the_buffers_left_intact():
    import torch
    w, h = 67, 35
    cur, prev = synthetic(w, h)
    cam = camera(w, h, rt.CORRECTED)
    par = rt.temporal_params(w, h)
    t = {n: torch.from_numpy(np.ascontiguousarray(cur[n]).view(np.int32) if n == "sphere_id" else np.array(cur[n])).to("cuda:0")
         for n in CUR}
    t.update({"prev_" + n: torch.from_numpy(np.ascontiguousarray(prev[n]).view(np.int32) if n == "sphere_id"
                                            else np.array(prev[n])).to("cuda:0") for n in PREV})
    for n in ("out_color", "out_variance", "out_history"):
        t[n] = torch.full((h, w, 3) if n == "out_color" else (h, w), SENTINEL, dtype=torch.float32, device="cuda:0")
    keep = {n: a.clone() for n, a in t.items()}
    ptr = {n: a.data_ptr() for n, a in t.items()}
    for field, other in (("out_color", "beauty"), ("out_color", "prev_color"), ("out_variance", "variance"),
                         ("out_variance", "prev_depth"), ("out_history", "prev_history"), ("out_history", "alpha"),
                         ("out_variance", "out_color"), ("out_history", "out_variance")):
        q = dict(ptr)
        q[field] = ptr[other]
        with pytest.raises(rt.RtError) as e:
            rt.temporal_device(q, par, cam, cam)
        assert e.value.status == abi.RT_ERR_INVALID and field in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for n in t:
        assert torch.equal(t[n], keep[n]), n
