"""The progressive session on the GPU (rt_progressive_*): after every window the
resolved estimate against the CPU restatement (tests/tools/progressive_ref.py over the per-sample
colours of tests/tools/moments_ref.py), and after the last window against the one-shot calls.

Every comparison is on uint32 (or uint8) views with zero mismatches allowed. The references are
computed once per module and shared. Sizes 64 x 36 (whole 64-pixel blocks: tile classes order the
dealing) and 30 x 17 (the natural order, pixels not in whole blocks).
"""
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import moments_ref  # noqa: E402
import progressive_ref  # noqa: E402
import test_variance_gpu as TV  # noqa: E402  (its scenes and the plan variants of its render)
from motion_cases import huge_a_b  # noqa: E402
from support import assert_all_bits  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SEED = TV.SEED
TAU = 0.1
SENTINEL = dict(rgb=F(-7.0), var=F(-7.0), rgb8=np.uint8(77))
CAMERAS = TV.CAMERAS
scene = TV.scene
_SAMPLES = {}


def samples_of(scene_name, w, h, spp, mode, seed=SEED, records=None, **kw):
    """The per-sample colours of the frame (and the oracle's rgb, var), once."""
    key = (scene_name, w, h, spp, mode, seed, tuple(sorted(kw.items())))
    if key not in _SAMPLES:
        s, m = records if records is not None else scene(scene_name)
        kw_ref = {k: v for k, v in kw.items() if k not in ("brute_force", "full_frame")}  # packed rows; same bits
        _SAMPLES[key] = moments_ref.render(s, m, rt.Camera.default(w, h, mode), TV.params(w, h, spp, seed, **kw_ref))
    return _SAMPLES[key]


class Outs:
    """One set of a step's outputs on the device, filled with sentinels."""

    def __init__(self, p):
        import torch
        rows = p.height if p.flags & abi.RT_FLAG_FULL_FRAME else abi.rows_of(p)
        dev = "cuda:0"
        self.rgb = torch.full((rows, p.width, 3), float(SENTINEL["rgb"]), dtype=torch.float32, device=dev)
        self.var = torch.full((rows, p.width), float(SENTINEL["var"]), dtype=torch.float32, device=dev)
        self.rgb8 = torch.full((rows, p.width, 3), int(SENTINEL["rgb8"]), dtype=torch.uint8, device=dev)
        self.noisy = torch.full((1,), 12345, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

    def record(self):
        return rt.progressive_outputs(self.rgb.data_ptr(), self.var.data_ptr(), self.rgb8.data_ptr(), self.noisy.data_ptr(), TAU)

    def read(self):
        return dict(rgb=self.rgb.cpu().numpy(), var=self.var.cpu().numpy(), rgb8=self.rgb8.cpu().numpy(),
                    noisy=int(self.noisy.cpu().numpy()[0]))


def assert_estimate(got, want, what):
    assert_all_bits(got, want, what, ("rgb", "var", "rgb8"))
    print(what, "noisy:", got["noisy"], "expected", want["noisy"])
    assert got["noisy"] == want["noisy"], f"{what}: noise count"


def run_session(ds, cam, p, windows, stream=None):
    """A fresh session's estimates after each window, read back after each step: [dict]."""
    import torch
    st = stream or torch.cuda.current_stream()
    pg = ds.progressive(cam, p)
    got = []
    try:
        for n in windows:
            o = Outs(p)
            pg.step(n, outputs=o.record(), stream=st.cuda_stream)
            st.synchronize()
            got.append(o.read())
        assert pg.info()["done"] == p.spp
    finally:
        pg.close()
    return got


def check_windows(scene_name, w, h, spp, mode, windows, opts=None, seed=SEED, ds=None, **kw):
    """A session on `scene_name` through `windows` against the restatement after every window; the
    final estimate is returned."""
    _, _, samples = samples_of(scene_name, w, h, spp, mode, seed, **kw)
    p = TV.params(w, h, spp, seed, **kw)
    want = [progressive_ref.place(e, p, SENTINEL) for e in progressive_ref.run(samples, windows, tau=TAU)]
    own = ds is None
    if own:
        ds = rt.DeviceScene(scene(scene_name), device=0, options=rt.options(**opts) if opts else None)
    try:
        got = run_session(ds, rt.Camera.default(w, h, mode), p, windows)
    finally:
        if own:
            ds.close()
    for i, (g, r) in enumerate(zip(got, want)):
        assert_estimate(g, r, f"after window {i + 1} of {windows}")
    return got[-1]


# ---- windows ---------------------------------------------------------------------------------------
WINDOWS = {"4-4-4-4": (16, (4, 4, 4, 4)), "8-8": (16, (8, 8)), "4-12": (16, (4, 12)), "16": (16, (16,)),
           "4-8-11": (23, (4, 8, 11))}
_ONE_SHOT = {}


def one_shot(scene_name, w, h, spp, mode):
    key = (scene_name, w, h, spp, mode)
    if key not in _ONE_SHOT:
        p, cam = TV.params(w, h, spp), rt.Camera.default(w, h, mode)
        rgb, var, _ = rt.render_var(scene(scene_name), p, cam)
        plain, _ = rt.render_f32(scene(scene_name), p, cam)
        _ONE_SHOT[key] = (rgb, var, plain)
    return _ONE_SHOT[key]


@pytest.mark.parametrize("windows", sorted(WINDOWS))
@pytest.mark.parametrize("camera", sorted(CAMERAS))
@pytest.mark.parametrize("scene_name", ["huge", "glass"])
def test_every_window_is_the_restatements_prefix(scene_name, camera, windows):
    """rgb, var, rgb8 and the noise count after every window; after the last one also the one-shot
    render_var and render_f32. The tail of 3 of the 23-sample frame arrives with the last window."""
    spp, wins = WINDOWS[windows]
    last = check_windows(scene_name, 64, 36, spp, CAMERAS[camera], wins)
    rgb, var, plain = one_shot(scene_name, 64, 36, spp, CAMERAS[camera])
    TV.assert_same(last["rgb"], rgb, "rgb against render_var")
    TV.assert_same(last["var"], var, "var against render_var")
    TV.assert_same(last["rgb"], plain, "rgb against render_f32")


def test_one_window_of_four_is_the_golden_frame():
    import golden_io as G
    last = check_windows("huge", 64, 36, 4, rt.REFERENCE, (4,))
    gold = np.fromfile(os.path.join(G.GOLDEN, "huge_64x36_s4.f32"), dtype=F).reshape(36, 64, 3)
    gold8 = np.fromfile(os.path.join(G.GOLDEN, "huge_64x36_s4.u8"), dtype=np.uint8).reshape(36, 64, 3)
    TV.assert_same(last["rgb"], gold, "rgb against the golden frame")
    assert np.array_equal(last["rgb8"], gold8)


@pytest.mark.parametrize("spp,windows", [(7, (4, 3)), (7, (7,)), (2, (2,)), (3, (3,)), (3, (4,))],
                         ids=["7-in-4-3", "7-in-7", "2", "3", "3-asked-4"])
def test_natural_order_and_short_frames(spp, windows):
    """30 x 17: pixels not in whole 64-blocks, the natural order; 2 and 3 samples: one window only."""
    m = [progressive_ref.window(spp, 0, windows[0])] + list(windows[1:])
    _, _, samples = samples_of("huge", 30, 17, spp, rt.REFERENCE)
    want = progressive_ref.run(samples, m, tau=TAU)
    ds = rt.DeviceScene(scene("huge"), device=0)
    try:
        got = run_session(ds, rt.Camera.default(30, 17), TV.params(30, 17, spp), windows)
    finally:
        ds.close()
    for i, (g, r) in enumerate(zip(got, want)):
        assert_estimate(g, r, f"after window {i + 1}")
    oracle_rgb, oracle_var, _ = samples_of("huge", 30, 17, spp, rt.REFERENCE)
    TV.assert_same(got[-1]["rgb"], oracle_rgb, "rgb against the oracle")
    TV.assert_same(got[-1]["var"], oracle_var, "var against the oracle")


# ---- plans and layouts -----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(TV.VARIANTS))
def test_plan_variants(variant):
    """Every cut of test_variance_gpu: one window of 16 (under `four-passes` a window of four passes)
    and windows of 8, on one scene with the variant's options."""
    scene_name, opts, kw = TV.VARIANTS[variant]
    ds = rt.DeviceScene(scene(scene_name), device=0, options=rt.options(**opts) if opts else None)
    try:
        check_windows(scene_name, 64, 36, 16, rt.REFERENCE, (16,), ds=ds, **kw)
        usage = ds.usage()
        print("usage after one window of 16:", usage)
        check_windows(scene_name, 64, 36, 16, rt.REFERENCE, (8, 8), ds=ds, **kw)
    finally:
        ds.close()
    assert usage["pair_passes"] == 0 and usage["sky_tiles"] == 0, usage
    if "four-passes" in variant:
        assert usage["pass_samples"] == 4, usage
    if variant.startswith("deep"):
        assert usage["split_passes"] >= 1, usage


@pytest.mark.parametrize("layout", ["packed-rows", "full-frame-rows"])
def test_rows_and_layout(layout):
    """Rows 1, 4, 7, ... packed and at their global position; rows not rendered keep their sentinel."""
    kw = dict(row_offset=1, row_stride=3, full_frame=True) if layout == "full-frame-rows" else dict(row_offset=1, row_stride=3)
    last = check_windows("huge", 64, 36, 7, rt.REFERENCE, (4, 3), **kw)
    assert last["rgb"].shape[0] == (36 if layout == "full-frame-rows" else 12)
    if layout == "full-frame-rows":
        rest = np.ones(36, dtype=bool)
        rest[1::3] = False
        assert (last["rgb"][rest] == SENTINEL["rgb"]).all() and (last["var"][rest] == SENTINEL["var"]).all()
        assert (last["rgb8"][rest] == SENTINEL["rgb8"]).all()


def test_only_the_planes_given_are_written_and_the_session_reports_its_bytes():
    import torch
    w, h, spp = 64, 36, 8
    _, _, samples = samples_of("huge", w, h, spp, rt.REFERENCE)
    want = progressive_ref.run(samples, (4, 4), tau=TAU)
    p, cam = TV.params(w, h, spp), rt.Camera.default(w, h)
    ds = rt.DeviceScene(scene("huge"), device=0)
    try:
        before = ds.usage()
        pg = ds.progressive(cam, p)
        assert ds.usage() == before  # rt_scene_usage does not count a session
        assert pg.info() == dict(done=0, spp=spp, n_pixels=w * h, state_bytes=128 + 24 * w * h, device_bytes=24 * w * h)
        a, b, c = Outs(p), Outs(p), Outs(p)
        pg.step(4, rgb8_ptr=a.rgb8.data_ptr())
        pg.step(0, variance_ptr=b.var.data_ptr())       # no samples: the estimate after 4 again
        pg.step(4)                                      # no resolve
        pg.step(0, noisy_ptr=c.noisy.data_ptr(), noise_tau=TAU)
        torch.cuda.synchronize()
        assert pg.info()["done"] == 8
        pg.step(4)                                      # the frame is complete: nothing to render
        assert pg.info()["done"] == 8
        pg.close()
        # refusals with a live session leave it as it was
        fresh = ds.progressive(cam, p)
        for n, kw, word in ((3, {}, "n_samples"), (0, dict(rgb_ptr=a.rgb.data_ptr()), "done")):
            with pytest.raises(rt.RtError) as e:
                fresh.step(n, **kw)
            assert e.value.status == abi.RT_ERR_INVALID and word in str(e.value), str(e.value)
        assert fresh.info()["done"] == 0
        fresh.close()
    finally:
        ds.close()
    ga, gb, gc = a.read(), b.read(), c.read()
    assert np.array_equal(ga["rgb8"], want[0]["rgb8"]) and (ga["rgb"] == SENTINEL["rgb"]).all() and ga["noisy"] == 12345
    TV.assert_same(gb["var"], want[0]["var"], "var alone")
    assert (gb["rgb"] == SENTINEL["rgb"]).all() and (gb["rgb8"] == SENTINEL["rgb8"]).all()
    assert gc["noisy"] == want[1]["noisy"] and (gc["rgb"] == SENTINEL["rgb"]).all() and (gc["var"] == SENTINEL["var"]).all()


# ---- interleaving and stream order -----------------------------------------------------------------
def test_two_sessions_and_other_renders_interleaved():
    """Two sessions with different cameras and seeds, step by step on one scene whose passes hold 4
    samples, with a multi-pass plain render and a multi-pass variance render (which use the scene's
    own sums) between the steps: each session ends on its own frame."""
    import torch
    w, h, spp = 64, 36, 16
    cases = [(rt.REFERENCE, SEED), (rt.CORRECTED, SEED + 5)]
    refs = [samples_of("huge", w, h, spp, mode, seed) for mode, seed in cases]
    other = samples_of("huge", w, h, spp, rt.REFERENCE, SEED + 9)
    ds = rt.DeviceScene(scene("huge"), device=0, options=rt.options(max_pass_bytes=w * h * 12 * 4))
    try:
        ps = [TV.params(w, h, spp, seed) for _, seed in cases]
        cams = [rt.Camera.default(w, h, mode) for mode, _ in cases]
        pgs = [ds.progressive(c, p) for c, p in zip(cams, ps)]
        outs = [Outs(p) for p in ps]
        plain, varied = Outs(ps[0]), Outs(ps[0])
        po = TV.params(w, h, spp, SEED + 9)
        for i in range(4):
            pgs[0].step(4, outputs=outs[0].record())
            if i == 1:
                ds.render(cams[0], po, plain.rgb.data_ptr())
            pgs[1].step(4, outputs=outs[1].record())
            if i == 2:
                ds.render_var(cams[0], po, varied.rgb.data_ptr(), varied.var.data_ptr())
        torch.cuda.synchronize()
        assert ds.usage()["pass_samples"] == 4
        for pg in pgs:
            pg.close()
    finally:
        ds.close()
    for o, (rgb, var, _) in zip(outs, refs):
        g = o.read()
        TV.assert_same(g["rgb"], rgb, "a session's rgb")
        TV.assert_same(g["var"], var, "a session's var")
    TV.assert_same(plain.read()["rgb"], other[0], "the plain render between")
    TV.assert_same(varied.read()["rgb"], other[0], "the variance render between: rgb")
    TV.assert_same(varied.read()["var"], other[1], "the variance render between: var")


def test_three_steps_back_to_back_in_stream_order():
    """Three steps into three output sets on a side stream without a host wait."""
    import torch
    w, h, spp, windows = 64, 36, 23, (4, 8, 11)
    _, _, samples = samples_of("huge", w, h, spp, rt.REFERENCE)
    want = progressive_ref.run(samples, windows, tau=TAU)
    p = TV.params(w, h, spp)
    outs = [Outs(p) for _ in windows]
    st = torch.cuda.Stream()
    ds = rt.DeviceScene(scene("huge"), device=0)
    try:
        pg = ds.progressive(rt.Camera.default(w, h), p)
        for n, o in zip(windows, outs):
            pg.step(n, outputs=o.record(), stream=st.cuda_stream)
        st.synchronize()
        pg.close()
    finally:
        ds.close()
    for i, (o, r) in enumerate(zip(outs, want)):
        assert_estimate(o.read(), r, f"step {i + 1}")


# ---- checkpoints, reset, scene updates -------------------------------------------------------------
def test_save_destroy_everything_load_and_finish():
    import torch
    w, h, spp = 64, 36, 16
    rgb, var, samples = samples_of("huge", w, h, spp, rt.REFERENCE)
    want = progressive_ref.run(samples, (8, 8), tau=TAU)
    p, cam = TV.params(w, h, spp), rt.Camera.default(w, h)
    ds = rt.DeviceScene(scene("huge"), device=0)
    pg = ds.progressive(cam, p)
    pg.step(8)
    blob = pg.save()  # (waits for the step)
    assert len(blob) == pg.info()["state_bytes"] and rt.progressive_blob_check(blob, p, cam)["done"] == 8
    pg.close()
    ds.close()
    ds = rt.DeviceScene(scene("huge"), device=0)
    try:
        pg = ds.progressive(cam, p)
        with pytest.raises(rt.RtError) as e:
            pg.load(blob[:1000])
        assert e.value.status == abi.RT_ERR_CAPACITY
        other = ds.progressive(cam, TV.params(w, h, spp, SEED + 1))
        with pytest.raises(rt.RtError) as e:
            other.load(blob)
        assert e.value.status == abi.RT_ERR_INVALID and "params.seed" in str(e.value)
        other.close()
        pg.load(blob)
        assert pg.info()["done"] == 8
        o = Outs(p)
        pg.step(8, outputs=o.record())
        torch.cuda.synchronize()
        assert pg.save() != blob and pg.info()["done"] == 16
        pg.close()
    finally:
        ds.close()
    assert_estimate(o.read(), want[1], "after load and the second window")
    TV.assert_same(o.read()["rgb"], rgb, "rgb against the oracle")
    TV.assert_same(o.read()["var"], var, "var against the oracle")


def test_reset_with_a_new_seed_is_a_fresh_session():
    import torch
    w, h, spp = 64, 36, 16
    _, _, samples = samples_of("huge", w, h, spp, rt.CORRECTED, SEED + 5)
    want = progressive_ref.run(samples, (4, 12), tau=TAU)
    p = TV.params(w, h, spp)
    ds = rt.DeviceScene(scene("huge"), device=0)
    try:
        pg = ds.progressive(rt.Camera.default(w, h), p)
        pg.step(8)
        pg.reset(camera=rt.Camera.default(w, h, rt.CORRECTED), seed=SEED + 5)
        assert pg.info()["done"] == 0
        outs = [Outs(p), Outs(p)]
        for n, o in zip((4, 12), outs):
            pg.step(n, outputs=o.record())
        torch.cuda.synchronize()
        pg.close()
    finally:
        ds.close()
    for i, (o, r) in enumerate(zip(outs, want)):
        assert_estimate(o.read(), r, f"after reset, window {i + 1}")


def test_a_scene_update_is_refused_until_reset():
    import torch
    w, h, spp = 64, 36, 8
    a, b = huge_a_b()
    _, _, samples = samples_of("huge-b", w, h, spp, rt.REFERENCE, records=b)
    want = progressive_ref.run(samples, (4, 4), tau=TAU)
    p = TV.params(w, h, spp)
    ds = rt.DeviceScene(a, device=0)
    try:
        pg = ds.progressive(rt.Camera.default(w, h), p)
        pg.step(4)
        ds.update(b)
        with pytest.raises(rt.RtError) as e:
            pg.step(4)
        assert e.value.status == abi.RT_ERR_INVALID and "updated" in str(e.value)
        assert pg.info()["done"] == 4
        pg.reset()
        outs = [Outs(p), Outs(p)]
        for o in outs:
            pg.step(4, outputs=o.record())
        torch.cuda.synchronize()
        pg.close()
    finally:
        ds.close()
    for i, (o, r) in enumerate(zip(outs, want)):
        assert_estimate(o.read(), r, f"on the updated scene, window {i + 1}")
