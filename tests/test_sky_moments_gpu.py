"""rt_options.sky_moments = 1 on the GPU (sky_moments_kernel): frames that carry
per-pixel moments hand their proven-sky tiles to the sky kernel's moments form. The option changes no
bit, so every frame, window, step and preview output is compared with what the references of the
existing tests give (tests/tools: moments_ref, progressive_ref, adaptive_ref) or with the same calls
on a scene without the option, on uint32 (or uint8) views with zero mismatches allowed.

Every case meant to exercise the kernel asserts rt_scene_usage's sky_tiles > 0 and pair_passes == 0
after the call: a plan that fell back to the main launch fails. The huge scene at 64 x 36: 22 of its
36 tiles are proven sky with the reference camera, none with the corrected camera at its default
position (that camera's frames stay in the main launch and must not change), 16 with the corrected
camera looking at (0, 3, 0). References are computed once per process and shared with the modules
this one borrows its helpers from.
"""
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import adaptive_cases as AC  # noqa: E402
import adaptive_ref  # noqa: E402
import moments_ref  # noqa: E402
import progressive_ref  # noqa: E402
import test_adaptive_gpu as TA  # noqa: E402  (its output sets and step comparison)
import test_progressive_gpu as TP  # noqa: E402  (its output sets and estimate comparison)
import test_variance_gpu as TV  # noqa: E402  (its scenes, params, references and plan variants)
from support import words  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SEED = 64, 36, TV.SEED
ON = dict(sky_moments=1)
SKY_TILES = 22  # tests/golden/plan_usage.json: the reference camera's proven-sky tiles at 64 x 36


def camera(name, w=W, h=H):
    if name == "corrected-up":  # the corrected camera with sky tiles: the default position, looking higher
        pos, look = (-4.0, 3.2, 5.0), (0.0, 3.0, 0.0)
        focus = float(F(np.linalg.norm(np.subtract(pos, look).astype(F))))
        return rt.Camera(pos, look, (0, 1, 0), w / h, 42.0, 0.0625, focus, rt.CORRECTED)
    return rt.Camera.default(w, h, TV.CAMERAS[name])


_REFS = {}


def reference(cam_name, w, h, spp, **kw):
    """moments_ref's (rgb, var, samples) of the huge scene's frame, once (packed rows: the same bits)."""
    key = (cam_name, w, h, spp, tuple(sorted(kw.items())))
    if key not in _REFS:
        if cam_name in TV.CAMERAS and "row_stride" not in kw:
            _REFS[key] = TP.samples_of("huge", w, h, spp, TV.CAMERAS[cam_name], **kw)  # shared with that module
        else:
            kw_ref = {k: v for k, v in kw.items() if k not in ("brute_force", "full_frame")}
            s, m = TV.scene("huge")
            _REFS[key] = moments_ref.render(s, m, camera(cam_name, w, h), TV.params(w, h, spp, **kw_ref))
    return _REFS[key]


def place(plane, p, sentinel=TV.SENTINEL):
    """A packed plane at the rows of a full-frame call; the rows not rendered hold the sentinel."""
    if not p.flags & abi.RT_FLAG_FULL_FRAME:
        return plane
    out = np.full((p.height,) + plane.shape[1:], sentinel, dtype=plane.dtype)
    out[p.row_offset::p.row_stride or 1] = plane
    return out


def var_frame(p, cam, opts, records=None, ds=None):
    """rt_render_var_device into sentinel-filled planes: (rgb, var, segments, usage)."""
    import torch
    rows = p.height if p.flags & abi.RT_FLAG_FULL_FRAME else abi.rows_of(p)
    rgb = torch.full((rows, p.width, 3), TV.SENTINEL, dtype=torch.float32, device="cuda:0")
    var = torch.full((rows, p.width), TV.SENTINEL, dtype=torch.float32, device="cuda:0")
    seg = torch.zeros((3,), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    own = ds is None
    if own:
        ds = rt.DeviceScene(records or TV.scene("huge"), device=0, options=rt.options(**opts) if opts else None)
    try:
        ds.render_var(cam, p, rgb.data_ptr(), var.data_ptr(), torch.cuda.current_stream().cuda_stream, seg.data_ptr())
        usage = ds.usage()
        torch.cuda.synchronize()
    finally:
        if own:
            ds.close()
    return rgb.cpu().numpy(), var.cpu().numpy(), seg.cpu().numpy(), usage


def assert_kernel_ran(usage, n_sky=None):
    assert usage["sky_tiles"] > 0 and usage["pair_passes"] == 0, usage
    if n_sky is not None:
        assert usage["sky_tiles"] == n_sky, usage


def check_frame(cam_name, spp, opts=None, w=W, h=H, sky=True, **kw):
    """The variance frame under `opts` + sky_moments against the oracle and against the same call
    without sky_moments (the segment count, and that call's sky_tiles == 0); the usage with the option on."""
    p, cam = TV.params(w, h, spp, **kw), camera(cam_name, w, h)
    ref_rgb, ref_var, _ = reference(cam_name, w, h, spp, **kw)
    rgb, var, seg, usage = var_frame(p, cam, dict(opts or {}, **ON))
    off_rgb, off_var, off_seg, off_usage = var_frame(p, cam, opts)
    print("usage:", usage, "segments:", seg, "without the option:", off_seg)
    TV.assert_same(rgb, place(ref_rgb, p), "rgb against the oracle")
    TV.assert_same(var, place(ref_var, p), "var against moments_ref")
    TV.assert_same(off_rgb, rgb, "rgb with the option off")
    TV.assert_same(off_var, var, "var with the option off")
    assert off_usage["sky_tiles"] == 0, off_usage
    # the segments are the same; the kernel counts no sphere or box test for its samples, which the main
    # launch tested against the scene before
    assert seg[0] == off_seg[0] and seg[0] >= w * abi.rows_of(p) * spp, (seg, off_seg)
    assert (seg[1:] < off_seg[1:]).all() if sky else np.array_equal(seg, off_seg), (seg, off_seg)
    if sky:
        assert_kernel_ran(usage)
    else:
        assert usage["sky_tiles"] == 0 and usage["pair_passes"] == 0, usage
    return rgb, usage


# ---- 1. the one-shot variance frame ----------------------------------------------------------------
_PLAIN = {}


@pytest.mark.parametrize("spp", [2, 3, 7, 16, 33])
@pytest.mark.parametrize("cam_name", ["reference", "corrected", "corrected-up"])
def test_one_shot_frame(cam_name, spp):
    """No full block (2, 3), a tail alone and blocks with a tail (7, 33), whole blocks (16). The
    corrected camera at its default position proves no tile sky: its plan must stay as it was."""
    n_sky = rt.tile_order(TV.scene("huge"), TV.params(W, H, spp), camera(cam_name))[2]
    assert n_sky == {"reference": SKY_TILES, "corrected": 0, "corrected-up": 16}[cam_name]
    rgb, usage = check_frame(cam_name, spp, sky=n_sky > 0)
    assert usage["sky_tiles"] == n_sky
    plain, _ = rt.render_f32(TV.scene("huge"), TV.params(W, H, spp), camera(cam_name))
    TV.assert_same(rgb, plain, "rgb against render_f32")


def test_the_synchronous_call_takes_the_process_default():
    p, cam = TV.params(W, H, 7), camera("reference")
    ref_rgb, ref_var, _ = reference("reference", W, H, 7)
    with rt.default_options_set(sky_moments=1):
        rgb, var, st = rt.render_var(TV.scene("huge"), p, cam)
    off_rgb, off_var, off_st = rt.render_var(TV.scene("huge"), p, cam)
    TV.assert_same(rgb, ref_rgb, "rgb")
    TV.assert_same(var, ref_var, "var")
    assert st.segments == off_st.segments and st.primaries == W * H * 7
    # that the default was picked up: the kernel tests its samples against nothing, so the call with the
    # option counts fewer sphere and box tests than the call without
    print("sphere tests:", st.sphere_tests, "against", off_st.sphere_tests, "box tests:", st.box_tests, "against", off_st.box_tests)
    assert 0 < st.sphere_tests < off_st.sphere_tests and 0 < st.box_tests < off_st.box_tests


# ---- 2. plans --------------------------------------------------------------------------------------
PLANS = {
    "four-passes": dict(max_pass_bytes=W * H * 12 * 4),
    "in-flight": dict(in_flight=True),
    "in-flight-four-passes": dict(in_flight=True, max_pass_bytes=W * H * 12 * 4),
    "one-stream": dict(render_streams=1),
    "one-stream-four-passes": dict(render_streams=1, max_pass_bytes=W * H * 12 * 4),
    "sky-serial": dict(sky_serial=True),
    "tile-classes": dict(tile_classes=1),
    "workspace-cap": TV.PAIRS_CAP,
}


@pytest.mark.parametrize("spp", [16, 33])
@pytest.mark.parametrize("plan", sorted(PLANS))
def test_plans(plan, spp):
    """16 samples, and 33: under passes of 4 the last pass then holds one sample, and the kernel's
    second slot row lies past that pass's own rows."""
    _, usage = check_frame("reference", spp, PLANS[plan])
    assert usage["sky_tiles"] == SKY_TILES
    if "four-passes" in plan:
        assert usage["pass_samples"] == 4, usage
    if "one-stream" in plan:
        assert usage["render_streams"] == 1, usage
    if plan == "workspace-cap":
        assert usage["pass_samples"] < 16 and usage["workspace_bytes"] <= TV.PAIRS_CAP["max_workspace_bytes"], usage


@pytest.mark.parametrize("case", ["brute-force", "no-sky", "60x36", "depth-0"])
def test_plans_without_sky_tiles_keep_the_main_launch(case):
    if case == "brute-force":
        check_frame("reference", 7, sky=False, brute_force=True)
    elif case == "no-sky":
        check_frame("reference", 7, dict(no_sky=True), sky=False)
    elif case == "60x36":  # no whole 64-pixel blocks: the natural order
        check_frame("reference", 7, w=60, sky=False)
    else:  # max_depth 0: every colour is 0, not the sky's
        p, cam = rt.make_params(W, H, 7, 0, SEED), camera("reference")
        rgb, var, _, usage = var_frame(p, cam, ON)
        assert usage["sky_tiles"] == 0 and not rgb.any() and not var.any()


# ---- 3. rows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["packed", "full-frame"])
def test_rows(layout):
    """Rows 1, 4, 7, ...: 12 rows, one row of tiles and 4 leftover rows; 6 of the 12 blocks are sky."""
    kw = dict(row_offset=1, row_stride=3, **(dict(full_frame=True) if layout == "full-frame" else {}))
    rgb, usage = check_frame("reference", 7, **kw)
    assert usage["sky_tiles"] == 6
    if layout == "full-frame":
        rest = np.ones(H, dtype=bool)
        rest[1::3] = False
        assert rgb.shape[0] == H and (rgb[rest] == F(TV.SENTINEL)).all()


# ---- 4. progressive --------------------------------------------------------------------------------
def estimates(cam_name, spp, windows):
    p = TV.params(W, H, spp)
    return [progressive_ref.place(e, p, TP.SENTINEL) for e in progressive_ref.run(reference(cam_name, W, H, spp)[2], windows, tau=TP.TAU)]


SCHEDULES = {"16": (16, (16,)), "8-8": (16, (8, 8)), "4-12": (16, (4, 12)), "4-4-4-4": (16, (4, 4, 4, 4)),
             "13-in-4-8-1": (13, (4, 8, 1)), "13-in-12-1": (13, (12, 1))}


@pytest.mark.parametrize("plan", ["default", "in-flight", "one-stream", "four-passes"])
@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_progressive_windows_back_to_back(schedule, plan):
    """Every window's resolve against progressive_ref, the last against the oracle; the steps are
    enqueued on a side stream with no host wait between them, so each window's kernel must wait for
    the step before it and each resolve for its window's kernel. Starts 4 and 12 are no multiples of
    the ring's depth."""
    import torch
    spp, windows = SCHEDULES[schedule]
    want = estimates("reference", spp, windows)
    p, cam = TV.params(W, H, spp), camera("reference")
    outs = [TP.Outs(p) for _ in windows]
    st = torch.cuda.Stream()
    opts = {} if plan == "default" else PLANS[plan]
    ds = rt.DeviceScene(TV.scene("huge"), device=0, options=rt.options(**dict(opts, **ON)))
    try:
        pg = ds.progressive(cam, p)
        usages = []
        for n, o in zip(windows, outs):
            pg.step(n, outputs=o.record(), stream=st.cuda_stream)
            usages.append(ds.usage())
        st.synchronize()
        assert pg.info()["done"] == spp
        pg.close()
    finally:
        ds.close()
    for u in usages:
        assert_kernel_ran(u, SKY_TILES)
    got = [o.read() for o in outs]
    for i, (g, r) in enumerate(zip(got, want)):
        TP.assert_estimate(g, r, f"window {i + 1} of {windows}")
    rgb, var, _ = reference("reference", W, H, spp)
    TV.assert_same(got[-1]["rgb"], rgb, "the last window's rgb against the oracle")
    TV.assert_same(got[-1]["var"], var, "the last window's var against the oracle")


def test_progressive_with_the_corrected_camera_looking_up():
    import torch
    want = estimates("corrected-up", 13, (4, 8, 1))
    p, cam = TV.params(W, H, 13), camera("corrected-up")
    ds = rt.DeviceScene(TV.scene("huge"), device=0, options=rt.options(**ON))
    try:
        got = TP.run_session(ds, cam, p, (4, 8, 1))
        assert_kernel_ran(ds.usage(), 16)
    finally:
        ds.close()
    for i, (g, r) in enumerate(zip(got, want)):
        TP.assert_estimate(g, r, f"window {i + 1}")


def test_two_sessions_a_plain_render_and_a_checkpoint_interleaved():
    """Two sessions (reference camera; the corrected one looking up, another seed) step by step on one
    scene, nothing waited for in between; a plain render and a one-shot variance render between two
    steps; the first session saved after its second window, destroyed, and loaded into a new session
    that finishes the frame."""
    import torch
    spp = 16
    cases = [("reference", SEED), ("corrected-up", SEED + 5)]
    ps = [TV.params(W, H, spp, seed) for _, seed in cases]
    cams = [camera(n) for n, _ in cases]
    s, m = TV.scene("huge")
    refs = [reference("reference", W, H, spp), moments_ref.render(s, m, cams[1], ps[1])]
    other = TP.samples_of("huge", W, H, spp, rt.REFERENCE, SEED + 9)
    st = torch.cuda.Stream()
    ds = rt.DeviceScene(TV.scene("huge"), device=0, options=rt.options(**ON))
    try:
        pgs = [ds.progressive(c, p) for c, p in zip(cams, ps)]
        outs = [TP.Outs(p) for p in ps]
        plain, varied = TP.Outs(ps[0]), TP.Outs(ps[0])
        po = TV.params(W, H, spp, SEED + 9)
        sky = []
        for i in range(4):
            pgs[0].step(4, outputs=outs[0].record(), stream=st.cuda_stream)
            sky.append(ds.usage()["sky_tiles"])
            if i == 1:
                ds.render(cams[0], po, plain.rgb.data_ptr(), st.cuda_stream)
                blob = pgs[0].save()  # (waits for the session's steps)
                pgs[0].close()
                pgs[0] = ds.progressive(cams[0], ps[0])
                pgs[0].load(blob)
                assert pgs[0].info()["done"] == 8
            pgs[1].step(4, outputs=outs[1].record(), stream=st.cuda_stream)
            sky.append(ds.usage()["sky_tiles"])
            if i == 2:
                ds.render_var(cams[0], po, varied.rgb.data_ptr(), varied.var.data_ptr(), st.cuda_stream)
                assert_kernel_ran(ds.usage(), SKY_TILES)
        st.synchronize()
        for pg in pgs:
            assert pg.info()["done"] == spp
            pg.close()
    finally:
        ds.close()
    assert sky == [SKY_TILES, 16] * 4, sky
    for o, (rgb, var, _) in zip(outs, refs):
        g = o.read()
        TV.assert_same(g["rgb"], rgb, "a session's rgb")
        TV.assert_same(g["var"], var, "a session's var")
    TV.assert_same(plain.read()["rgb"], other[0], "the plain render between")
    TV.assert_same(varied.read()["rgb"], other[0], "the variance render between: rgb")
    TV.assert_same(varied.read()["var"], other[1], "the variance render between: var")


# ---- 5. adaptive -----------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["default", "in-flight", "one-stream"])
def test_adaptive_steps_are_the_restatements(plan):
    """reference-tau0.25 (min_samples 4, windows 4-4-4-4): the sky blocks retire after the first window.
    Each step's sky_tiles is the number of proven-sky blocks the restatement renders in that step: 22
    in the first, none later, and the later steps still match."""
    case = "reference-tau0.25"
    scene_name, mode, tau, max_noisy = AC.CASES[case]
    p, cam = TV.params(W, H, AC.SPP), rt.Camera.default(W, H, mode)
    steps = adaptive_ref.run(AC.case_samples(case), AC.WINDOWS, tau, max_noisy, AC.MIN_SAMPLES)
    want = [adaptive_ref.place(e, p, TA.SENTINEL) for e in steps]
    perm, _, n_sky = rt.tile_order(TV.scene(scene_name), p, cam)
    sky_blocks = perm[len(perm) - n_sky:]
    counts = [np.zeros(AC.N_BLOCKS, dtype=np.int64)] + [np.asarray(r["d_b"]).astype(np.int64) for r in want]
    sky_rendered = [int(np.count_nonzero((b - a)[sky_blocks])) for a, b in zip(counts, counts[1:])]
    print("sky blocks rendered per step:", sky_rendered)
    assert sky_rendered[0] == SKY_TILES and sky_rendered[-1] == 0
    opts = {} if plan == "default" else PLANS[plan]
    ds = rt.DeviceScene(TV.scene(scene_name), device=0, options=rt.options(**dict(opts, **ON)))
    try:
        ad = ds.adaptive(cam, p, rt.adaptive_params(tau, max_noisy, AC.MIN_SAMPLES))
        got, usages = [], []
        for n in AC.WINDOWS:
            got += TA.run_adaptive(ds, cam, p, None, (n,), session=ad)
            usages.append(ds.usage())
        ad.close()
    finally:
        ds.close()
    for i, (g, r) in enumerate(zip(got, want)):
        TA.assert_step(g, r, f"step {i + 1}")
    assert tuple(g["info"]["active_blocks"] for g in got) == AC.ACTIVE[case]
    for i, (u, n) in enumerate(zip(usages, sky_rendered)):
        assert u["sky_tiles"] == n and u["pair_passes"] == 0, (i, u, n)


def test_adaptive_that_retires_nothing_is_the_progressive_session():
    """min_samples >= N: every step's outputs equal the progressive session's on the same scene, and
    every window of both runs the kernel."""
    import torch
    spp, windows = 16, (4, 4, 8)
    p, cam = TV.params(W, H, spp), camera("reference")
    ds = rt.DeviceScene(TV.scene("huge"), device=0, options=rt.options(**ON))
    try:
        ad = ds.adaptive(cam, p, rt.adaptive_params(0.1, 0, spp))
        got = []
        for n in windows:
            got += TA.run_adaptive(ds, cam, p, None, (n,), session=ad)
            assert_kernel_ran(ds.usage(), SKY_TILES)
        ad.close()
        pg, plain = ds.progressive(cam, p), []
        for n in windows:
            o = TA.Outs(p)
            pg.step(n, rgb_ptr=o.rgb.data_ptr(), variance_ptr=o.var.data_ptr(), rgb8_ptr=o.rgb8.data_ptr(),
                    noisy_ptr=o.noisy.data_ptr(), noise_tau=0.1)
            assert_kernel_ran(ds.usage(), SKY_TILES)
            torch.cuda.synchronize()
            plain.append(o.read())
        pg.close()
    finally:
        ds.close()
    for i, (g, q) in enumerate(zip(got, plain)):
        TV.assert_same(g["rgb"], q["rgb"], f"step {i + 1} rgb against the progressive session")
        TV.assert_same(g["var"], q["var"], f"step {i + 1} var against the progressive session")
        assert np.array_equal(g["rgb8"], q["rgb8"]) and g["noisy"] == q["noisy"]
    rgb, var, _ = reference("reference", W, H, spp)
    TV.assert_same(got[-1]["rgb"], rgb, "rgb against the oracle")
    TV.assert_same(got[-1]["var"], var, "var against the oracle")


# ---- 6. preview ------------------------------------------------------------------------------------
def test_preview_frames_and_a_refinement():
    """Three frames of the 1.5 degree orbit at 4 spp, then a 16-sample refinement in calls of 4, 4 and
    8, on a scene with the option and on one without: the same outputs; the completed refinement is
    rt.render_f32's frame."""
    import torch
    from test_tile_device_gpu import orbit
    pp = rt.preview_params(W, H, 4, max_depth=8, denoise=dict(levels=2))
    total, seed = 16, 5
    runs = {}
    for on in (1, 0):
        ds = rt.DeviceScene(TV.scene("huge"), device=0, options=rt.options(sky_moments=on))
        pv = ds.preview(pp)
        st = torch.cuda.Stream()
        rgb = torch.full((H, W, 3), TV.SENTINEL, dtype=torch.float32, device="cuda:0")
        rgb8 = torch.full((H, W, 3), 77, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        out, sky = [], []
        try:
            for i in range(3):
                pv.frame(orbit(W, H, i), 1 + i, rgb.data_ptr(), rgb8.data_ptr(), st.cuda_stream)
                sky.append(ds.usage()["sky_tiles"])
                st.synchronize()
                out.append((rgb.cpu().numpy(), rgb8.cpu().numpy()))
            for n in (4, 4, 8):
                pv.refine(orbit(W, H, 2), seed, total, n, rgb.data_ptr(), rgb8.data_ptr(), st.cuda_stream)
                sky.append(ds.usage()["sky_tiles"])
                st.synchronize()
                out.append((rgb.cpu().numpy(), rgb8.cpu().numpy()))
            assert pv.refine_info() == (total, total)
            pv.close()
        finally:
            ds.close()
        print("sky_moments", on, "sky tiles per call:", sky)
        assert all(n > 0 for n in sky) if on else not any(sky), sky
        runs[on] = out
    for i, ((a, a8), (b, b8)) in enumerate(zip(runs[1], runs[0])):
        TV.assert_same(a, b, f"call {i} rgb")
        assert np.array_equal(a8, b8), f"call {i} rgb8"
    exact, _ = rt.render_f32(TV.scene("huge"), rt.make_params(W, H, total, 8, seed), orbit(W, H, 2))
    TV.assert_same(runs[1][-1][0], exact, "the completed refinement against render_f32")


# ---- 7. scene update -------------------------------------------------------------------------------
def test_a_variance_frame_after_a_scene_update():
    """Every other small sphere moved by 0.3 along the ground (a sphere lifted above the others would
    leave no tile proven sky: the proof bounds the scene's height): the updated scene's variance frame
    equals a freshly created scene's, both with the option, and both still run the kernel."""
    s, m = TV.scene("huge")
    moved = s.copy()
    moved["center"][5::2] = moved["center"][5::2] + np.array((0.3, 0.0, 0.0), dtype=F)
    A, B = (s, m), (moved, m)
    p, cam = TV.params(W, H, 7), camera("reference")
    ds = rt.DeviceScene(A, device=0, options=rt.options(**ON))
    try:
        before = var_frame(p, cam, None, ds=ds)
        ds.update(B)
        after = var_frame(p, cam, None, ds=ds)
    finally:
        ds.close()
    fresh = var_frame(p, cam, ON, records=B)
    off = var_frame(p, cam, None, records=B)
    for u in (before[3], after[3], fresh[3]):
        assert_kernel_ran(u, SKY_TILES)
    assert int(np.count_nonzero(words(before[0]) != words(after[0]))) > 100  # (the update changed the picture)
    for i, what in enumerate(("rgb", "var")):
        TV.assert_same(after[i], fresh[i], f"{what} against a fresh scene")
        TV.assert_same(after[i], off[i], f"{what} against a fresh scene without the option")
    assert np.array_equal(after[2], fresh[2]) and after[2][0] == off[2][0]
    assert after[3]["sky_tiles"] == fresh[3]["sky_tiles"]
