"""The adaptive session on the GPU (rt_adaptive_*): after every step the outputs, the
noise count, the blocks' sample counts and the session's report against the CPU restatement
(tests/tools/adaptive_ref.py over the per-sample colours of tests/tools/moments_ref.py), and the
compaction kernel alone against numpy.

Every comparison is on uint32 (or uint8) views with zero mismatches allowed, against outputs filled
with sentinels. The references are computed once per module and shared (tests/tools/adaptive_cases.py).
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
import progressive_ref  # noqa: E402
import test_variance_gpu as TV  # noqa: E402
from motion_cases import huge_a_b  # noqa: E402
from support import assert_all_bits  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, SEED = AC.W, AC.H, AC.SPP, AC.SEED
SENTINEL = dict(rgb=F(-7.0), var=F(-7.0), rgb8=np.uint8(77), samples=np.uint32(0x2BCD1234))
PLANES = ("rgb", "var", "rgb8", "samples")


class Outs:
    """One set of a step's outputs on the device, filled with sentinels."""

    def __init__(self, p):
        import torch
        rows = p.height if p.flags & abi.RT_FLAG_FULL_FRAME else abi.rows_of(p)
        dev = "cuda:0"
        self.rgb = torch.full((rows, p.width, 3), float(SENTINEL["rgb"]), dtype=torch.float32, device=dev)
        self.var = torch.full((rows, p.width), float(SENTINEL["var"]), dtype=torch.float32, device=dev)
        self.rgb8 = torch.full((rows, p.width, 3), int(SENTINEL["rgb8"]), dtype=torch.uint8, device=dev)
        self.samples = torch.full((rows, p.width), int(SENTINEL["samples"]), dtype=torch.int32, device=dev)
        self.noisy = torch.full((1,), 12345, dtype=torch.int32, device=dev)
        self.seg = torch.zeros((3,), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

    def record(self):
        return rt.adaptive_outputs(self.rgb.data_ptr(), self.var.data_ptr(), self.rgb8.data_ptr(), self.samples.data_ptr(),
                                   self.noisy.data_ptr())

    def read(self):
        return dict(rgb=self.rgb.cpu().numpy(), var=self.var.cpu().numpy(), rgb8=self.rgb8.cpu().numpy(),
                    samples=self.samples.cpu().numpy().view(np.uint32), noisy=int(self.noisy.cpu().numpy()[0]),
                    segments=int(self.seg.cpu().numpy()[0]))


def run_adaptive(ds, cam, p, ap, windows, session=None):
    """A session's outputs, block counts and report after each step, read back after each step."""
    import torch
    ad = session or ds.adaptive(cam, p, ap)
    got = []
    try:
        for n in windows:
            o = Outs(p)
            ad.step(n, outputs=o.record(), segments=o.seg.data_ptr())
            torch.cuda.synchronize()
            g = o.read()
            g["d_b"] = ad.blocks()
            g["info"] = ad.info()
            got.append(g)
    finally:
        if session is None:
            ad.close()
    return got


def assert_step(g, r, what):
    assert_all_bits(g, r, what, PLANES)
    print(what, "noisy:", g["noisy"], "expected", r["noisy"], "active:", g["info"]["active_blocks"], "expected", r["active_blocks"])
    assert g["noisy"] == r["noisy"], f"{what}: noise count"
    assert np.array_equal(g["d_b"], r["d_b"]), f"{what}: rt_adaptive_blocks"
    i = g["info"]
    assert (i["active_blocks"], i["samples_rendered"], bool(i["finished"]), i["done"]) == \
        (r["active_blocks"], r["samples_rendered"], r["finished"], r["done"]), f"{what}: info {i}"


def check_case(case, opts=None, windows=AC.WINDOWS, w=W, h=H, **kw):
    """The case's session under the scene options `opts` and params `kw` against the restatement after
    every step; the steps are returned."""
    scene_name, mode, tau, max_noisy = AC.CASES[case]
    samples = AC.samples_of(scene_name, w, h, SPP, mode, **kw)[2]
    p = TV.params(w, h, SPP, SEED, **kw)
    want = [adaptive_ref.place(e, p, SENTINEL) for e in adaptive_ref.run(samples, windows, tau, max_noisy, AC.MIN_SAMPLES)]
    ds = rt.DeviceScene(TV.scene(scene_name), device=0, options=rt.options(**opts) if opts else None)
    try:
        got = run_adaptive(ds, rt.Camera.default(w, h, mode), p, rt.adaptive_params(tau, max_noisy, AC.MIN_SAMPLES), windows)
    finally:
        ds.close()
    for i, (g, r) in enumerate(zip(got, want)):
        assert_step(g, r, f"{case} step {i + 1}")
    return got


# ---- every step is the restatement's ---------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(AC.CASES))
def test_every_step_is_the_restatements(case):
    got = check_case(case)
    assert tuple(g["info"]["active_blocks"] for g in got) == AC.ACTIVE[case]
    info = got[-1]["info"]
    assert info["n_blocks"] == AC.N_BLOCKS and info["n_pixels"] == W * H and info["spp"] == SPP
    assert info["device_bytes"] == 24 * W * H + 16 * AC.N_BLOCKS + 16


# ---- nothing retires: the exact frame --------------------------------------------------------------
@pytest.mark.parametrize("spp,windows,min_samples", [(16, (4, 4, 4, 4), 16), (23, (4, 8, 11), 24)], ids=["16-in-4-4-4-4", "23-in-4-8-11"])
def test_nothing_retires_is_the_exact_frame(spp, windows, min_samples):
    """min_samples >= N: every step equals the plain progressive session's outputs on the device, the
    last one rt.render_var and rt.render_f32 (23 spp: the tail of 3 arrives with the last window)."""
    import torch
    p, cam = TV.params(W, H, spp), rt.Camera.default(W, H)
    ds = rt.DeviceScene(TV.scene("huge"), device=0)
    try:
        got = run_adaptive(ds, cam, p, rt.adaptive_params(0.1, 0, min_samples), windows)
        pg, plain = ds.progressive(cam, p), []
        for n in windows:
            o = Outs(p)
            pg.step(n, rgb_ptr=o.rgb.data_ptr(), variance_ptr=o.var.data_ptr(), rgb8_ptr=o.rgb8.data_ptr(),
                    noisy_ptr=o.noisy.data_ptr(), noise_tau=0.1)
            torch.cuda.synchronize()
            plain.append(o.read())
        pg.close()
    finally:
        ds.close()
    done = 0
    for i, (g, q) in enumerate(zip(got, plain)):
        done += progressive_ref.window(spp, done, windows[i])
        TV.assert_same(g["rgb"], q["rgb"], f"step {i + 1} rgb against the plain session")
        TV.assert_same(g["var"], q["var"], f"step {i + 1} var against the plain session")
        assert np.array_equal(g["rgb8"], q["rgb8"]) and g["noisy"] == q["noisy"]
        assert (g["samples"] == done).all() and (g["d_b"] == done).all()
        if done < spp:
            assert g["info"]["active_blocks"] == AC.N_BLOCKS and not g["info"]["finished"]
    assert got[-1]["info"]["finished"] and got[-1]["info"]["samples_rendered"] == W * H * spp
    rgb, var, _ = rt.render_var(TV.scene("huge"), p, cam)
    flat, _ = rt.render_f32(TV.scene("huge"), p, cam)
    TV.assert_same(got[-1]["rgb"], rgb, "rgb against render_var")
    TV.assert_same(got[-1]["var"], var, "var against render_var")
    TV.assert_same(got[-1]["rgb"], flat, "rgb against render_f32")


# ---- retired pixels are not traced -----------------------------------------------------------------
def test_retired_pixels_are_not_traced():
    """The oracle tool gives no per-pixel segment counts, so: the first window (every block active)
    traces exactly the plain session's segments; every later window of a session that has retired
    blocks traces strictly fewer than the plain session's same window, and at least one segment per
    sample it renders; the samples rendered, as rt_adaptive_info reports them, are the restatement's."""
    import torch
    case = "reference-tau0.25"
    scene_name, mode, tau, max_noisy = AC.CASES[case]
    p, cam = TV.params(W, H, SPP), rt.Camera.default(W, H, mode)
    want = adaptive_ref.run(AC.case_samples(case), AC.WINDOWS, tau, max_noisy, AC.MIN_SAMPLES)
    ds = rt.DeviceScene(TV.scene(scene_name), device=0)
    try:
        got = run_adaptive(ds, cam, p, rt.adaptive_params(tau, max_noisy, AC.MIN_SAMPLES), AC.WINDOWS)
        pg, plain = ds.progressive(cam, p), []
        for n in AC.WINDOWS:
            seg = torch.zeros((3,), dtype=torch.int64, device="cuda:0")
            pg.step(n, segments=seg.data_ptr())
            torch.cuda.synchronize()
            plain.append(int(seg.cpu().numpy()[0]))
        pg.close()
    finally:
        ds.close()
    rendered_before = 0
    for i, (g, r, q) in enumerate(zip(got, want, plain)):
        rendered = g["info"]["samples_rendered"] - rendered_before
        rendered_before = g["info"]["samples_rendered"]
        print(f"window {i + 1}: adaptive segments {g['segments']}, plain {q}, samples rendered {rendered}")
        assert g["info"]["samples_rendered"] == r["samples_rendered"]
        assert g["segments"] >= rendered
        if i == 0:
            assert g["segments"] == q and rendered == W * H * 4
        else:
            assert 0 < g["segments"] < q and rendered < W * H * 4


# ---- plans -----------------------------------------------------------------------------------------
# (a pass holds at least 4 samples, so a 4-sample window is one pass whatever max_pass_bytes says: under
# `small-passes` the schedule runs once more in windows of 8, each cut into two passes of 4 over the
# window's active list)
PLANS = {
    "in-flight": (dict(in_flight=True), {}),
    "one-stream": (dict(render_streams=1), {}),
    "deep-split-0": (dict(deep_split=0), {}),
    "deep-split-2": (dict(deep_split=2, deep_min_items=0), {}),
    "small-passes": (dict(max_pass_bytes=64 * 12 * 4), {}),
    "brute-force": (None, dict(brute_force=True)),
}


@pytest.mark.parametrize("plan", sorted(PLANS))
def test_plans_give_the_same_bits(plan):
    opts, kw = PLANS[plan]
    got = check_case("reference-tau0.25", opts, **kw)
    assert tuple(g["info"]["active_blocks"] for g in got) == AC.ACTIVE["reference-tau0.25"]
    if plan == "small-passes":
        got = check_case("reference-tau0.25", opts, windows=(8, 8))
        assert got[0]["info"]["active_blocks"] < AC.N_BLOCKS and got[1]["info"]["done"] == SPP


# ---- rows ------------------------------------------------------------------------------------------
def test_a_row_share_in_the_full_frame_layout():
    """Rows 1, 3, 5, ... of a 64 x 72 frame (36 rows): the rows not rendered keep their sentinels."""
    got = check_case("reference-tau0.25", h=72, row_offset=1, row_stride=2, full_frame=True)
    last = got[-1]
    assert last["rgb"].shape[0] == 72 and last["info"]["n_blocks"] == 36
    for name in PLANES:
        assert (last[name][0::2] == SENTINEL[name]).all(), name
    assert len(set(last["d_b"].tolist())) > 1, "the share's schedule retires nothing: the test shows nothing"


def test_blocks_that_are_not_whole_are_refused():
    ds = rt.DeviceScene(TV.scene("huge"), device=0)
    try:
        with pytest.raises(rt.RtError) as e:
            ds.adaptive(rt.Camera.default(30, 17), TV.params(30, 17, SPP), rt.adaptive_params(0.25))
        assert e.value.status == abi.RT_ERR_UNSUPPORTED
    finally:
        ds.close()


# ---- independence ----------------------------------------------------------------------------------
def test_sessions_and_renders_interleaved_do_not_disturb_each_other():
    """An adaptive session, a plain session with another camera and seed, and a plain render between
    their steps, on one scene: each gives what it gives alone."""
    import torch
    case = "reference-tau0.25"
    scene_name, mode, tau, max_noisy = AC.CASES[case]
    want = adaptive_ref.run(AC.case_samples(case), AC.WINDOWS, tau, max_noisy, AC.MIN_SAMPLES)
    p, cam = TV.params(W, H, SPP), rt.Camera.default(W, H, mode)
    p2, cam2 = TV.params(W, H, SPP, SEED + 5), rt.Camera.default(W, H, rt.CORRECTED)
    plain_want = progressive_ref.run(AC.samples_of("huge", W, H, SPP, rt.CORRECTED, SEED + 5)[2], AC.WINDOWS, tau=0.1)
    p3 = TV.params(W, H, SPP, SEED + 9)
    frame_want = AC.samples_of("huge", W, H, SPP, rt.REFERENCE, SEED + 9)[0]
    ds = rt.DeviceScene(TV.scene(scene_name), device=0)
    try:
        ad, pg = ds.adaptive(cam, p, rt.adaptive_params(tau, max_noisy, AC.MIN_SAMPLES)), ds.progressive(cam2, p2)
        got, plain, frames = [], [], []
        for n in AC.WINDOWS:
            got += run_adaptive(ds, cam, p, None, (n,), session=ad)
            o = Outs(p2)
            pg.step(n, rgb_ptr=o.rgb.data_ptr(), variance_ptr=o.var.data_ptr(), rgb8_ptr=o.rgb8.data_ptr(),
                    noisy_ptr=o.noisy.data_ptr(), noise_tau=0.1)
            f = Outs(p3)
            ds.render(cam, p3, f.rgb.data_ptr())
            torch.cuda.synchronize()
            plain.append(o.read())
            frames.append(f.read()["rgb"])
        ad.close()
        pg.close()
    finally:
        ds.close()
    for i, (g, r) in enumerate(zip(got, want)):
        assert_step(g, r, f"adaptive step {i + 1}")
    for i, (g, r) in enumerate(zip(plain, plain_want)):
        TV.assert_same(g["rgb"], r["rgb"], f"plain session step {i + 1} rgb")
        TV.assert_same(g["var"], r["var"], f"plain session step {i + 1} var")
        assert g["noisy"] == r["noisy"]
    for f in frames:
        TV.assert_same(f, frame_want, "the plain render between")


# ---- reset and scene updates -----------------------------------------------------------------------
def test_reset_starts_the_schedule_again_with_the_same_bits():
    case = "reference-tau0.25"
    scene_name, mode, tau, max_noisy = AC.CASES[case]
    want = adaptive_ref.run(AC.case_samples(case), AC.WINDOWS, tau, max_noisy, AC.MIN_SAMPLES)
    p, cam = TV.params(W, H, SPP), rt.Camera.default(W, H, mode)
    ds = rt.DeviceScene(TV.scene(scene_name), device=0)
    try:
        ad = ds.adaptive(cam, p, rt.adaptive_params(tau, max_noisy, AC.MIN_SAMPLES))
        first = run_adaptive(ds, cam, p, None, AC.WINDOWS[:3], session=ad)
        ad.reset()
        i = ad.info()
        assert (i["done"], i["active_blocks"], i["samples_rendered"], i["finished"]) == (0, AC.N_BLOCKS, 0, 0)
        assert not ad.blocks().any()
        again = run_adaptive(ds, cam, p, None, AC.WINDOWS, session=ad)
        ad.close()
    finally:
        ds.close()
    for i, (g, r) in enumerate(zip(first, want)):
        assert_step(g, r, f"before reset, step {i + 1}")
    for i, (g, r) in enumerate(zip(again, want)):
        assert_step(g, r, f"after reset, step {i + 1}")


def test_a_scene_update_is_refused_until_reset():
    a, b = huge_a_b()
    p, cam, tau = TV.params(W, H, 8), rt.Camera.default(W, H), 0.25
    import moments_ref
    samples = moments_ref.render(b[0], b[1], cam, p)[2]
    want = adaptive_ref.run(samples, (4, 4), tau, 0, 4)
    ds = rt.DeviceScene(a, device=0)
    try:
        ad = ds.adaptive(cam, p, rt.adaptive_params(tau, 0, 4))
        ad.step(4)
        ds.update(b)
        with pytest.raises(rt.RtError) as e:
            ad.step(4)
        assert e.value.status == abi.RT_ERR_INVALID and "updated" in str(e.value)
        assert ad.info()["done"] == 4
        ad.reset()
        got = run_adaptive(ds, cam, p, None, (4, 4), session=ad)
        ad.close()
    finally:
        ds.close()
    for i, (g, r) in enumerate(zip(got, want)):
        assert_step(g, r, f"on the updated scene, step {i + 1}")


# ---- the compaction kernel alone -------------------------------------------------------------------
def splits_of(n):
    """Class splits of n entries: an empty first, middle and last class among them."""
    a, b = n // 3, n // 2
    return [(0, b, n - b), (a, 0, n - a), (a, n - a, 0), (a, b - a, n - b), (n, 0, 0), (0, 0, n)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 3000])
def test_the_compaction_kernel_alone(n):
    """One lane, the wave edges, the chunk edges and three chunks; flags all set, none set, alternating
    and seeded random: the four counts and every output entry; entries past the kept ones keep their
    sentinel."""
    import torch
    rng = np.random.default_rng(n)
    src = rng.permutation(n).astype(np.uint32)
    flags = [np.ones(n, np.uint32), np.zeros(n, np.uint32), (np.arange(n) & 1).astype(np.uint32),
             (rng.integers(0, 2, n) * rng.integers(1, 1 << 31, n)).astype(np.uint32)]
    d_src = torch.from_numpy(src.view(np.int32)).to("cuda:0")
    for split in splits_of(n):
        for k, active in enumerate(flags):
            d_act = torch.from_numpy(active.view(np.int32)).to("cuda:0")
            d_out = torch.full((n,), 0x5EADBEEF, dtype=torch.int32, device="cuda:0")
            d_cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            rt.block_compact_device(d_src.data_ptr(), n, split, d_act.data_ptr(), d_out.data_ptr(), d_cnt.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            out, cnt = d_out.cpu().numpy().view(np.uint32), d_cnt.cpu().numpy().view(np.uint32)
            want, counts = adaptive_ref.compact(src, split, active)
            assert cnt.tolist() == counts.tolist(), (n, split, k)
            kept = int(counts[0])
            assert np.array_equal(out[:kept], want), (n, split, k)
            assert (out[kept:] == 0x5EADBEEF).all(), (n, split, k)
