"""The adaptive session's host side without a GPU (rt_adaptive_*): the restatement
(tests/tools/adaptive_ref.py) against the progressive session's restatement, the schedules of the
shared cases (tests/tools/adaptive_cases.py), the numpy twin of the compaction stage against a plain
loop, and every refusal that is decided before a device is touched, with its field named (each call
is given a null scene or a null session, so nothing touches HIP).
"""
import ctypes as C
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
from support import words as u32  # noqa: E402

F = np.float32
W, H = AC.W, AC.H


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(u32(a), u32(b))


# ---- the restatement -------------------------------------------------------------------------------
def test_blocks_of_the_natural_enumeration():
    """64 x 36: 32 tiles of 8 x 8 over rows 0..31, then 4 runs of 64 over rows 32..35."""
    b = adaptive_ref.block_of_pixels(36, 64)
    assert b.max() == 35 and (np.bincount(b.ravel()) == 64).all()
    assert b[0, 0] == 0 and b[7, 7] == 0 and b[0, 8] == 1 and b[8, 0] == 8 and b[31, 63] == 31
    assert (b[32] == 32).all() and (b[35] == 35).all()
    with pytest.raises(AssertionError):
        adaptive_ref.block_of_pixels(17, 30)


@pytest.mark.parametrize("spp,windows,min_samples", [(16, (4, 4, 4, 4), 16), (16, (8, 8), 20), (23, (4, 8, 11), 24)])
def test_nothing_retires_is_the_progressive_session(spp, windows, min_samples):
    """min_samples >= N: after every window the plain session's restatement, bit for bit."""
    samples = AC.samples_of("huge", W, H, spp, rt.REFERENCE)[2]
    tau = 0.25
    plain = progressive_ref.run(samples, windows, tau=tau)
    got = adaptive_ref.run(samples, windows, tau, 0, min_samples)
    for i, (g, p) in enumerate(zip(got, plain)):
        assert same(g["rgb"], p["rgb"]) and same(g["var"], p["var"]) and same(g["rgb8"], p["rgb8"]), i
        assert g["noisy"] == p["noisy"] and (g["samples"] == g["done"]).all()
        assert g["samples_rendered"] == W * H * g["done"]
        if g["done"] < min_samples:  # (at d_b = min_samples = N the rule may retire blocks: the frame is complete)
            assert g["active_blocks"] == AC.N_BLOCKS
    assert got[-1]["finished"] and not got[-2]["finished"]


@pytest.mark.parametrize("case", sorted(AC.CASES))
def test_schedule_and_prefixes(case):
    """The blocks still active after every step; A never grows; every pixel's estimate is the plain
    session's after d_b samples of its block."""
    _, _, tau, max_noisy = AC.CASES[case]
    samples = AC.case_samples(case)
    steps = adaptive_ref.run(samples, AC.WINDOWS, tau, max_noisy, AC.MIN_SAMPLES)
    active = tuple(e["active_blocks"] for e in steps)
    print(case, "active after each step:", active, "done:", [e["done"] for e in steps], "noisy:", [e["noisy"] for e in steps])
    assert active == AC.ACTIVE[case]
    assert int((steps[-1]["d_b"] == AC.SPP).sum()) == AC.AT_CAP[case]
    prev = np.ones(AC.N_BLOCKS, dtype=bool)
    for e in steps:
        assert not (e["active"] & ~prev).any(), "A grew"
        prev = e["active"]
    plain = {d: est for d, est in zip((4, 8, 12, 16), progressive_ref.run(samples, AC.WINDOWS))}
    block = adaptive_ref.block_of_pixels(H, W)
    for e in steps:
        assert set(np.unique(e["d_b"])) <= set(plain) and (e["d_b"] <= e["done"]).all()
        for d, est in plain.items():
            px = e["d_b"][block] == d
            assert np.array_equal(u32(e["rgb"])[px], u32(est["rgb"])[px])
            assert np.array_equal(u32(e["var"])[px], u32(est["var"])[px])
            assert np.array_equal(e["rgb8"][px], est["rgb8"][px])
        assert e["samples_rendered"] == 64 * int(e["d_b"].sum()) and (e["samples"] == e["d_b"][block]).all()


def test_the_cases_cover_what_they_are_chosen_for():
    """Asserted on the restatement alone: retirements at two or more distinct steps in one case, a block
    that reaches N in one case, a case finished before N."""
    runs = {c: adaptive_ref.run(AC.case_samples(c), AC.WINDOWS, AC.CASES[c][2], AC.CASES[c][3], AC.MIN_SAMPLES) for c in AC.CASES}

    def retiring_steps(steps):
        counts = (AC.N_BLOCKS,) + tuple(e["active_blocks"] for e in steps)
        return sum(1 for a, b in zip(counts, counts[1:]) if b < a)
    assert any(retiring_steps(s) >= 2 for s in runs.values())
    assert any((s[-1]["d_b"] == AC.SPP).any() for s in runs.values())
    assert any(s[-1]["finished"] and s[-1]["done"] < AC.SPP for s in runs.values())
    # a step after the session finished renders nothing and resolves to the same bits
    early = runs["reference-tau0.25-noisy2"]
    assert early[2]["finished"] and early[3]["done"] == 12 and same(early[3]["rgb"], early[2]["rgb"])
    assert early[3]["samples_rendered"] == early[2]["samples_rendered"]


# ---- the compaction stage's twin -------------------------------------------------------------------
@pytest.mark.parametrize("n,split", [(1, (1, 0, 0)), (65, (0, 65, 0)), (300, (100, 0, 200)), (1025, (400, 600, 25))])
def test_compact_twin_against_a_plain_loop(n, split):
    rng = np.random.default_rng(n)
    src = rng.permutation(n).astype(np.uint32)
    for active in (np.ones(n, np.uint32), np.zeros(n, np.uint32), (np.arange(n) & 1).astype(np.uint32),
                   rng.integers(0, 2, n).astype(np.uint32) * 7):
        out, counts = adaptive_ref.compact(src, split, active)
        want, cls = [], [0, 0, 0]
        for i, b in enumerate(src):
            if active[b]:
                want.append(int(b))
                cls[0 if i < split[0] else 1 if i < split[0] + split[1] else 2] += 1
        assert out.tolist() == want and counts.tolist() == [len(want)] + cls


# ---- refusals decided before a device is touched ---------------------------------------------------
def test_record_sizes():
    assert C.sizeof(abi.RtAdaptiveParams) == 16 and C.sizeof(abi.RtAdaptiveOutputs) == 48 and C.sizeof(abi.RtAdaptiveInfo) == 48


def good():
    return rt.make_params(W, H, 16, 64, AC.SEED), rt.Camera.default(W, H), rt.adaptive_params(0.25, 0, 4)


@pytest.mark.parametrize("field,change", [
    ("size", dict(size=12)), ("max_noisy", dict(max_noisy=64)), ("min_samples", dict(min_samples=6)),
    ("min_samples", dict(min_samples=0)), ("noise_tau", dict(noise_tau=-0.5)), ("noise_tau", dict(noise_tau=float("nan"))),
    ("noise_tau", dict(noise_tau=float("inf")))], ids=lambda v: v if isinstance(v, str) else "-".join(f"{k}={x}" for k, x in v.items()))
def test_create_refuses_a_bad_adaptive_record_first(field, change):
    """With a null scene AND bad params: the adaptive record is what the message names."""
    p, cam, a = good()
    p.spp = 1
    for k, v in change.items():
        setattr(a, k, v)
    with pytest.raises(rt.RtError) as e:
        rt.Adaptive(None, cam, p, a)
    assert e.value.status == abi.RT_ERR_INVALID and f"adaptive.{field}" in str(e.value), str(e.value)


def test_create_names_its_null_arguments_and_refuses_params_before_the_scene():
    p, cam, a = good()
    for args, name in (((None, cam, p, None), "adaptive"), ((None, cam, None, a), "params"), ((None, None, p, a), "camera"),
                       ((None, cam, p, a), "scene")):
        with pytest.raises(rt.RtError) as e:
            rt.Adaptive(*args)
        assert e.value.status == abi.RT_ERR_INVALID and name in str(e.value), str(e.value)
    assert rt.lib().rt_adaptive_create(None, C.byref(cam.c), C.byref(p), C.byref(a), None) == abi.RT_ERR_INVALID
    p.spp = 1
    with pytest.raises(rt.RtError) as e:
        rt.Adaptive(None, cam, p, a)
    assert e.value.status == abi.RT_ERR_INVALID and "spp" in str(e.value)
    p = rt.make_params(W, H, 16, 64, AC.SEED, fast_math=True)
    with pytest.raises(rt.RtError) as e:
        rt.Adaptive(None, cam, p, a)
    assert e.value.status == abi.RT_ERR_UNSUPPORTED and "RT_FLAG_FAST_MATH" in str(e.value)


def test_a_pixel_count_that_is_no_multiple_of_64_is_unsupported():
    a = rt.adaptive_params(0.25)
    with pytest.raises(rt.RtError) as e:
        rt.Adaptive(None, rt.Camera.default(30, 17), rt.make_params(30, 17, 16, 64, AC.SEED), a)
    assert e.value.status == abi.RT_ERR_UNSUPPORTED and "64" in str(e.value), str(e.value)


@pytest.mark.parametrize("field,fields", [
    ("out.size", dict(size=40)), ("out.variance", dict(rgb=256, variance=256)), ("out.rgb8", dict(rgb=256, rgb8=256)),
    ("out.samples", dict(variance=512, samples=512)), ("out.noisy", dict(samples=1024, noisy=1024))],
    ids=["size", "variance-is-rgb", "rgb8-is-rgb", "samples-is-variance", "noisy-is-samples"])
def test_step_refuses_its_outputs_record_before_the_session(field, fields):
    o = rt.adaptive_outputs()
    for k, v in fields.items():
        setattr(o, k, v)
    assert rt.lib().rt_adaptive_step_device(None, 4, C.byref(o), None, None) == abi.RT_ERR_INVALID
    msg = rt.lib().rt_last_error().decode()
    assert f" {field} " in msg.replace(":", " ") + " ", msg
    assert "null session" not in msg


def test_null_session_arguments():
    L = rt.lib()
    o = rt.adaptive_outputs(rgb_ptr=256, variance_ptr=512, rgb8_ptr=768, samples_ptr=1024, noisy_ptr=1280)
    info, words = abi.RtAdaptiveInfo(), (C.c_uint32 * 4)()
    for rc in (L.rt_adaptive_step_device(None, 4, C.byref(o), None, None), L.rt_adaptive_step_device(None, 4, None, None, None),
               L.rt_adaptive_info(None, C.byref(info)), L.rt_adaptive_blocks(None, words, 4), L.rt_adaptive_reset(None, None, None),
               L.rt_adaptive_destroy(None)):
        assert rc == abi.RT_ERR_INVALID and b"null session" in L.rt_last_error()


@pytest.mark.parametrize("name,args", [
    ("d_src_perm", (0, 4, (1, 2, 1), 256, 512, 768)), ("class_counts", (128, 4, None, 256, 512, 768)),
    ("d_active", (128, 4, (1, 2, 1), 0, 512, 768)), ("d_out_perm", (128, 4, (1, 2, 1), 256, 0, 768)),
    ("d_counts", (128, 4, (1, 2, 1), 256, 512, 0)), ("n_blocks", (128, 0, (0, 0, 0), 256, 512, 768)),
    ("n_blocks", (128, (1 << 26) + 1, (0, (1 << 26) + 1, 0), 256, 512, 768)), ("class_counts", (128, 4, (1, 2, 2), 256, 512, 768)),
    ("d_out_perm", (128, 4, (1, 2, 1), 256, 128, 768))])
def test_the_stage_call_names_its_bad_argument(name, args):
    with pytest.raises(rt.RtError) as e:
        rt.block_compact_device(*args)
    assert e.value.status == abi.RT_ERR_INVALID and name in str(e.value), str(e.value)
