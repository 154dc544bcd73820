"""The progressive session's host side without a GPU (rt_progressive_*): the
restatement (tests/tools/progressive_ref.py) against the CPU oracle's frame, what its intermediate
estimates look like, and every refusal that is decided before a device is touched, with its field
named: the Step rule (rt_progressive_window), the outputs record of a step (checked before the
session), creation (params before the scene) and a checkpoint's header (rt_progressive_blob_check,
the check rt_progressive_load makes).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import moments_ref  # noqa: E402
import progressive_ref  # noqa: E402
from support import assert_bits, words as u32  # noqa: E402

F = np.float32
SEED = 1234
W, H = 64, 36
_FRAMES = {}


def frame(w, h, spp):
    """moments_ref's (rgb, var, samples) of the huge scene's frame, once."""
    key = (w, h, spp)
    if key not in _FRAMES:
        s, m = rt.huge_scene_arrays(SEED)
        _FRAMES[key] = moments_ref.render(s, m, rt.Camera.default(w, h), rt.make_params(w, h, spp, 64, SEED))
    return _FRAMES[key]


# ---- the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,spp,windows", [(64, 36, 16, (4, 4, 4, 4)), (64, 36, 16, (8, 8)), (64, 36, 16, (4, 12)),
                                             (64, 36, 16, (16,)), (64, 36, 23, (4, 8, 11)), (30, 17, 7, (4, 3)),
                                             (30, 17, 7, (7,))])
def test_the_last_window_is_the_oracles_frame(w, h, spp, windows):
    rgb, var, samples = frame(w, h, spp)
    last = progressive_ref.run(samples, windows)[-1]
    for name, got, ref in (("rgb", last["rgb"], rgb), ("var", last["var"], var)):
        bad = int(np.count_nonzero(u32(got) != u32(ref)))
        print(name, "mismatching values:", bad, "of", ref.size)
        assert got.shape == ref.shape and bad == 0, name


def test_a_prefix_is_not_the_frame():
    """The estimate after 4 of 16 samples differs from the final frame in thousands of values: a session
    that rendered everything at once cannot pass the intermediate checks of the GPU tests."""
    rgb, var, samples = frame(W, H, 16)
    first = progressive_ref.run(samples, (4,))[0]
    n_rgb = int(np.count_nonzero(u32(first["rgb"]) != u32(rgb)))
    n_var = int(np.count_nonzero(u32(first["var"]) != u32(var)))
    print("after 4 of 16:", n_rgb, "of", rgb.size, "rgb values and", n_var, "of", var.size, "variances differ")
    assert n_rgb > 2000 and n_var > 1000


def test_the_prefix_is_not_a_shorter_frame_either():
    """The keys are the 16-sample frame's: its first 4 samples are not the 4-sample frame's."""
    _, _, samples = frame(W, H, 16)
    rgb4, _, _ = frame(W, H, 4)
    first = progressive_ref.run(samples, (4,))[0]
    assert int(np.count_nonzero(u32(first["rgb"]) != u32(rgb4))) > 2000


def test_carried_moments_are_the_prefixes_variance():
    """The moments carried window by window against moments_ref.variance over each whole prefix."""
    _, _, samples = frame(W, H, 23)
    for est, d in zip(progressive_ref.run(samples, (4, 8, 11)), (4, 12, 23)):
        assert_bits(est["var"], moments_ref.variance(samples[:, :, :d]), d)


def test_noise_count_of_the_restatement():
    _, _, samples = frame(W, H, 16)
    counts = [e["noisy"] for e in progressive_ref.run(samples, (4, 4, 4, 4), tau=0.1)]
    print("noisy after 4, 8, 12, 16 samples:", counts, "of", W * H)
    assert counts == [149, 131, 78, 50]


def test_texel_of_the_restatement_is_the_goldens():
    """64 x 36 x 4 in one window: the committed frame and its texels."""
    import golden_io as G
    _, _, samples = frame(W, H, 4)
    est = progressive_ref.run(samples, (4,))[0]
    gold = np.fromfile(os.path.join(G.GOLDEN, "huge_64x36_s4.f32"), dtype=F).reshape(H, W, 3)
    gold8 = np.fromfile(os.path.join(G.GOLDEN, "huge_64x36_s4.u8"), dtype=np.uint8).reshape(H, W, 3)
    assert_bits(est["rgb"], gold)
    assert np.array_equal(est["rgb8"], gold8)


# ---- the Step rule ---------------------------------------------------------------------------------
def test_window_rule():
    assert rt.progressive_window(16, 0, 4) == 4 and rt.progressive_window(16, 8, 8) == 8
    assert rt.progressive_window(16, 12, 100) == 4 and rt.progressive_window(16, 16, 4) == 0
    assert rt.progressive_window(16, 4, 0) == 0
    # the tail arrives with the last window; a window that reaches the end may have any size
    assert rt.progressive_window(23, 12, 11) == 11 and rt.progressive_window(23, 20, 3) == 3
    assert rt.progressive_window(23, 20, 5) == 3 and rt.progressive_window(3, 0, 3) == 3 and rt.progressive_window(2, 0, 7) == 2
    for spp, done, n in ((16, 0, 3), (16, 4, 6), (23, 20, 2), (23, 0, 22), (7, 0, 5)):
        with pytest.raises(rt.RtError) as e:
            rt.progressive_window(spp, done, n)
        assert e.value.status == abi.RT_ERR_INVALID and "n_samples" in str(e.value), str(e.value)
        with pytest.raises(ValueError):
            progressive_ref.window(spp, done, n)
    for spp, done in ((16, 2), (16, 17), (23, 21)):
        with pytest.raises(rt.RtError) as e:
            rt.progressive_window(spp, done, 4)
        assert e.value.status == abi.RT_ERR_INVALID and "done" in str(e.value)
    with pytest.raises(rt.RtError) as e:
        rt.progressive_window(1, 0, 4)
    assert e.value.status == abi.RT_ERR_INVALID and "spp" in str(e.value)
    assert rt.lib().rt_progressive_window(16, 0, 4, None) == abi.RT_ERR_INVALID


# ---- creation and the null session -----------------------------------------------------------------
def test_record_sizes():
    assert C.sizeof(abi.RtProgressiveOutputs) == 40 and C.sizeof(abi.RtProgressiveInfo) == 40


CREATE_REFUSED = [
    ("spp", dict(spp=1), abi.RT_ERR_INVALID), ("width", dict(width=0), abi.RT_ERR_INVALID),
    ("rows", dict(row_offset=30, num_rows=10), abi.RT_ERR_INVALID), ("flag", dict(flags=1 << 9), abi.RT_ERR_INVALID),
    ("RT_FLAG_FAST_MATH", dict(flags=abi.RT_FLAG_FAST_MATH), abi.RT_ERR_UNSUPPORTED),
    ("RT_FLAG_SCALAR_SCENE", dict(flags=abi.RT_FLAG_SCALAR_SCENE), abi.RT_ERR_UNSUPPORTED),
    ("RT_FLAG_WAVEFRONT", dict(flags=abi.RT_FLAG_WAVEFRONT), abi.RT_ERR_UNSUPPORTED),
    ("RT_FLAG_CUDA_COMPAT", dict(flags=abi.RT_FLAG_CUDA_COMPAT), abi.RT_ERR_UNSUPPORTED),
    ("no rows", dict(row_offset=36), abi.RT_ERR_INVALID),
]


@pytest.mark.parametrize("name,change,status", CREATE_REFUSED, ids=[c[0].replace(" ", "-") for c in CREATE_REFUSED])
def test_create_refuses_as_the_variance_render_does(name, change, status):
    p = rt.make_params(W, H, 16, 64, SEED)
    for k, v in change.items():
        setattr(p, k, v)
    with pytest.raises(rt.RtError) as e:
        rt.Progressive(None, rt.Camera.default(W, H), p)
    assert e.value.status == status and name in str(e.value), str(e.value)


def test_create_names_its_null_arguments():
    p, cam = rt.make_params(W, H, 16, 64, SEED), rt.Camera.default(W, H)
    for args, name in (((None, cam, None), "params"), ((None, None, p), "camera"), ((None, cam, p), "scene")):
        with pytest.raises(rt.RtError) as e:
            rt.Progressive(*args)
        assert e.value.status == abi.RT_ERR_INVALID and name in str(e.value), str(e.value)


def test_null_session_arguments():
    L = rt.lib()
    info = abi.RtProgressiveInfo()
    assert L.rt_progressive_step_device(None, 4, None, None, None) == abi.RT_ERR_INVALID
    assert b"null session" in L.rt_last_error()
    assert L.rt_progressive_info(None, C.byref(info)) == abi.RT_ERR_INVALID
    assert L.rt_progressive_reset(None, None, None) == abi.RT_ERR_INVALID
    assert L.rt_progressive_save(None, None, 0) == abi.RT_ERR_INVALID
    assert L.rt_progressive_load(None, None, 0) == abi.RT_ERR_INVALID
    assert L.rt_progressive_destroy(None) == abi.RT_ERR_INVALID


OUT_REFUSED = [
    ("out.size", dict(size=36)), ("out", dict()), ("out.variance", dict(rgb=256, variance=256)),
    ("out.rgb8", dict(rgb=256, rgb8=256)), ("out.rgb8", dict(variance=512, rgb8=512)), ("out.noisy", dict(rgb=256, noisy=256)),
    ("out.noisy", dict(variance=256, rgb8=512, noisy=512)),
    ("out.noise_tau", dict(noisy=256, noise_tau=-1.0)), ("out.noise_tau", dict(noisy=256, noise_tau=float("nan"))),
    ("out.noise_tau", dict(rgb=512, noisy=256, noise_tau=float("inf"))),
]


@pytest.mark.parametrize("field,fields", OUT_REFUSED, ids=[f"{i}-{f}" for i, (f, _) in enumerate(OUT_REFUSED)])
def test_step_refuses_its_outputs_record_before_the_session(field, fields):
    """Wrong size, nothing asked for, aliased outputs, a bad threshold (the record is checked first,
    so a null session shows the refusal without a device)."""
    o = rt.progressive_outputs()
    for k, v in fields.items():
        setattr(o, k, v)
    assert rt.lib().rt_progressive_step_device(None, 4, C.byref(o), None, None) == abi.RT_ERR_INVALID
    msg = rt.lib().rt_last_error().decode()
    assert f" {field} " in msg.replace(":", " ") + " ", msg
    assert "null session" not in msg


def test_a_good_outputs_record_gets_as_far_as_the_session():
    o = rt.progressive_outputs(rgb_ptr=256, variance_ptr=512, rgb8_ptr=768, noisy_ptr=1024, noise_tau=0.1)
    assert rt.lib().rt_progressive_step_device(None, 4, C.byref(o), None, None) == abi.RT_ERR_INVALID
    assert b"null session" in rt.lib().rt_last_error()


# ---- checkpoints -----------------------------------------------------------------------------------
class Header(C.Structure):
    """The head of a checkpoint as this build writes it (the blob is opaque to callers; the test
    builds one by hand to show each refusal without a device)."""
    _fields_ = [("magic", C.c_uint64), ("version", C.c_uint32), ("layout", C.c_uint32), ("params", abi.RtParams),
                ("camera", abi.RtCamera), ("n_pixels", C.c_uint64), ("done", C.c_uint32), ("reserved", C.c_uint32)]


def blob(p, cam, at, **changes):
    h = Header(int.from_bytes(b"RQTPROG1", "little"), 2, 0x33383301, p, cam.c, p.width * abi.rows_of(p), at, 0)
    for k, v in changes.items():
        obj = h
        *head, last = k.split("__")
        for n in head:
            obj = getattr(obj, n)
        setattr(obj, last, v)
    return bytes(h) + bytes(2 * 12 * p.width * abi.rows_of(p))


def test_blob_check_accepts_the_sessions_own():
    p, cam = rt.make_params(W, H, 16, 64, SEED), rt.Camera.default(W, H)
    assert C.sizeof(Header) == 128
    info = rt.progressive_blob_check(blob(p, cam, 8), p, cam)
    assert info == dict(done=8, spp=16, n_pixels=W * H, state_bytes=128 + 24 * W * H, device_bytes=24 * W * H)
    q = rt.make_params(W, H, 23, 64, SEED, row_offset=1, row_stride=3)
    assert rt.progressive_blob_check(blob(q, cam, 23), q, cam)["n_pixels"] == W * 12


BLOB_REFUSED = [
    ("magic", dict(magic=0x1234)), ("version", dict(version=3)), ("layout", dict(layout=7)),
    ("params.width", dict(params__width=W + 1)), ("params.height", dict(params__height=H + 1)), ("params.spp", dict(params__spp=20)),
    ("params.max_depth", dict(params__max_depth=8)), ("params.seed", dict(params__seed=SEED + (1 << 40))),
    ("params.row_offset", dict(params__row_offset=1)), ("params.row_stride", dict(params__row_stride=2)),
    ("params.num_rows", dict(params__num_rows=3)), ("params.flags", dict(params__flags=abi.RT_FLAG_BRUTE_FORCE)),
    ("camera", dict(camera__lens_radius=0.5)), ("camera", dict(camera__mode=1)), ("n_pixels", dict(n_pixels=5)),
    ("done", dict(done=6)), ("done", dict(done=20)),
]


@pytest.mark.parametrize("field,changes", BLOB_REFUSED, ids=[f"{i}-{f}" for i, (f, _) in enumerate(BLOB_REFUSED)])
def test_blob_check_refuses_a_foreign_or_mismatching_header(field, changes):
    p, cam = rt.make_params(W, H, 16, 64, SEED), rt.Camera.default(W, H)
    with pytest.raises(rt.RtError) as e:
        rt.progressive_blob_check(blob(p, cam, 8, **changes), p, cam)
    assert e.value.status == abi.RT_ERR_INVALID, str(e.value)
    assert f" {field} " in str(e.value).replace(":", " ") + " ", str(e.value)


def test_blob_check_refuses_a_truncated_blob():
    p, cam = rt.make_params(W, H, 16, 64, SEED), rt.Camera.default(W, H)
    good = blob(p, cam, 8)
    for cut in (0, 64, 127, 128, len(good) - 1):
        with pytest.raises(rt.RtError) as e:
            rt.progressive_blob_check(good[:cut], p, cam)
        assert e.value.status == (abi.RT_ERR_INVALID if cut == 0 else abi.RT_ERR_CAPACITY), (cut, str(e.value))
    assert rt.progressive_blob_check(good + b"more", p, cam)["done"] == 8
