"""CPU-side checks of the first-hit feature buffers (rt_render_aov / rt_render_aov_device,
DESIGN.md §4.8): the record's layout, the argument validation (decided before any HIP call, so
none of it needs a device) and the CPU reference tool the GPU tests compare against
(tests/tools/aov_ref.cpp), itself held to the restatement's beauty image.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle_binding as O
import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import aov_ref  # noqa: E402
from support import assert_bits, words as u32  # noqa: E402


def bubble_camera(mode):
    """From the centre of the simple scene's glass ball (sphere 3, radius 1, with the hollow
    sphere 4 of radius -0.99 inside it): every primary ray leaves through sphere 4's far root."""
    return rt.Camera((-2, 1, 0), (0, 1, 0), (0, 1, 0), 2.0, 90.0, .0625, 1.0, mode)


# ---- ABI ---------------------------------------------------------------------------------
def test_record_layout():
    assert C.sizeof(abi.RtAovBuffers) == 8 + 5 * C.sizeof(C.c_void_p)
    rec = rt.render.aov_buffers({"depth": 4096})
    assert rec.size == C.sizeof(abi.RtAovBuffers) and rec.samples == 0
    assert rec.depth == 4096 and not rec.albedo and not rec.normal and not rec.alpha and not rec.sphere_id
    with pytest.raises(KeyError):
        rt.render.aov_buffers({"beauty": 4096})


def _host_call(params, rec, camera=None):
    """rt_render_aov on the simple scene with the record as given: (status, message)."""
    s, m = rt.simple_scene_arrays()
    cam = camera if camera is not None else rt.Camera.default(params.width, params.height).c
    rc = rt.lib().rt_render_aov(abi.ptr(s, C.POINTER(abi.RtSphere)), len(s), abi.ptr(m, C.POINTER(abi.RtMaterial)), len(m),
                                C.byref(cam), C.byref(params) if params is not None else None,
                                C.byref(rec) if rec is not None else None, None)
    return rc, rt.lib().rt_last_error().decode()


def _record(samples=0, **planes):
    # (addresses that no call reaches: every case below fails before any HIP call)
    return rt.render.aov_buffers(planes or {"albedo": 4096, "sphere_id": 8192}, samples)


def test_invalid_arguments():
    p = rt.make_params(16, 8, 4)
    rc, msg = _host_call(p, None)
    assert rc == abi.RT_ERR_INVALID and "null aov" in msg
    bad = _record()
    bad.size -= 8
    rc, msg = _host_call(p, bad)
    assert rc == abi.RT_ERR_INVALID and "sizeof(rt_aov_buffers)" in msg
    rc, msg = _host_call(p, _record(samples=5))
    assert rc == abi.RT_ERR_INVALID and "exceed spp" in msg
    none = abi.RtAovBuffers(C.sizeof(abi.RtAovBuffers), 0)
    rc, msg = _host_call(p, none)
    assert rc == abi.RT_ERR_INVALID and "no plane" in msg
    # the existing check_params failures
    for q, text in ((rt.make_params(0, 8, 4), "must be > 0"), (rt.make_params(16, 8, 0), "must be > 0"),
                    (rt.make_params(16, 8, 4, row_offset=5, num_rows=6), "rows exceed"),
                    (rt.make_params(1 << 16, 1 << 16, 1, num_rows=1), "2^32")):
        rc, msg = _host_call(q, _record(), camera=rt.Camera.default(16, 8).c)
        assert rc == abi.RT_ERR_INVALID and text in msg, (rc, msg)
    q = rt.make_params(16, 8, 4)
    q.flags |= 1 << 20
    rc, msg = _host_call(q, _record())
    assert rc == abi.RT_ERR_INVALID and "unknown flag" in msg
    rc, msg = _host_call(None, _record(), camera=rt.Camera.default(16, 8).c)
    assert rc == abi.RT_ERR_INVALID and "params: null" in msg


@pytest.mark.parametrize("field,name", [("fast_math", "RT_FLAG_FAST_MATH"), ("scalar_scene", "RT_FLAG_SCALAR_SCENE"),
                                        ("wavefront", "RT_FLAG_WAVEFRONT"), ("cuda_compat", "RT_FLAG_CUDA_COMPAT")])
def test_unsupported_flags_are_named(field, name):
    rc, msg = _host_call(rt.make_params(16, 8, 4, **{field: True}), _record())
    assert rc == abi.RT_ERR_UNSUPPORTED and name in msg, (rc, msg)


def test_device_entry_validates_before_the_scene():
    p = rt.make_params(16, 8, 4)
    cam = rt.Camera.default(16, 8).c
    f = rt.lib().rt_render_aov_device
    assert f(None, C.byref(cam), C.byref(p), None, None) == abi.RT_ERR_INVALID
    assert "null aov" in rt.lib().rt_last_error().decode()
    rec = _record(samples=9)
    assert f(None, C.byref(cam), C.byref(p), C.byref(rec), None) == abi.RT_ERR_INVALID
    assert "exceed spp" in rt.lib().rt_last_error().decode()
    q = rt.make_params(16, 8, 4, wavefront=True)
    rec = _record()
    assert f(None, C.byref(cam), C.byref(q), C.byref(rec), None) == abi.RT_ERR_UNSUPPORTED
    assert "RT_FLAG_WAVEFRONT" in rt.lib().rt_last_error().decode()
    assert f(None, C.byref(cam), C.byref(p), C.byref(rec), None) == abi.RT_ERR_INVALID  # a null scene
    assert "null argument" in rt.lib().rt_last_error().decode()


# ---- the reference tool ----------------------------------------------------------------------
def test_reference_miss_albedo_is_the_beauty():
    """A pixel whose samples all miss: its albedo is the beauty pixel, bit for bit (every sample is
    the sky's colour under an attenuation of 1, summed and divided alike)."""
    s, m = rt.huge_scene_arrays(1234)
    W, H, spp = 64, 36, 4
    p = rt.make_params(W, H, spp, 64, 1234)
    cam = O.camera_default(W, H, 0)
    ref = aov_ref.render(s, m, cam, p)
    beauty, _ = O.render_f32(s, m, cam, p)
    miss = ref["alpha"] == 0
    assert int(miss.sum()) >= 1000
    assert np.array_equal(u32(ref["albedo"])[miss], u32(beauty)[miss])
    # and such a pixel has no normal, no depth and no sphere
    assert not u32(ref["normal"])[miss].any() and not u32(ref["depth"])[miss].any()
    assert (ref["sphere_id"][miss] == 0xffffffff).all()
    # a covered pixel's planes are its hit's: alpha in (0, 1] in steps of 1 / spp, depth > 0
    hit = ~miss
    assert np.isin(ref["alpha"][hit], np.arange(1, spp + 1, dtype=np.float32) / np.float32(spp)).all()
    assert (ref["depth"][hit] > 0).all()


@pytest.mark.parametrize("mode", [rt.REFERENCE, rt.CORRECTED])
def test_reference_bubble_camera(mode):
    s, m = rt.simple_scene_arrays()
    assert s["radius"][4] == np.float32(-0.99)
    W, H, spp = 64, 32, 4
    ref = aov_ref.render(s, m, bubble_camera(mode), rt.make_params(W, H, spp, 64, 1234), sample_ids=True)
    assert ref["sample_ids"].shape == (H, W, spp)
    assert (ref["sample_ids"] == 4).all()
    assert (ref["sphere_id"] == 4).all() and (ref["alpha"] == 1).all()
    # the glass material's albedo (1, 1, 1), summed and averaged exactly
    assert (ref["albedo"] == 1).all()
    # a negative radius flips the normal: it points back at the camera inside the ball, towards the centre
    assert (ref["depth"] > 0).all() and np.isfinite(ref["normal"]).all()


def test_reference_rows_and_sample_prefix():
    """Row fields and samples < spp: the planes of a strided pass are the matching rows of the whole
    pass, and samples keyed over the frame's spp differ from a frame of that many samples."""
    s, m = rt.huge_scene_arrays(1234)
    W, H = 64, 36
    cam = O.camera_default(W, H, 0)
    whole = aov_ref.render(s, m, cam, rt.make_params(W, H, 4, 64, 1234))
    part = aov_ref.render(s, m, cam, rt.make_params(W, H, 4, 64, 1234, row_offset=1, row_stride=2))
    full = aov_ref.render(s, m, cam, rt.make_params(W, H, 4, 64, 1234, row_offset=1, row_stride=2, full_frame=True))
    for n in abi.AOV_PLANES:
        assert_bits(part[n], whole[n][1::2], n)
        assert_bits(full[n][1::2], whole[n][1::2], n)
        assert (full[n][0::2] == abi.AOV_PLANES[n][2]).all(), n
    pre = aov_ref.render(s, m, cam, rt.make_params(W, H, 8, 64, 1234), samples=3)
    own = aov_ref.render(s, m, cam, rt.make_params(W, H, 3, 64, 1234))
    assert not np.array_equal(u32(pre["albedo"]), u32(own["albedo"]))
