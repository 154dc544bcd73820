"""The preview session's host side without a GPU (rt_preview_*): record sizes and
defaults, every refusal of rt_preview_create with its field named (creation is called with a null
scene, and the params are checked before the scene is looked at, so no device is touched), and the
restatement's own composition (tests/tools/preview_ref.py).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import denoise_var_ref  # noqa: E402
import preview_ref  # noqa: E402
import temporal_ref  # noqa: E402

F = np.float32
W, H = 64, 36


def test_record_sizes_and_defaults():
    assert C.sizeof(abi.RtPreviewParams) == 96 and C.sizeof(abi.RtPreviewPlanes) == 120
    p = rt.preview_params(W, H, 8)
    assert (p.size, p.width, p.height, p.spp, p.max_depth) == (96, W, H, 8, 64)
    assert p.flags & ~(abi.RT_PREVIEW_DEMODULATE | abi.RT_PREVIEW_FEEDBACK) == 0
    dp, dv = rt.denoise_var_params(W, H)
    assert bytes(p.temporal) == bytes(rt.temporal_params(W, H)) and bytes(p.denoise) == bytes(dp)
    assert p.var_floor == dv.var_floor
    assert (preview_ref.DEMODULATE, preview_ref.FEEDBACK, preview_ref.NO_TEMPORAL) == \
        (abi.RT_PREVIEW_DEMODULATE, abi.RT_PREVIEW_FEEDBACK, abi.RT_PREVIEW_NO_TEMPORAL)
    for bad in ((0, H, 4), (W, 0, 4), (W, H, 1)):
        with pytest.raises(rt.RtError) as e:
            rt.preview_params(*bad)
        assert e.value.status == abi.RT_ERR_INVALID


def test_params_builder_sets_flags_and_sub_records():
    p = rt.preview_params(W, H, 4, demodulate=True, feedback=True, temporal=dict(alpha_min=0.2), denoise=dict(levels=3),
                          max_depth=8)
    assert p.flags == abi.RT_PREVIEW_DEMODULATE | abi.RT_PREVIEW_FEEDBACK
    assert p.temporal.alpha_min == F(0.2) and p.denoise.levels == 3 and p.max_depth == 8
    q = rt.preview_params(70, 37, 4, base=p, feedback=False, temporal=False)
    assert q.flags == abi.RT_PREVIEW_DEMODULATE | abi.RT_PREVIEW_NO_TEMPORAL
    assert (q.width, q.temporal.width, q.denoise.width, q.height, q.temporal.height, q.denoise.height) == (70, 70, 70, 37, 37, 37)
    assert q.denoise.levels == 3
    with pytest.raises(KeyError):
        rt.preview_params(W, H, 4, size=3)


def _set(path, value):
    def change(p):
        obj = p
        *head, last = path.split(".")
        for n in head:
            obj = getattr(obj, n)
        setattr(obj, last, value)
    return change


REFUSED = [
    ("size", _set("size", 92)), ("width", _set("width", 0)), ("width", _set("width", 65537)),
    ("height", _set("height", 0)), ("height", _set("height", 65537)),
    ("spp", _set("spp", 1)), ("spp", _set("spp", 0)), ("max_depth", _set("max_depth", 0)),
    ("flags", _set("flags", 8)), ("flags", _set("flags", 1 << 31)),
    ("flags", _set("flags", abi.RT_PREVIEW_FEEDBACK | abi.RT_PREVIEW_NO_TEMPORAL)),
    ("var_floor", _set("var_floor", 0.0)), ("var_floor", _set("var_floor", -1.0)), ("var_floor", _set("var_floor", float("inf"))),
    ("var_floor", _set("var_floor", float("nan"))),
    ("temporal.size", _set("temporal.size", 28)), ("temporal.width", _set("temporal.width", W + 1)),
    ("temporal.height", _set("temporal.height", H - 1)),
    ("temporal.alpha_min", _set("temporal.alpha_min", 0.0)), ("temporal.alpha_min", _set("temporal.alpha_min", 1.5)),
    ("temporal.max_history", _set("temporal.max_history", 0.5)), ("temporal.normal_tol", _set("temporal.normal_tol", -1.0)),
    ("temporal.depth_tol", _set("temporal.depth_tol", float("nan"))), ("temporal.flags", _set("temporal.flags", 1)),
    ("denoise.size", _set("denoise.size", 40)), ("denoise.width", _set("denoise.width", W - 1)),
    ("denoise.height", _set("denoise.height", H + 1)),
    ("denoise.levels", _set("denoise.levels", 0)), ("denoise.levels", _set("denoise.levels", 7)),
    ("denoise.sigma_color", _set("denoise.sigma_color", -1.0)), ("denoise.sigma_color", _set("denoise.sigma_color", 1e-30)),
    ("denoise.sigma_normal", _set("denoise.sigma_normal", 0.0)), ("denoise.sigma_normal", _set("denoise.sigma_normal", 1e-30)),
    ("denoise.sigma_depth", _set("denoise.sigma_depth", 0.0)), ("denoise.sigma_depth", _set("denoise.sigma_depth", float("inf"))),
    ("denoise.sigma_albedo", _set("denoise.sigma_albedo", float("nan"))),
    ("denoise.flags", _set("denoise.flags", abi.RT_DENOISE_DEMODULATE)),
    ("denoise.flags", _set("denoise.flags", abi.RT_DENOISE_DEMODULATE | abi.RT_DENOISE_DIRECT)),
    ("denoise.flags", _set("denoise.flags", 4)),
]


@pytest.mark.parametrize("field,change", REFUSED, ids=[f"{i}-{f}" for i, (f, _) in enumerate(REFUSED)])
def test_create_refuses_with_the_field_named(field, change):
    p = rt.preview_params(W, H, 4)
    change(p)
    with pytest.raises(rt.RtError) as e:
        rt.Preview(None, p)
    assert e.value.status == abi.RT_ERR_INVALID, str(e.value)
    # the field's name stands alone: "width" must not be found in "temporal.width"
    assert f" {field} " in str(e.value).replace(":", " ") + " ", str(e.value)


def test_create_accepts_direct_and_names_the_null_scene():
    """A valid record (RT_DENOISE_DIRECT in denoise.flags included) gets as far as the scene."""
    for p in (rt.preview_params(W, H, 4), rt.preview_params(W, H, 2, denoise=dict(direct=True), demodulate=True, feedback=True),
              rt.preview_params(W, H, 4, temporal=False, denoise=dict(sigma_color=0.0, sigma_albedo=0.0))):
        with pytest.raises(rt.RtError) as e:
            rt.Preview(None, p)
        assert e.value.status == abi.RT_ERR_INVALID and "scene" in str(e.value)
    h = C.c_void_p()
    assert rt.lib().rt_preview_create(None, None, C.byref(h)) == abi.RT_ERR_INVALID and not h.value


def test_null_session_arguments():
    L = rt.lib()
    cam = rt.Camera.default(W, H, rt.CORRECTED)
    n = C.c_uint64(0)
    assert L.rt_preview_frame_device(None, C.byref(cam.c), 1, None, None, None) == abi.RT_ERR_INVALID
    assert L.rt_preview_reset(None) == abi.RT_ERR_INVALID
    assert L.rt_preview_planes(None, None) == abi.RT_ERR_INVALID
    assert L.rt_preview_usage(None, C.byref(n)) == abi.RT_ERR_INVALID
    L.rt_preview_destroy(None)
    for args, name in (((0, H, 16, 16, 16, 16, 16), "width"), ((W, H, 16, 0, 16, 16, 16), "variance"),
                       ((W, H, 16, 16, 16, 16, 0), "variance_out")):
        with pytest.raises(rt.RtError) as e:
            rt.preview_split_device(*args)
        assert e.value.status == abi.RT_ERR_INVALID and name in str(e.value)
    for args, name in (((W, 1 << 17, 16, None, 16, None), "height"), ((W, H, 0, None, 16, None), "filtered"),
                       ((W, H, 16, 16, None, None), "d_rgb8")):
        with pytest.raises(rt.RtError) as e:
            rt.preview_merge_device(*args)
        assert e.value.status == abi.RT_ERR_INVALID and name in str(e.value)


def _planes(seed, w=23, h=9):
    g = np.random.default_rng(seed)
    ids = np.array([0, 1, 0xffffffff], dtype=np.uint32)[g.integers(0, 3, (h, w))]
    return dict(beauty=g.random((h, w, 3), dtype=F), variance=g.random((h, w), dtype=F) * F(0.02),
                albedo=g.random((h, w, 3), dtype=F), normal=np.array([[0, 1, 0], [1, 0, 0]], dtype=F)[g.integers(0, 2, (h, w))],
                depth=g.uniform(5, 6, (h, w)).astype(F), alpha=(ids != 0xffffffff).astype(F), sphere_id=ids)


def test_restatement_with_the_flags_off_is_the_two_stages_composed():
    w, h = 23, 9
    p = rt.preview_params(w, h, 4, flags=0)
    cam = rt.Camera.default(w, h, rt.CORRECTED)
    s = preview_ref.Session(p)
    prev = None
    kept = 0
    for seed in (1, 2):
        cur = _planes(seed, w, h)
        r = s.frame(cur, cam)
        tcur = {n: cur[n] for n in ("beauty", "variance", "normal", "depth", "alpha", "sphere_id")}
        c, v, n, reason = temporal_ref.accumulate(tcur, prev, cam, cam, p.temporal)
        dp, dv = rt.denoise_var_params(w, h)
        want = denoise_var_ref.denoise(c, v, cur["albedo"], cur["normal"], cur["depth"], **denoise_var_ref.params_kwargs(dp, dv))[0]
        for a, b in ((r["out"], want), (r["color"], c), (r["variance"], v), (r["history"], n)):
            assert a.dtype == F and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        prev = dict(color=c, variance=v, history=n, normal=cur["normal"], depth=cur["depth"], sphere_id=cur["sphere_id"])
        kept += int((reason == temporal_ref.KEPT).sum())
    assert kept > w * h // 8  # the second frame did reproject the first


def test_restatement_split_and_merge():
    cur = _planes(3)
    cur["albedo"][0, 0] = (0.001, 0.5, 0.5)
    cur["beauty"][0, 0] = cur["albedo"][0, 0]
    i, v = preview_ref.split(cur["beauty"], cur["variance"], cur["albedo"])
    assert i[0, 0, 0] == F(0.001) * F(128) and i[0, 0, 1] == 1 and i[0, 0, 2] == 1
    la = (F(0.2126) * F(0.0078125) + F(0.7152) * F(0.5)) + F(0.0722) * F(0.5)
    assert v[0, 0] == cur["variance"][0, 0] / (la * la)
    back = preview_ref.merge(i, cur["albedo"])
    assert np.array_equal(back[0, 0], cur["beauty"][0, 0])  # x / 2^-7 * 2^-7 and 1 * a are exact
    assert np.allclose(back, cur["beauty"], rtol=3e-7, atol=0)  # two roundings
    assert np.array_equal(preview_ref.merge(i).view(np.uint32), i.view(np.uint32))
    # feedback with one level: the fed-back image is the frame's output
    p = rt.preview_params(23, 9, 4, flags=abi.RT_PREVIEW_FEEDBACK, denoise=dict(levels=1))
    s = preview_ref.Session(p)
    r = s.frame(cur, rt.Camera.default(23, 9, rt.CORRECTED))
    assert np.array_equal(r["out"].view(np.uint32), s.prev["color"].view(np.uint32))
