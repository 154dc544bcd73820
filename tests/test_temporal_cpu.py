"""Temporal accumulation without a GPU (rt_temporal*, rt_reproject_basis): the
records, the projection record against its numpy restatement (tests/tools/temporal_ref.py), the
restatement's projection against float64 geometry, properties of the restatement, and every
argument check (all made before any device call).
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import temporal_ref  # noqa: E402
from support import assert_bits, words as u32  # noqa: E402

F = np.float32


# ---- records -------------------------------------------------------------------------------------
def test_record_sizes_and_default_record():
    assert C.sizeof(abi.RtTemporalParams) == 32 and C.sizeof(abi.RtTemporalBuffers) == 128
    assert [n for n, _ in abi.RtTemporalBuffers._fields_[1:]] == list(abi.TEMPORAL_PLANES)
    L = rt.lib()
    p = abi.RtTemporalParams()
    assert L.rt_temporal_params_default(640, 360, C.byref(p)) == abi.RT_OK
    assert (p.size, p.width, p.height, p.flags) == (32, 640, 360, 0)
    # the defaults lie in the ranges the checks accept (their values are not pinned)
    assert 0 < p.alpha_min <= 1 and p.max_history >= 1 and p.normal_tol >= 0 and p.depth_tol >= 0
    assert all(np.isfinite(v) for v in (p.alpha_min, p.max_history, p.normal_tol, p.depth_tol))
    rc, msg = _call(False)
    assert rc != abi.RT_ERR_INVALID, msg  # (RT_ERR_DEVICE without a GPU: the checks all passed)
    assert L.rt_temporal_params_default(0, 360, C.byref(p)) == abi.RT_ERR_INVALID
    assert L.rt_temporal_params_default(640, 0, C.byref(p)) == abi.RT_ERR_INVALID
    assert L.rt_temporal_params_default(640, 360, None) == abi.RT_ERR_INVALID
    q = rt.temporal_params(8, 4, alpha_min=0.5, max_history=4.0)
    assert (q.width, q.height, q.alpha_min, q.max_history, q.depth_tol) == (8, 4, 0.5, 4.0, p.depth_tol)
    assert rt.temporal_params(9, 5, base=q).alpha_min == 0.5
    with pytest.raises(KeyError):
        rt.temporal_params(8, 4, alpha=1)
    with pytest.raises(KeyError):
        rt.temporal_buffers({"color": 1})


# ---- the projection record ------------------------------------------------------------------------
CUSTOM = ((1, 2, 3), (0, 0, -1), (0, 1, 0), 1.5, 60.0, 0.5, 2.0)  # test_camera_init_custom's
CAMERAS = {
    "default-reference": lambda: rt.Camera.default(64, 36, rt.REFERENCE),
    "default-corrected": lambda: rt.Camera.default(64, 36, rt.CORRECTED),
    "custom": lambda: rt.Camera(*CUSTOM, rt.CORRECTED),
    "cuda": lambda: rt.Camera.cuda(1280, 720),
}


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_reproject_basis_is_the_restatement_bit_for_bit(name):
    cam = CAMERAS[name]()
    got, ref = rt.reproject_basis(cam), temporal_ref.basis(cam)
    assert got.dtype == np.float32 and got.shape == (12,) and np.isfinite(got).all()
    assert_bits(got, ref, (got, ref))
    assert np.array_equal(got[9:], np.array(cam.c.origin, dtype=F))


def test_reproject_basis_refuses_a_degenerate_camera():
    cam = rt.Camera.default(64, 36, rt.CORRECTED)
    bad = abi.RtCamera.from_buffer_copy(bytes(cam.c))
    bad.vertical[:] = (0.0, 1.0, 0.0)
    bad.horizontal[:] = (0.0, 2.0, 0.0)  # parallel to vertical: D = 0 exactly
    with pytest.raises(rt.RtError) as e:
        rt.reproject_basis(bad)
    assert e.value.status == abi.RT_ERR_INVALID and "prev_camera" in str(e.value)
    assert temporal_ref.basis(bad) is None
    nan = abi.RtCamera.from_buffer_copy(bytes(cam.c))
    nan.origin[1] = float("nan")
    with pytest.raises(rt.RtError) as e:
        rt.reproject_basis(nan)
    assert e.value.status == abi.RT_ERR_INVALID and "prev_camera" in str(e.value)
    assert rt.lib().rt_reproject_basis(None, None) == abi.RT_ERR_INVALID


def test_projection_of_the_restatement_against_float64_geometry():
    """400 random points in front of a corrected pinhole camera: px and py of temporal_ref.project
    (float32, the Cramer form over the camera record) against the perspective projection formed in
    float64 from the camera's construction arguments (position, look-at, up, field of view), which
    shares nothing with the record. Observed maximum on the CPU when written: 7.2e-5 pixels (the
    record itself is float32: a relative 2^-24 of a basis entry moves a pixel coordinate of ~10^2 by
    ~10^-5, and a dozen such roundings add up); the bound is 4 times that."""
    W, H = 320, 180
    pos, look, up, vfov = np.array([1.0, 2.0, 3.0]), np.array([0.0, 0.0, -1.0]), np.array([0.0, 1.0, 0.0]), 50.0
    aspect = W / H
    cam = rt.Camera(tuple(pos), tuple(look), tuple(up), aspect, vfov, 0.0, float(np.linalg.norm(pos - look)), rt.CORRECTED)
    record = temporal_ref.basis(cam)
    w = (pos - look) / np.linalg.norm(pos - look)
    u = np.cross(up, w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    half_h = math.tan(math.radians(vfov) / 2)
    half_w = half_h * aspect
    g = np.random.default_rng(7)
    # points in the view frustum, 0.5 .. 30 units along the view direction
    z = g.uniform(0.5, 30.0, 400)
    sx, sy = g.uniform(-0.98, 0.98, 400), g.uniform(-0.98, 0.98, 400)
    pts = pos + (sx * half_w * z)[:, None] * u + (sy * half_h * z)[:, None] * v - z[:, None] * w
    want_x = (sx + 1) / 2 * W - 0.5
    want_y = (1 - (sy + 1) / 2) * H - 0.5
    q = pts.astype(F) - record[9:12]
    ga, px, py = temporal_ref.project(q, record, W, H)
    assert (ga > 0).all()
    err = max(np.abs(px - want_x).max(), np.abs(py - want_y).max())
    print(f"largest difference from the float64 projection: {err:.3e} pixels")
    assert err < 2.9e-4  # 4 x 7.2e-5


# ---- properties of the restatement -----------------------------------------------------------------
def _planes(w, h, seed):
    """A current and a previous frame of seeded random planes that agree in their guides (a surface
    everywhere, depth taken from a plane facing the camera so that a static camera reprojects every
    pixel onto itself)."""
    g = np.random.default_rng(seed)
    cam = rt.Camera.default(w, h, rt.CORRECTED)
    normal = np.zeros((h, w, 3), dtype=F)
    normal[..., 1] = 1
    guides = dict(normal=normal, depth=np.full((h, w), F(0.75)), sphere_id=np.full((h, w), 3, dtype=np.uint32))
    cur = dict(beauty=g.random((h, w, 3), dtype=F), variance=g.random((h, w), dtype=F) * F(0.01),
               alpha=np.ones((h, w), dtype=F), **guides)
    prev = dict(color=g.random((h, w, 3), dtype=F), variance=g.random((h, w), dtype=F) * F(0.01),
                history=np.full((h, w), F(3)), **{n: a.copy() for n, a in guides.items()})
    return cam, cur, prev


def test_restatement_static_camera_blends_every_pixel_with_itself():
    """Static camera, matching guides: the reprojected position is the pixel's own centre up to
    rounding (a bilinear weight within 1e-3 of one tap), every pixel is kept, the history grows by
    one, k = 1 / N, and the blend is the running mean to float precision."""
    w, h = 12, 7
    cam, cur, prev = _planes(w, h, 3)
    par = rt.temporal_params(w, h, alpha_min=0.01, max_history=64.0, normal_tol=0.1, depth_tol=0.1)
    c, v, n, reason = temporal_ref.accumulate(cur, prev, cam, cam, par)
    assert (reason == temporal_ref.KEPT).all()
    assert np.abs(n - 4).max() < 1e-5
    assert np.abs(c - (0.25 * cur["beauty"] + 0.75 * prev["color"])).max() < 2e-3
    assert c.dtype == v.dtype == n.dtype == np.float32
    # max_history = 1: k = 1, the colour is the current beauty's bits, the variance the current one's
    par1 = rt.temporal_params(w, h, base=par, max_history=1.0)
    c1, v1, n1, _ = temporal_ref.accumulate(cur, prev, cam, cam, par1)
    assert np.array_equal(u32(c1), u32(cur["beauty"])) and np.array_equal(u32(v1), u32(cur["variance"])) and (n1 == 1).all()


def test_restatement_reasons():
    w, h = 12, 7
    cam, cur, prev = _planes(w, h, 4)
    par = rt.temporal_params(w, h)
    out = temporal_ref.accumulate(cur, None, cam, None, par)
    assert (out[3] == temporal_ref.NO_PREV).all() and np.array_equal(u32(out[0]), u32(cur["beauty"])) and (out[2] == 1).all()
    cur["alpha"][0, :] = F(0.5)          # edge pixels
    cur["sphere_id"][1, :] = 9           # another sphere than prev's: every tap rejected
    prev["depth"][2, :] = F(2.0)         # depth off by far more than depth_tol
    away = rt.Camera((-4, 3.2, 5), (-8, 5.4, 10), (0, 1, 0), w / h, 42.0, 0.0625, 6.4, rt.CORRECTED)
    c, v, n, reason = temporal_ref.accumulate(cur, prev, cam, cam, par)
    assert (reason[0] == temporal_ref.EDGE).all() and (reason[1:3] == temporal_ref.REJECTED).all()
    assert (reason[3:] == temporal_ref.KEPT).all()
    lost = reason != temporal_ref.KEPT
    assert np.array_equal(u32(c[lost]), u32(cur["beauty"][lost])) and (n[lost] == 1).all()
    _, _, _, reason = temporal_ref.accumulate(cur, prev, cam, away, par)
    assert (reason[3:] == temporal_ref.BEHIND).all() and (reason[0] == temporal_ref.EDGE).all()


# ---- argument checks --------------------------------------------------------------------------------
W0, H0 = 6, 4
_HOST = {n: np.zeros((H0, W0, 3) if ch == 3 else (H0, W0), dtype=dt) for n, (ch, dt) in abi.TEMPORAL_PLANES.items()}
PREV = tuple(n for n in abi.TEMPORAL_PLANES if n.startswith("prev_"))
OUT = tuple(n for n in abi.TEMPORAL_PLANES if n.startswith("out_"))
CUR = tuple(n for n in abi.TEMPORAL_PLANES if n not in PREV + OUT)


def _degenerate():
    c = abi.RtCamera.from_buffer_copy(bytes(rt.Camera.default(W0, H0).c))
    c.vertical[:] = (0.0, 1.0, 0.0)
    c.horizontal[:] = (0.0, 2.0, 0.0)
    return c


def _call(device, drop=(), alias=None, params_size=None, buffers_size=None, camera=True, prev_camera=True,
          raw=None, **fields):
    """The status and message of rt_temporal (host) or rt_temporal_device with host addresses, which
    a call that fails its checks never touches."""
    p = rt.temporal_params(W0, H0, **fields)
    for k, v in (raw or {}).items():
        setattr(p, k, v)
    if params_size is not None:
        p.size = params_size
    ptr = {n: a.ctypes.data for n, a in _HOST.items() if n not in drop}
    for a, b in (alias or {}).items():
        ptr[a] = ptr[b]
    rec = rt.temporal_buffers(ptr)
    if buffers_size is not None:
        rec.size = buffers_size
    cam = C.byref(rt.Camera.default(W0, H0).c) if camera else None
    prev = None if not prev_camera else C.byref(prev_camera if prev_camera is not True else rt.Camera.default(W0, H0).c)
    L = rt.lib()
    f = L.rt_temporal_device if device else L.rt_temporal
    rc = f(C.byref(p), cam, prev, C.byref(rec), None)
    return rc, L.rt_last_error().decode()


BAD = [
    ("params.size", dict(params_size=28)),
    ("buffers.size", dict(buffers_size=120)),
    ("width", dict(raw=dict(width=0))),
    ("width", dict(raw=dict(width=65537))),
    ("height", dict(raw=dict(height=0))),
    ("height", dict(raw=dict(height=65537))),
    ("alpha_min", dict(alpha_min=0.0)),
    ("alpha_min", dict(alpha_min=-0.5)),
    ("alpha_min", dict(alpha_min=1.5)),
    ("alpha_min", dict(alpha_min=float("nan"))),
    ("max_history", dict(max_history=0.5)),
    ("max_history", dict(max_history=float("inf"))),
    ("max_history", dict(max_history=float("nan"))),
    ("normal_tol", dict(normal_tol=-1e-3)),
    ("normal_tol", dict(normal_tol=float("nan"))),
    ("depth_tol", dict(depth_tol=-1.0)),
    ("depth_tol", dict(depth_tol=float("inf"))),
    ("flags", dict(flags=1)),
    ("camera", dict(camera=False)),
    ("prev_camera", dict(prev_camera=False)),
    ("prev_camera", dict(prev_camera=_degenerate())),
] + [(n, dict(drop=(n,))) for n in CUR + OUT] + [
    # prev partly given: one plane missing, and one plane alone
    (n, dict(drop=(n,))) for n in PREV] + [
    ("prev_", dict(drop=PREV[1:])),
] + [(o, dict(alias={o: i})) for o in OUT for i in CUR + PREV] + [
    ("out_variance", dict(alias={"out_variance": "out_color"})),
    ("out_history", dict(alias={"out_history": "out_color"})),
    ("out_history", dict(alias={"out_history": "out_variance"})),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("field,kw", BAD, ids=[f"{i}-{f}" for i, (f, _) in enumerate(BAD)])
def test_argument_checks_name_the_field(field, kw, device):
    """RT_ERR_INVALID before any device call (this test runs without a GPU), the field named."""
    rc, msg = _call(device, **kw)
    assert rc == abi.RT_ERR_INVALID, (rc, msg)
    assert field in msg and msg.startswith("rt_temporal_device:" if device else "rt_temporal:"), msg


def test_null_records_fail_and_prev_camera_is_ignored_without_history():
    L = rt.lib()
    assert L.rt_temporal(None, None, None, None, None) == abi.RT_ERR_INVALID
    assert L.rt_temporal_device(None, None, None, None, None) == abi.RT_ERR_INVALID
    # no prev plane: a null or degenerate prev_camera is no error (without a GPU only the device is
    # missing). The host call alone: these arguments pass, and the planes are host memory.
    for prev_camera in (False, _degenerate()):
        rc, msg = _call(False, drop=PREV, prev_camera=prev_camera)
        assert rc != abi.RT_ERR_INVALID, msg


def test_python_wrapper_checks_planes_shapes_and_dtypes():
    cam = rt.Camera.default(W0, H0)
    cur = {n: _HOST[n] for n in CUR}
    with pytest.raises(KeyError):
        rt.temporal({n: cur[n] for n in CUR[1:]}, None, cam, None)
    with pytest.raises(KeyError):
        rt.temporal(cur, {"color": _HOST["prev_color"]}, cam, cam)
    with pytest.raises(ValueError):
        rt.temporal({**cur, "sphere_id": _HOST["sphere_id"].astype(np.float32)}, None, cam, None)
    with pytest.raises(ValueError):
        rt.temporal({**cur, "depth": _HOST["depth"][:, 1:]}, None, cam, None)
    with pytest.raises(KeyError):
        rt.temporal(cur, None, cam, None, alpha=1.0)
