"""Moving spheres without a GPU: the restatement of the temporal stage with object
motion (tests/tools/temporal_motion_ref.py) against the static one and against geometry, every
argument check of rt_temporal_motion* and the record checks of rt_scene_update (all made before any
device call), and the host-only precondition of the update tests on the GPU.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import temporal_motion_ref as M  # noqa: E402
from motion_cases import huge_a_b, huge_far_a_b, records_a_b  # noqa: E402
import temporal_ref as T  # noqa: E402
from support import assert_bits, words as u32  # noqa: E402

F = np.float32


def synthetic_planes(w, h, seed):
    """Planes of the kind the temporal CPU test uses (a surface everywhere, matching guides, one id),
    with a few sky and edge pixels and a second id so that every class occurs."""
    g = np.random.default_rng(seed)
    cam = rt.Camera.default(w, h, rt.CORRECTED)
    normal = np.zeros((h, w, 3), dtype=F)
    normal[..., 1] = 1
    sid = np.full((h, w), 3, dtype=np.uint32)
    sid[:, w // 2:] = 1
    depth = np.full((h, w), F(0.75))
    alpha = np.ones((h, w), dtype=F)
    alpha[0, :] = F(0.5)
    alpha[1, :] = F(0)
    for a in (normal, depth):
        a[1] = 0
    sid[1, :] = 0xffffffff
    guides = dict(normal=normal, depth=depth, sphere_id=sid)
    cur = dict(beauty=g.random((h, w, 3), dtype=F), variance=g.random((h, w), dtype=F) * F(0.01), alpha=alpha, **guides)
    prev = dict(color=g.random((h, w, 3), dtype=F), variance=g.random((h, w), dtype=F) * F(0.01),
                history=np.full((h, w), F(3)), **{n: a.copy() for n, a in guides.items()})
    return cam, cur, prev


def test_record_sizes():
    assert C.sizeof(abi.RtTemporalMotion) == 24 and C.sizeof(abi.RtSceneMotion) == 40
    s, m = rt.simple_scene_arrays()
    t = rt.sphere_table((s, m))
    assert t.dtype == np.float32 and t.shape == (5, 4)
    assert np.array_equal(u32(t[:, :3]), u32(s["center"])) and np.array_equal(u32(t[:, 3]), u32(s["radius"]))


def test_equal_tables_give_the_static_restatement_bit_for_bit():
    """m = +0 and x - (+0) = x: with prev_centres == centres the motion restatement's every output
    is temporal_ref.accumulate's, for a static and for a moved camera."""
    w, h = 48, 27
    cam, cur, prev = synthetic_planes(w, h, 11)
    moved = rt.Camera((-8.2, 5.4, 10.1), (-4, 3.2, 5), (0, 1, 0), w / h, 42.0, 0.0625, 6.4, rt.CORRECTED)
    table = np.random.default_rng(5).normal(size=(6, 4)).astype(F)
    table[2, 0] = F(-0.0)
    par = rt.temporal_params(w, h)
    for prev_cam in (cam, moved):
        want = T.accumulate(cur, prev, cam, prev_cam, par)
        got = M.accumulate(cur, prev, cam, prev_cam, par, table, table.copy())
        for a, b in zip(got[:3], want[:3]):
            assert_bits(a, b)
        assert np.array_equal(got[3], want[3])
    kept = T.accumulate(cur, prev, cam, cam, par)[3]
    assert (kept == T.KEPT).sum() > w * h // 2 and (kept == T.EDGE).sum() == w


def test_one_pixel_shift():
    """A static corrected camera, one id over the frame, constant depth t and normal; the sphere moved
    by m = t * horizontal / w, one pixel to the right at that depth. The previous frame saw the point
    under pixel x at x - 1: every interior pixel is KEPT and projects within 1e-3 of x - 1 (the
    projection's own error is ~1e-4 pixels, test_temporal_cpu), and the left column, whose source is
    x = -1, half a pixel outside the image's taps, is OFFSCREEN or has every tap rejected."""
    w, h = 48, 27
    cam = rt.Camera.default(w, h, rt.CORRECTED)
    t = F(0.75)
    hor = np.array(cam.c.horizontal[:], dtype=F)
    m = (t * hor) / F(w)
    now = np.array([[0, 0, 0, 1], [1, 2, 3, 0.5]], dtype=F)
    was = now.copy()
    was[1, :3] = now[1, :3] - m
    m_used = now[1, :3] - was[1, :3]
    normal = np.zeros((h, w, 3), dtype=F)
    normal[..., 2] = 1
    g = np.random.default_rng(2)
    guides = dict(normal=normal, depth=np.full((h, w), t), sphere_id=np.full((h, w), 1, dtype=np.uint32))
    cur = dict(beauty=g.random((h, w, 3), dtype=F), variance=g.random((h, w), dtype=F), alpha=np.ones((h, w), dtype=F),
               **guides)
    # the previous colour encodes its own column, so that the blend shows where it was read
    col = np.broadcast_to(np.arange(w, dtype=F)[None, :, None], (h, w, 3)).copy()
    prev = dict(color=col, variance=np.zeros((h, w), dtype=F), history=np.full((h, w), F(1)),
                **{n: a.copy() for n, a in guides.items()})
    par = rt.temporal_params(w, h, alpha_min=0.5, max_history=2.0)
    c, v, n, reason = M.accumulate(cur, prev, cam, cam, par, now, was)
    assert (reason[:, 1:] == M.KEPT).all(), np.unique(reason[:, 1:])
    assert np.isin(reason[:, 0], (M.OFFSCREEN, M.REJECTED, M.KEPT)).all()
    # the position, from the restatement's own pieces
    record = T.basis(cam)
    d = T.pixel_rays(cam, w, h)
    o = np.array(cam.c.origin[:], dtype=F)
    q = ((o + t * d) - m_used) - record[9:12]
    _, px, py = T.project(q, record, w, h)
    xs = np.arange(w, dtype=np.float64)[None, :]
    ys = np.arange(h, dtype=np.float64)[:, None]
    err_x, err_y = np.abs(px - (xs - 1)).max(), np.abs(py - ys).max()
    print(f"largest distance from (x - 1, y): {err_x:.2e}, {err_y:.2e} pixels")
    assert err_x < 1e-3 and err_y < 1e-3
    # k = 0.5: the blend's history half is the column x - 1 within the bilinear weight's error
    hist = (c[:, 1:] - F(0.5) * cur["beauty"][:, 1:]) * F(2)
    assert np.abs(hist - (xs[:, 1:, None] - 1)).max() < 0.05
    # the left column: off-screen, or nothing but a sliver of column 0 (weight ~1e-4 < 0.01)
    assert not (reason[:, 0] == M.KEPT).any()
    assert_bits(c[:, 0], cur["beauty"][:, 0])
    # the static stage on the same planes keeps every pixel at its own column: the motion matters
    cs = T.accumulate(cur, prev, cam, cam, par)[0]
    assert (u32(cs) != u32(c)).any(axis=2).sum() > w * h // 2


def test_resized_and_unknown_ids_restart():
    w, h = 12, 7
    cam, cur, prev = synthetic_planes(w, h, 3)
    par = rt.temporal_params(w, h)
    now = np.zeros((4, 4), dtype=F)
    now[:, 3] = 1
    was = now.copy()
    was[1, 3] = np.nextafter(F(1), F(2))      # id 1: the radius differs in its last bit
    was[0] = np.nan                            # rows no pixel names may hold anything
    c, v, n, reason = M.accumulate(cur, prev, cam, cam, par, now, was)
    assert (reason[2:, w // 2:] == M.RESIZED).all() and (reason[2:, :w // 2] == M.KEPT).all()
    assert (reason[0] == M.EDGE).all() and (reason[1] == M.KEPT).all()      # edge and sky rows are untouched
    # three rows only: id 3 is now outside the tables
    c, v, n, reason = M.accumulate(cur, prev, cam, cam, par, now[:3], now[:3])
    assert (reason[2:, :w // 2] == M.RESIZED).all() and (reason[2:, w // 2:] == M.KEPT).all()
    lost = reason == M.RESIZED
    assert np.array_equal(u32(c[lost]), u32(cur["beauty"][lost])) and (n[lost] == 1).all()
    # no table at all
    reason = M.accumulate(cur, prev, cam, cam, par, np.zeros((0, 4), F), np.zeros((0, 4), F))[3]
    assert (reason[2:] == M.RESIZED).all() and (reason[1] == M.KEPT).all()


# ---- argument checks of rt_temporal_motion / rt_temporal_motion_device -------------------------------
W0, H0 = 6, 4
_HOST = {n: np.zeros((H0, W0, 3) if ch == 3 else (H0, W0), dtype=dt) for n, (ch, dt) in abi.TEMPORAL_PLANES.items()}
_TABLES = [np.zeros((8, 4), dtype=F), np.zeros((8, 4), dtype=F)]


def _call(device, motion="ok", drop=(), alias=None, **fields):
    p = rt.temporal_params(W0, H0, **fields)
    ptr = {n: a.ctypes.data for n, a in _HOST.items() if n not in drop}
    for a, b in (alias or {}).items():
        ptr[a] = ptr[b]
    rec = rt.temporal_buffers(ptr)
    cam = rt.Camera.default(W0, H0).c
    m = abi.RtTemporalMotion(C.sizeof(abi.RtTemporalMotion), 8, _TABLES[0].ctypes.data, _TABLES[1].ctypes.data)
    if callable(motion):
        motion(m, ptr)
    L = rt.lib()
    f = L.rt_temporal_motion_device if device else L.rt_temporal_motion
    rc = f(C.byref(p), C.byref(cam), C.byref(cam), C.byref(rec), None if motion is None else C.byref(m), None)
    return rc, L.rt_last_error().decode()


def _set(**kw):
    def apply(m, ptr):
        for k, v in kw.items():
            setattr(m, k, ptr[v] if isinstance(v, str) else v)
    return apply


BAD = [
    ("alpha_min", dict(alpha_min=0.0)),                      # rt_temporal_device's checks come first
    ("out_color", dict(drop=("out_color",))),
    ("prev_depth", dict(drop=("prev_depth",))),
    ("out_history", dict(alias={"out_history": "beauty"})),
    ("motion", dict(motion=None)),
    ("motion.size", dict(motion=_set(size=16))),
    ("motion.centres", dict(motion=_set(centres=None))),
    ("motion.prev_centres", dict(motion=_set(prev_centres=None))),
    ("motion.centres", dict(motion=_set(centres="out_color"))),
    ("motion.centres", dict(motion=_set(centres="out_history"))),
    ("motion.prev_centres", dict(motion=_set(prev_centres="out_variance"))),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("field,kw", BAD, ids=[f"{i}-{f}" for i, (f, _) in enumerate(BAD)])
def test_motion_argument_checks_name_the_field(field, kw, device):
    """RT_ERR_INVALID before any device call (this test runs without a GPU), the field named."""
    rc, msg = _call(device, **kw)
    assert rc == abi.RT_ERR_INVALID, (rc, msg)
    assert field in msg and msg.startswith("rt_temporal_motion_device:" if device else "rt_temporal_motion:"), msg


def test_motion_record_is_checked_without_history_and_tables_may_be_one():
    PREV = tuple(n for n in abi.TEMPORAL_PLANES if n.startswith("prev_"))
    rc, msg = _call(True, drop=PREV, motion=_set(size=16))
    assert rc == abi.RT_ERR_INVALID and "motion.size" in msg
    # an unaligned table is refused by the device call (a row is one 16-byte load), not by the host call
    rc, msg = _call(True, motion=_set(centres=_TABLES[0].ctypes.data + 4))
    assert rc == abi.RT_ERR_INVALID and "16-byte" in msg
    # these pass every check; without a GPU only the device is missing. The host call alone: its planes
    # are host memory. No sphere: null tables are fine; the same table twice is fine.
    for ok in (_set(n_spheres=0, centres=None, prev_centres=None), _set(prev_centres=_TABLES[0].ctypes.data),
               _set(centres=_TABLES[0].ctypes.data + 4)):
        rc, msg = _call(False, motion=ok)
        assert rc != abi.RT_ERR_INVALID, msg
    L = rt.lib()
    assert L.rt_temporal_motion(None, None, None, None, None, None) == abi.RT_ERR_INVALID
    assert L.rt_temporal_motion_device(None, None, None, None, None, None) == abi.RT_ERR_INVALID


def test_python_wrapper_checks_the_tables():
    cam = rt.Camera.default(W0, H0)
    cur = {n: _HOST[n] for n in ("beauty", "variance", "normal", "depth", "alpha", "sphere_id")}
    with pytest.raises(ValueError):
        rt.temporal(cur, None, cam, None, motion=(np.zeros((3, 4), F), np.zeros((2, 4), F)))
    with pytest.raises(ValueError):
        rt.temporal(cur, None, cam, None, motion=(np.zeros((3, 4), np.float64), np.zeros((3, 4), np.float64)))


# ---- rt_scene_update's record checks: before the scene is looked at, so a null scene serves -----------
def _update(s, m, n_spheres=None, n_materials=None, spheres=True, materials=True):
    L = rt.lib()
    rc = L.rt_scene_update(None, abi.ptr(s, C.POINTER(abi.RtSphere)) if spheres else None,
                           len(s) if n_spheres is None else n_spheres,
                           abi.ptr(m, C.POINTER(abi.RtMaterial)) if materials else None,
                           len(m) if n_materials is None else n_materials)
    return rc, L.rt_last_error().decode()


def test_scene_update_checks_the_records_before_the_scene():
    s, m = rt.simple_scene_arrays()
    bad = s.copy()
    bad["material"][2] = 4
    rc, msg = _update(bad, m)
    assert rc == abi.RT_ERR_INVALID and msg.startswith("rt_scene_update:") and "sphere 2" in msg and "material index" in msg
    kind = m.copy()
    kind["kind"][1] = 3
    rc, msg = _update(s, kind)
    assert rc == abi.RT_ERR_INVALID and "material 1" in msg and "kind" in msg
    rc, msg = _update(s, m, spheres=False)
    assert rc == abi.RT_ERR_INVALID and "spheres is null" in msg
    rc, msg = _update(s, m, materials=False)
    assert rc == abi.RT_ERR_INVALID and "materials is null" in msg
    rc, msg = _update(s, m, n_materials=0)
    assert rc == abi.RT_ERR_INVALID and "n_materials" in msg
    # good records: the next check is the scene itself
    rc, msg = _update(s, m)
    assert rc == abi.RT_ERR_INVALID and "scene is null" in msg
    L = rt.lib()
    assert L.rt_scene_motion(None, None) == abi.RT_ERR_INVALID and "rt_scene_motion" in L.rt_last_error().decode()


# ---- the precondition of the update tests on the GPU ----------------------------------------------------
def test_update_precondition_trap_windows_and_tile_order_differ():
    A, B = records_a_b()
    wa, wb = rt.trap_windows(A), rt.trap_windows(B)
    assert not np.array_equal(u32(wa[3]), u32(wb[3])), (wa[3], wb[3])
    assert tuple(wa[3]) == (1.0, 0.0) and wb[3][0] < wb[3][1]
    p = rt.make_params(64, 40, 4)
    pa, la, sa = rt.tile_order(A, p)
    pb, lb, sb = rt.tile_order(B, p)
    assert len(pa) == len(pb) == 64 * 40 // 64
    assert not np.array_equal(pa, pb) or (la, sa) != (lb, sb)
    assert not np.array_equal(pa, pb)


def test_update_precondition_of_the_huge_pairs():
    """The device scene of the simple pair has no clusters and so no dealing order: the cached orders are
    exercised by the huge pairs. Both change trap windows; the far one changes the order too."""
    p = rt.make_params(64, 40, 4)
    cam = rt.Camera.default(64, 40, rt.CORRECTED)
    for pair, order_differs in ((huge_a_b, False), (huge_far_a_b, True)):
        A, B = pair()
        wa, wb = rt.trap_windows(A), rt.trap_windows(B)
        assert all(wa[i][0] < wa[i][1] and not np.array_equal(u32(wa[i]), u32(wb[i])) for i in (12, 13, 15))
        (pa, la, sa), (pb, lb, sb) = rt.tile_order(A, p, cam), rt.tile_order(B, p, cam)
        assert (not np.array_equal(pa, pb) or (la, sa) != (lb, sb)) == order_differs
