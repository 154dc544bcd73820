"""TEST INFRASTRUCTURE: CPU restatement of the temporal stage with object motion (include/rt_api.h,
rt_temporal_motion_t) in numpy float32, written from the contract and not from the
kernel. It restates the whole stage, so that equality with temporal_ref.accumulate under equal tables
is a test and not a construction; the helpers that state the camera record and the projection are
temporal_ref's.

    color, variance, history, reason = temporal_motion_ref.accumulate(cur, prev, camera, prev_camera, params,
                                                                      centres, prev_centres)

centres, prev_centres: float32 (n, 4) {cx, cy, cz, r}, now and at the previous frame. reason: the
codes of temporal_ref and RESIZED: a surface pixel whose id is at or above n, or whose sphere's
radius bits differ between the tables. Neither table is indexed at an id at or above n.
"""
import numpy as np

import temporal_ref as T
from temporal_ref import BEHIND, EDGE, KEPT, NO_PREV, OFFSCREEN, REJECTED  # noqa: F401

F = np.float32
RESIZED = 6
REASONS = {**T.REASONS, RESIZED: "resized or unknown sphere"}


def accumulate(cur, prev, camera, prev_camera, params, centres, prev_centres):
    beauty = np.asarray(cur["beauty"], dtype=F)
    variance = np.asarray(cur["variance"], dtype=F)
    h, w = variance.shape
    if prev is None:
        return beauty.copy(), variance.copy(), np.ones((h, w), dtype=F), np.full((h, w), NO_PREV, dtype=np.uint8)
    now, was = np.asarray(centres, dtype=F).reshape(-1, 4), np.asarray(prev_centres, dtype=F).reshape(-1, 4)
    n_spheres = len(now)
    assert len(was) == n_spheres
    record = T.basis(prev_camera)
    assert record is not None, "degenerate prev_camera"
    normal, depth, alpha = (np.asarray(cur[n], dtype=F) for n in ("normal", "depth", "alpha"))
    sid = np.asarray(cur["sphere_id"], dtype=np.uint32)
    p_color, p_var, p_hist, p_normal, p_depth = (np.asarray(prev[n], dtype=F)
                                                 for n in ("color", "variance", "history", "normal", "depth"))
    p_id = np.asarray(prev["sphere_id"], dtype=np.uint32)
    alpha_min, max_history = F(params.alpha_min), F(params.max_history)
    normal_tol, depth_tol = F(params.normal_tol), F(params.depth_tol)

    surface, sky = alpha == F(1), alpha == F(0)
    # step 3 of a surface pixel: the sphere's motion, from the two rows of its id
    known = sid < n_spheres
    row = np.where(known, sid, 0).astype(np.int64)  # (an id outside the tables indexes neither)
    if n_spheres:
        c_now, c_was = now[row], was[row]
        same_r = c_now[..., 3].view(np.uint32) == c_was[..., 3].view(np.uint32)
        with np.errstate(all="ignore"):
            m = c_now[..., :3] - c_was[..., :3]
    else:
        same_r = np.zeros((h, w), dtype=bool)
        m = np.zeros((h, w, 3), dtype=F)
    tracked = known & same_r
    resized = surface & ~tracked
    d = T.pixel_rays(camera, w, h)
    o, o_prev = T._vec(T._record(camera).origin), record[9:12]
    with np.errstate(all="ignore"):
        q = np.where(surface[..., None], ((o + depth[..., None] * d) - m) - o_prev, d)
    assert q.dtype == F and m.dtype == F
    ga, px, py = T.project(q, record, w, h)
    with np.errstate(invalid="ignore"):
        front = ga > F(0)
        inside = (px > F(-1)) & (px < F(w)) & (py > F(-1)) & (py < F(h))
    live = (surface | sky) & ~resized & front & inside
    px, py = np.where(live, px, F(0)), np.where(live, py, F(0))
    fx, fy = np.floor(px), np.floor(py)
    tx, ty = px - fx, py - fy
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    with np.errstate(all="ignore"):
        ztol = depth_tol * ga
    sumw, sumv, sumn = (np.zeros((h, w), dtype=F) for _ in range(3))
    acc = np.zeros((h, w, 3), dtype=F)
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = ix + i, iy + j
            ok = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            ok &= p_id[cy, cx] == sid
            dn = p_normal[cy, cx] - normal
            d2 = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
            with np.errstate(invalid="ignore"):
                ok &= ~(d2 > normal_tol)
                ok &= ~(surface & (np.abs(p_depth[cy, cx] - ga) > ztol))
            wgt = (tx if i else F(1) - tx) * (ty if j else F(1) - ty)
            assert wgt.dtype == F and d2.dtype == F
            with np.errstate(all="ignore"):
                sumw = np.where(ok, sumw + wgt, sumw)
                acc = np.where(ok[..., None], acc + wgt[..., None] * p_color[cy, cx], acc)
                sumv = np.where(ok, sumv + (wgt * wgt) * p_var[cy, cx], sumv)
                sumn = np.where(ok, sumn + wgt * p_hist[cy, cx], sumn)
    enough = sumw >= F(0.01)
    kept = live & enough
    with np.errstate(all="ignore"):
        c_h = acc / sumw[..., None]
        v_h = sumv / (sumw * sumw)
        n_h = sumn / sumw
        n = np.fmin(n_h + F(1), max_history)
        k = np.fmax(F(1) / n, alpha_min)
        rest = F(1) - k
        blend_c = k[..., None] * beauty + rest[..., None] * c_h
        blend_v = (k * k) * variance + (rest * rest) * v_h
    assert blend_c.dtype == F and blend_v.dtype == F and n.dtype == F
    out_c = np.where(kept[..., None], blend_c, beauty)
    out_v = np.where(kept, blend_v, variance)
    out_n = np.where(kept, n, F(1))
    reason = np.full((h, w), KEPT, dtype=np.uint8)
    reason[live & ~enough] = REJECTED
    reason[(surface | sky) & front & ~inside] = OFFSCREEN
    reason[(surface | sky) & ~front] = BEHIND
    reason[resized] = RESIZED
    reason[~(surface | sky)] = EDGE
    return out_c, out_v, out_n, reason
