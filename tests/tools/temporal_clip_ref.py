"""TEST INFRASTRUCTURE: CPU restatement of the temporal stage with the history clamp (include/rt_api.h,
rt_temporal_clip_t) in numpy float32, written from the contract and not from the
kernel. It restates the whole stage (steps 1 to 7 with step 5b between the resample and the blend), so
that its agreement with temporal_ref / temporal_motion_ref where nothing is clamped is a test and not a
construction; the helpers that state the camera record and the projection are temporal_ref's.

    box = temporal_clip_ref.window_box(beauty, sphere_id, radius, gamma)      # lo, hi: float32 (h, w, 3)
    color, variance, history, reason, info = temporal_clip_ref.accumulate(cur, prev, camera, prev_camera, params,
                                                                          clip, centres=None, prev_centres=None)

clip: anything with radius and gamma (an rt_temporal_clip_t record). centres, prev_centres: the two
tables of the stage with object motion, or both None: the static stage. reason: temporal_motion_ref's
codes. info: dict with lo, hi (the box of every pixel), resampled (C_h before the clamp), clamped (C_h
after it) and changed (bool (h, w): a pixel with history one of whose channels the clamp changed);
None without prev.
"""
import numpy as np

import temporal_ref as T
from temporal_motion_ref import BEHIND, EDGE, KEPT, NO_PREV, OFFSCREEN, REJECTED, REASONS, RESIZED  # noqa: F401

F = np.float32


def window_box(beauty, sphere_id, radius, gamma):
    """Step 5b's window and box for every pixel: (lo, hi), float32 (h, w, 3)."""
    b = np.asarray(beauty, dtype=F)
    sid = np.asarray(sphere_id, dtype=np.uint32)
    h, w = sid.shape
    r, gamma = int(radius), F(gamma)
    n = np.zeros((h, w), dtype=F)
    m1, m2 = np.zeros((h, w, 3), dtype=F), np.zeros((h, w, 3), dtype=F)
    ys, xs = np.mgrid[0:h, 0:w]
    for j in range(-r, r + 1):
        for i in range(-r, r + 1):
            qx, qy = xs + i, ys + j
            ok = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)   # (a skipped tap is computed and masked out)
            ok &= sid[cy, cx] == sid
            d = b[cy, cx] - b
            n = np.where(ok, n + F(1), n)
            m1 = np.where(ok[..., None], m1 + d, m1)
            m2 = np.where(ok[..., None], m2 + d * d, m2)
    assert (n >= 1).all()   # the centre tap always counts
    mean = m1 / n[..., None]
    ex2 = m2 / n[..., None]
    s2 = np.fmax(F(0), ex2 - mean * mean)
    half = gamma * np.sqrt(s2)
    mu = b + mean
    lo, hi = mu - half, mu + half
    assert lo.dtype == F and hi.dtype == F and half.dtype == F
    return lo, hi


def accumulate(cur, prev, camera, prev_camera, params, clip, centres=None, prev_centres=None):
    beauty = np.asarray(cur["beauty"], dtype=F)
    variance = np.asarray(cur["variance"], dtype=F)
    h, w = variance.shape
    if prev is None:
        return beauty.copy(), variance.copy(), np.ones((h, w), dtype=F), np.full((h, w), NO_PREV, dtype=np.uint8), None
    motion = centres is not None
    assert motion == (prev_centres is not None)
    record = T.basis(prev_camera)
    assert record is not None, "degenerate prev_camera"
    normal, depth, alpha = (np.asarray(cur[n], dtype=F) for n in ("normal", "depth", "alpha"))
    sid = np.asarray(cur["sphere_id"], dtype=np.uint32)
    p_color, p_var, p_hist, p_normal, p_depth = (np.asarray(prev[n], dtype=F)
                                                 for n in ("color", "variance", "history", "normal", "depth"))
    p_id = np.asarray(prev["sphere_id"], dtype=np.uint32)
    alpha_min, max_history = F(params.alpha_min), F(params.max_history)
    normal_tol, depth_tol = F(params.normal_tol), F(params.depth_tol)

    # steps 1 to 3
    surface, sky = alpha == F(1), alpha == F(0)
    d = T.pixel_rays(camera, w, h)
    o, o_prev = T._vec(T._record(camera).origin), record[9:12]
    resized = np.zeros((h, w), dtype=bool)
    with np.errstate(all="ignore"):
        hit = o + depth[..., None] * d
        if motion:
            now, was = np.asarray(centres, dtype=F).reshape(-1, 4), np.asarray(prev_centres, dtype=F).reshape(-1, 4)
            assert len(now) == len(was)
            known = sid < len(now)
            row = np.where(known, sid, 0).astype(np.int64)      # (an id outside the tables indexes neither)
            if len(now):
                c_now, c_was = now[row], was[row]
                same_r = c_now[..., 3].view(np.uint32) == c_was[..., 3].view(np.uint32)
                m = c_now[..., :3] - c_was[..., :3]
            else:
                same_r, m = np.zeros((h, w), dtype=bool), np.zeros((h, w, 3), dtype=F)
            resized = surface & ~(known & same_r)
            hit = hit - m
        q = np.where(surface[..., None], hit - o_prev, d)
    assert q.dtype == F
    # step 4
    ga, px, py = T.project(q, record, w, h)
    with np.errstate(invalid="ignore"):
        front = ga > F(0)
        inside = (px > F(-1)) & (px < F(w)) & (py > F(-1)) & (py < F(h))
    live = (surface | sky) & ~resized & front & inside
    # step 5 (a pixel that is not live is computed at a harmless position and masked out at the end)
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
    # step 5b: the box of the current frame's window, and the clamp
    lo, hi = window_box(beauty, sid, clip.radius, clip.gamma)
    with np.errstate(all="ignore"):
        c_h = acc / sumw[..., None]
        clamped = np.fmin(np.fmax(c_h, lo), hi)
        # step 6
        v_h = sumv / (sumw * sumw)
        n_h = sumn / sumw
        n = np.fmin(n_h + F(1), max_history)
        k = np.fmax(F(1) / n, alpha_min)
        rest = F(1) - k
        blend_c = k[..., None] * beauty + rest[..., None] * clamped
        blend_v = (k * k) * variance + (rest * rest) * v_h
    assert blend_c.dtype == F and blend_v.dtype == F and n.dtype == F and clamped.dtype == F
    out_c = np.where(kept[..., None], blend_c, beauty)
    out_v = np.where(kept, blend_v, variance)
    out_n = np.where(kept, n, F(1))
    reason = np.full((h, w), KEPT, dtype=np.uint8)
    reason[live & ~enough] = REJECTED
    reason[(surface | sky) & front & ~inside] = OFFSCREEN
    reason[(surface | sky) & ~front] = BEHIND
    reason[resized] = RESIZED
    reason[~(surface | sky)] = EDGE
    changed = kept & (clamped.view(np.uint32) != c_h.view(np.uint32)).any(axis=2)
    info = dict(lo=lo, hi=hi, resampled=c_h, clamped=clamped, changed=changed)
    return out_c, out_v, out_n, reason, info
