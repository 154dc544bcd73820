"""TEST INFRASTRUCTURE: CPU restatement of the temporal accumulation's contract (include/rt_api.h,
rt_temporal_buffers) in numpy float32, written from the contract and not from the
kernel.

    record = temporal_ref.basis(camera)                                  # float32 (12,): {A, B, G, o'}
    color, variance, history, reason = temporal_ref.accumulate(cur, prev, camera, prev_camera, params)

cur: dict of the current frame's planes (beauty, variance, normal, depth, alpha, sphere_id); prev:
dict of the previous frame's (color, variance, history, normal, depth, sphere_id) or None; the
cameras rt.Camera objects or rt_camera records; params anything with alpha_min, max_history,
normal_tol, depth_tol (an rt_temporal_params record). reason: uint8 per pixel, one of KEPT, EDGE,
BEHIND, OFFSCREEN, REJECTED (all taps rejected: sumw < 0.01), NO_PREV.

Vectorised over pixels, one numpy operation per contract operation; every scalar is an np.float32
and every array float32. A pixel that drops out at a step keeps being computed with whatever its
values give (the results are masked out at the end), as the taps of a skipped tap are.
"""
import numpy as np

F = np.float32
KEPT, EDGE, BEHIND, OFFSCREEN, REJECTED, NO_PREV = range(6)
REASONS = {KEPT: "kept", EDGE: "edge", BEHIND: "behind", OFFSCREEN: "off-screen", REJECTED: "all taps rejected",
           NO_PREV: "no prev"}


def _record(camera):
    return getattr(camera, "c", camera)


def _vec(a):
    return np.array([a[0], a[1], a[2]], dtype=F)


def _cross(x, y):
    return np.array([x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]], dtype=F)


def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def _corner(c):
    """a of the contract: the image plane's lower left corner as the pinhole ray's direction sees it."""
    llc = _vec(c.lower_left_corner)
    return llc - _vec(c.origin) if c.mode == 1 else llc


def basis(camera):
    """{A, B, G, o'} of the contract for a previous camera; None where rt_reproject_basis refuses."""
    c = _record(camera)
    h, v, a, o = _vec(c.horizontal), _vec(c.vertical), _corner(c), _vec(c.origin)
    with np.errstate(all="ignore"):
        va, ah, hv = _cross(v, a), _cross(a, h), _cross(h, v)
        d = _dot(h, va)
        out = np.concatenate([va / d, ah / d, hv / d, o]).astype(F)
    assert d.dtype == F
    if d == 0 or not np.isfinite(out).all():
        return None
    return out


def project(q, record, w, h):
    """Steps 4's (ga, px, py) for q of shape (..., 3) (q = P - o' already formed)."""
    A, B, G = record[0:3], record[3:6], record[6:9]
    qx, qy, qz = q[..., 0], q[..., 1], q[..., 2]
    al = (A[0] * qx + A[1] * qy) + A[2] * qz
    be = (B[0] * qx + B[1] * qy) + B[2] * qz
    ga = (G[0] * qx + G[1] * qy) + G[2] * qz
    with np.errstate(all="ignore"):
        px = (al / ga) * F(w) - F(0.5)
        py = (F(1) - be / ga) * F(h) - F(0.5)
    assert ga.dtype == F and px.dtype == F and py.dtype == F
    return ga, px, py


def pixel_rays(camera, w, h):
    """Step 2: d of every pixel, float32 (h, w, 3)."""
    c = _record(camera)
    a, hor, ver = _corner(c), _vec(c.horizontal), _vec(c.vertical)
    u = (np.arange(w, dtype=F) + F(0.5)) / F(w)
    m = F(1) - (np.arange(h, dtype=F) + F(0.5)) / F(h)
    d = np.empty((h, w, 3), dtype=F)
    for k in range(3):
        d[..., k] = (a[k] + hor[k] * u)[None, :] + (ver[k] * m)[:, None]
    return d


def accumulate(cur, prev, camera, prev_camera, params):
    beauty = np.asarray(cur["beauty"], dtype=F)
    variance = np.asarray(cur["variance"], dtype=F)
    h, w = variance.shape
    out_c, out_v, out_n = beauty.copy(), variance.copy(), np.ones((h, w), dtype=F)
    if prev is None:
        return out_c, out_v, out_n, np.full((h, w), NO_PREV, dtype=np.uint8)
    record = basis(prev_camera)
    assert record is not None, "degenerate prev_camera"
    normal, depth, alpha = (np.asarray(cur[n], dtype=F) for n in ("normal", "depth", "alpha"))
    sid = np.asarray(cur["sphere_id"], dtype=np.uint32)
    p_color, p_var, p_hist, p_normal, p_depth = (np.asarray(prev[n], dtype=F)
                                                 for n in ("color", "variance", "history", "normal", "depth"))
    p_id = np.asarray(prev["sphere_id"], dtype=np.uint32)
    alpha_min, max_history = F(params.alpha_min), F(params.max_history)
    normal_tol, depth_tol = F(params.normal_tol), F(params.depth_tol)

    surface, sky = alpha == F(1), alpha == F(0)
    d = pixel_rays(camera, w, h)
    o, o_prev = _vec(_record(camera).origin), record[9:12]
    q = np.where(surface[..., None], (o + depth[..., None] * d) - o_prev, d)
    assert q.dtype == F
    ga, px, py = project(q, record, w, h)
    front = ga > F(0)
    with np.errstate(invalid="ignore"):
        inside = (px > F(-1)) & (px < F(w)) & (py > F(-1)) & (py < F(h))
    live = (surface | sky) & front & inside
    # pixels that are not live are computed at a harmless position and masked out at the end
    px, py = np.where(live, px, F(0)), np.where(live, py, F(0))
    fx, fy = np.floor(px), np.floor(py)
    tx, ty = px - fx, py - fy
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
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
    reason[~(surface | sky)] = EDGE
    return out_c, out_v, out_n, reason
