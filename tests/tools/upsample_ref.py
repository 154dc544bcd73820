"""TEST INFRASTRUCTURE: CPU restatement of the guided upsample's contract (include/rt_api.h,
rt_upsample_buffers) in numpy float32, written from the contract and not from the
kernel.

    color, variance, reason, outside = upsample_ref.upsample(lo, guides, params)

lo: dict of the low-resolution planes (color, normal, depth, sphere_id, and optionally variance);
guides: dict of the output-size planes (normal, depth, alpha, sphere_id); params anything with
normal_tol and depth_tol (an rt_upsample_params record). variance is None when lo holds none.
reason: uint8 per output pixel, one of
    GUIDED      gw >= 0.01: the guided value
    REJ_ID      no tap was accepted, and every tap inside the image failed the id test
    REJ_NORMAL  no tap was accepted, some passed the id test, and every one of those failed the normal test
    REJ_DEPTH   no tap was accepted, some passed the id and the normal test (and so failed the depth test)
    LOW_WEIGHT  some tap was accepted, but gw < 0.01
(every reason but GUIDED takes the plain bilinear value). outside: bool per output pixel, some tap
of the four lay outside the low-resolution image.

Vectorised over pixels, one numpy operation per contract operation; every scalar is an np.float32 and
every array float32. A skipped tap is computed at a clamped position and masked out.
"""
import numpy as np

F = np.float32
GUIDED, REJ_ID, REJ_NORMAL, REJ_DEPTH, LOW_WEIGHT = range(5)
REASONS = {GUIDED: "guided", REJ_ID: "all taps rejected by id", REJ_NORMAL: "all taps rejected by normal",
           REJ_DEPTH: "all taps rejected by depth", LOW_WEIGHT: "weight below 0.01"}


def _f32(a):
    a = np.asarray(a)
    assert a.dtype == np.float32
    return a


def positions(w, h, lw, lh):
    """Step 1: (tx, ix) of every column and (ty, iy) of every row."""
    px = ((np.arange(w, dtype=F) + F(0.5)) / F(w)) * F(lw) - F(0.5)
    py = ((np.arange(h, dtype=F) + F(0.5)) / F(h)) * F(lh) - F(0.5)
    assert px.dtype == F and py.dtype == F
    fx, fy = np.floor(px), np.floor(py)
    return px - fx, fx.astype(np.int64), py - fy, fy.astype(np.int64)


def upsample(lo, guides, params):
    l_color, l_normal, l_depth = _f32(lo["color"]), _f32(lo["normal"]), _f32(lo["depth"])
    l_id = np.asarray(lo["sphere_id"])
    l_var = _f32(lo["variance"]) if lo.get("variance") is not None else None
    normal, depth, alpha = _f32(guides["normal"]), _f32(guides["depth"]), _f32(guides["alpha"])
    sid = np.asarray(guides["sphere_id"])
    assert l_id.dtype == np.uint32 and sid.dtype == np.uint32
    lh, lw = l_depth.shape
    h, w = depth.shape
    normal_tol, depth_tol = F(params.normal_tol), F(params.depth_tol)

    tx, ix, ty, iy = positions(w, h, lw, lh)
    assert ix.min() >= -1 and ix.max() <= lw - 1 and iy.min() >= -1 and iy.max() <= lh - 1
    tx, ix = np.broadcast_to(tx[None, :], (h, w)), np.broadcast_to(ix[None, :], (h, w))
    ty, iy = np.broadcast_to(ty[:, None], (h, w)), np.broadcast_to(iy[:, None], (h, w))
    surface = alpha == F(1)
    ztol = depth_tol * depth

    zeros = lambda: np.zeros((h, w), dtype=F)  # noqa: E731
    pw, pv, gw, gv = zeros(), zeros(), zeros(), zeros()
    ps, gs = np.zeros((h, w, 3), dtype=F), np.zeros((h, w, 3), dtype=F)
    outside = np.zeros((h, w), dtype=bool)
    any_id, any_normal, any_ok = (np.zeros((h, w), dtype=bool) for _ in range(3))
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = ix + i, iy + j
            inside = (qx >= 0) & (qx < lw) & (qy >= 0) & (qy < lh)
            outside |= ~inside
            cx, cy = np.clip(qx, 0, lw - 1), np.clip(qy, 0, lh - 1)
            wgt = (tx if i else F(1) - tx) * (ty if j else F(1) - ty)
            wc = wgt[..., None] * l_color[cy, cx]
            wv = (wgt * wgt) * l_var[cy, cx] if l_var is not None else zeros()
            assert wgt.dtype == F and wc.dtype == F and wv.dtype == F
            pw = np.where(inside, pw + wgt, pw)
            ps = np.where(inside[..., None], ps + wc, ps)
            pv = np.where(inside, pv + wv, pv)
            id_ok = inside & (l_id[cy, cx] == sid)
            dn = l_normal[cy, cx] - normal
            d2 = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
            assert d2.dtype == F
            with np.errstate(invalid="ignore"):
                n_ok = id_ok & ~(surface & (d2 > normal_tol))
                ok = n_ok & ~(surface & (np.abs(l_depth[cy, cx] - depth) > ztol))
            any_id |= id_ok
            any_normal |= n_ok
            any_ok |= ok
            gw = np.where(ok, gw + wgt, gw)
            gs = np.where(ok[..., None], gs + wc, gs)
            gv = np.where(ok, gv + wv, gv)
    assert (pw >= F(0.25)).all()
    guided = gw >= F(0.01)
    with np.errstate(all="ignore"):
        g_color, g_var = gs / gw[..., None], gv / (gw * gw)
    p_color, p_var = ps / pw[..., None], pv / (pw * pw)
    color = np.where(guided[..., None], g_color, p_color)
    variance = np.where(guided, g_var, p_var) if l_var is not None else None
    assert color.dtype == F and (variance is None or variance.dtype == F)
    reason = np.full((h, w), GUIDED, dtype=np.uint8)
    reason[~guided & any_ok] = LOW_WEIGHT
    reason[~any_ok & any_normal] = REJ_DEPTH
    reason[~any_normal & any_id] = REJ_NORMAL
    reason[~any_id] = REJ_ID
    return color, variance, reason, outside
