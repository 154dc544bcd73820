"""TEST INFRASTRUCTURE: CPU restatement of the à-trous denoiser's contract (include/rt_api.h,
rt_denoise_params) in numpy float32, written from the contract and not from the kernels.

    out, census = denoise_ref.denoise(beauty, albedo=None, normal=None, depth=None, levels=1,
                                      sigma_color=0, sigma_normal=0, sigma_depth=0, sigma_albedo=0,
                                      demodulate=False)

Vectorised over pixels; a Python loop over the levels and the 25 taps in the contract's order (j
outer, i inner); a skipped tap leaves the sums as they are (np.where). Every scalar is an
np.float32 and every array float32, so no operation is promoted to float64 and each is rounded on
its own. census = (zero, between, one): over all in-image non-centre taps of all levels, how many
had a total edge weight (the product of the terms' edge values) of exactly 0, strictly between 0
and 1, and exactly 1.
"""
import numpy as np

F = np.float32
H3 = (F(0.375), F(0.25), F(0.0625))
FLOOR = F(0.0078125)


def _f32(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, a.dtype
    return a


def _shift(a, dx, dy):
    """b[y, x] = a[y + dy, x + dx] where that is inside the image (elsewhere: a's own value, never
    used), and the mask of the pixels where it is."""
    h, w = a.shape[:2]
    ys, xs = np.arange(h) + dy, np.arange(w) + dx
    inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
    b = a[np.clip(ys, 0, h - 1)][:, np.clip(xs, 0, w - 1)]
    return b, inside


def _edge(d2, r):
    m = np.maximum(F(0), F(1) - d2 * r)
    return m * m


def _dist2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _r(sigma):
    sigma = F(sigma)
    return F(1) / (sigma * sigma)


def params_kwargs(p):
    """The keyword arguments of denoise() for an rt_denoise_params record."""
    return dict(levels=p.levels, sigma_color=p.sigma_color, sigma_normal=p.sigma_normal, sigma_depth=p.sigma_depth,
                sigma_albedo=p.sigma_albedo, demodulate=bool(p.flags & 1))


def denoise(beauty, albedo=None, normal=None, depth=None, levels=1, sigma_color=0.0, sigma_normal=0.0,
            sigma_depth=0.0, sigma_albedo=0.0, demodulate=False):
    beauty = _f32(beauty)
    albedo = None if albedo is None else _f32(albedo)
    normal = None if normal is None else _f32(normal)
    depth = None if depth is None else _f32(depth)
    assert 1 <= levels <= 6
    on_color = F(sigma_color) != 0
    on_albedo = albedo is not None and F(sigma_albedo) != 0
    r_n = _r(sigma_normal) if normal is not None else None
    r_z = _r(sigma_depth) if depth is not None else None
    r_a = _r(sigma_albedo) if on_albedo else None
    if demodulate:
        assert albedo is not None
        a1 = np.maximum(albedo, FLOOR)
        c = beauty / a1
    else:
        c = beauty
    zero = between = one = 0
    for level in range(levels):
        s = 1 << level
        # sigma_color * 2^-level, exact
        r_c = _r(F(sigma_color) * F(2.0 ** -level)) if on_color else None
        sumw = np.zeros(c.shape[:2], dtype=F)
        acc = np.zeros(c.shape, dtype=F)
        for j in range(-2, 3):
            for i in range(-2, 3):
                cq, inside = _shift(c, i * s, j * s)
                k = H3[abs(i)] * H3[abs(j)]
                w = np.full(c.shape[:2], k, dtype=F)
                edges = []
                if on_color:
                    edges.append(_edge(_dist2(cq, c), r_c))
                if normal is not None:
                    edges.append(_edge(_dist2(_shift(normal, i * s, j * s)[0], normal), r_n))
                if depth is not None:
                    dz = _shift(depth, i * s, j * s)[0] - depth
                    edges.append(_edge(dz * dz, r_z))
                if on_albedo:
                    edges.append(_edge(_dist2(_shift(albedo, i * s, j * s)[0], albedo), r_a))
                total = np.ones(c.shape[:2], dtype=F)  # the census's own product, not part of the filter
                for e in edges:
                    w = w * e
                    total = total * e
                assert w.dtype == F
                sumw = np.where(inside, sumw + w, sumw)
                term = w[..., None] * cq
                acc = np.where(inside[..., None], acc + term, acc)
                if i or j:
                    zero += int(np.count_nonzero(inside & (total == 0)))
                    one += int(np.count_nonzero(inside & (total == 1)))
                    between += int(np.count_nonzero(inside & (total > 0) & (total < 1)))
        c = acc / sumw[..., None]
        assert c.dtype == F
    if demodulate:
        c = c * a1
    return c, (zero, between, one)
