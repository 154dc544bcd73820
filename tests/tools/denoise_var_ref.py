"""TEST INFRASTRUCTURE: CPU restatement of the variance-guided à-trous filter's contract
(include/rt_api.h, rt_denoise_var_buffers) in numpy float32, written from the
contract and not from the kernel.

    out, vout, census = denoise_var_ref.denoise(beauty, variance, albedo=None, normal=None, depth=None,
                                                levels=1, sigma_color=0, sigma_normal=0, sigma_depth=0,
                                                sigma_albedo=0, var_floor=1e-4)

Vectorised over pixels; a Python loop over the levels, the 9 prefilter taps and the 25 filter taps in
the contract's order (j outer, i inner); a skipped tap leaves the sums as they are. Every scalar is
an np.float32 and every array float32. vout is V after the last level. census = (zero, between,
one) of the total edge weight over all in-image non-centre taps of all levels, as denoise_ref's.
"""
import numpy as np

from denoise_ref import F, H3, _dist2, _edge, _f32, _r, _shift


def params_kwargs(p, v):
    """The keyword arguments of denoise() for an rt_denoise_params and an rt_denoise_var_buffers record."""
    return dict(levels=p.levels, sigma_color=p.sigma_color, sigma_normal=p.sigma_normal, sigma_depth=p.sigma_depth,
                sigma_albedo=p.sigma_albedo, var_floor=v.var_floor)


def prefilter(v):
    """g of the contract: the 3x3 kernel {1/4, 1/8, 1/16} over V at clamped coordinates, spacing 1."""
    h, w = v.shape
    g = np.zeros((h, w), dtype=F)
    for j in (-1, 0, 1):
        ys = np.clip(np.arange(h) + j, 0, h - 1)
        for i in (-1, 0, 1):
            xs = np.clip(np.arange(w) + i, 0, w - 1)
            k = F(0.25) if (i == 0 and j == 0) else F(0.125) if (i == 0 or j == 0) else F(0.0625)
            g = g + k * v[ys][:, xs]
    assert g.dtype == np.float32
    return g


def denoise(beauty, variance, albedo=None, normal=None, depth=None, levels=1, sigma_color=0.0, sigma_normal=0.0,
            sigma_depth=0.0, sigma_albedo=0.0, var_floor=1e-4):
    c = _f32(beauty)
    v = _f32(variance)
    albedo = None if albedo is None else _f32(albedo)
    normal = None if normal is None else _f32(normal)
    depth = None if depth is None else _f32(depth)
    assert 1 <= levels <= 6 and v.shape == c.shape[:2]
    on_color = F(sigma_color) != 0
    on_albedo = albedo is not None and F(sigma_albedo) != 0
    r_n = _r(sigma_normal) if normal is not None else None
    r_z = _r(sigma_depth) if depth is not None else None
    r_a = _r(sigma_albedo) if on_albedo else None
    sc2 = F(sigma_color) * F(sigma_color)
    floor = F(var_floor)
    zero = between = one = 0
    for level in range(levels):
        s = 1 << level
        r_c = F(1) / (sc2 * prefilter(v) + floor) if on_color else None   # per pixel p, no 2^-l factor
        sumw = np.zeros(c.shape[:2], dtype=F)
        sumv = np.zeros(c.shape[:2], dtype=F)
        acc = np.zeros(c.shape, dtype=F)
        for j in range(-2, 3):
            for i in range(-2, 3):
                cq, inside = _shift(c, i * s, j * s)
                vq = _shift(v, i * s, j * s)[0]
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
                sumv = np.where(inside, sumv + (w * w) * vq, sumv)
                acc = np.where(inside[..., None], acc + w[..., None] * cq, acc)
                if i or j:
                    zero += int(np.count_nonzero(inside & (total == 0)))
                    one += int(np.count_nonzero(inside & (total == 1)))
                    between += int(np.count_nonzero(inside & (total > 0) & (total < 1)))
        c = acc / sumw[..., None]
        v = sumv / (sumw * sumw)
        assert c.dtype == F and v.dtype == F
    return c, v, (zero, between, one)
