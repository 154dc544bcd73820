"""TEST INFRASTRUCTURE: synthetic planes for the guided upsample (rt_upsample_*),
shared by the CPU and the GPU module.

    lo, guides = upsample_cases.planes(lw, lh, w, h)

lo: color, variance, normal, depth, sphere_id of lw x lh; guides: normal, depth, alpha, sphere_id of
w x h. numpy, fixed seed. The low-resolution guides are constant over blocks (ids from a few values
and 0xffffffff, vertical and horizontal neighbours differing; normals from the six axis directions;
depths in two layers, 2 and 5, with a jitter of 1 %). An output pixel takes the guides of the
low-resolution pixel nearest to its position, so its nearest tap passes every test, except in
three rectangles in the image's upper third, which are there so that every way of falling back occurs:
    A  an id no low-resolution pixel has                                (all taps rejected by id)
    B  alpha 1, the opposite normal (d2 = 4)                            (... by normal)
    C  alpha 1, the other depth layer                                   (... by depth)
and on part of every output row whose position falls on a low-resolution row exactly (ty = 0: the
two taps of the row below have weight 0): there the pixel takes that row's id and alpha 0, so that
where the two rows' ids differ only taps of weight 0 are accepted (weight below 0.01). Elsewhere alpha
is 1, 0 or 0.5 over 4 x 4 blocks.
"""
import numpy as np

import upsample_ref

F = np.float32
IDS = np.array([0, 1, 2, 3, 0xffffffff], dtype=np.uint32)
NO_SUCH_ID = np.uint32(9)
AXES = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=F)
LAYERS = (F(2), F(5))


def _blocks(g, h, w, bh, bw, values):
    """An (h, w) plane of indices into `values`, constant over bh x bw blocks, drawn at random."""
    nby, nbx = (h + bh - 1) // bh, (w + bw - 1) // bw
    return g.integers(0, values, (nby, nbx))[np.arange(h)[:, None] // bh, np.arange(w)[None, :] // bw]


def planes(lw, lh, w, h, seed=11):
    g = np.random.default_rng(seed)
    by, bx = np.arange(lh)[:, None] // 5, np.arange(lw)[None, :] // 6
    l_id = IDS[(bx + 2 * by) % 5]
    l_normal = AXES[_blocks(g, lh, lw, 4, 7, 6)]
    layer = _blocks(g, lh, lw, 6, 9, 2)
    l_depth = (np.where(layer == 0, LAYERS[0], LAYERS[1]) * (F(1) + F(0.01) * g.random((lh, lw), dtype=F))).astype(F)
    lo = dict(color=(g.random((lh, lw, 3), dtype=F) * F(4)).astype(F), variance=(g.random((lh, lw), dtype=F) * F(0.05)).astype(F),
              normal=np.ascontiguousarray(l_normal), depth=l_depth, sphere_id=np.ascontiguousarray(l_id))

    tx, ix, ty, iy = upsample_ref.positions(w, h, lw, lh)
    nx = np.clip(ix + (tx >= F(0.5)), 0, lw - 1)[None, :]   # the low-resolution pixel nearest to the position
    ny = np.clip(iy + (ty >= F(0.5)), 0, lh - 1)[:, None]
    sid, normal = l_id[ny, nx].copy(), l_normal[ny, nx].copy()
    depth = (l_depth[ny, nx] * (F(1) + F(0.01) * g.random((h, w), dtype=F))).astype(F)
    alpha = np.array([1, 1, 1, 0, 0.5], dtype=F)[_blocks(g, h, w, 4, 4, 5)]
    top = slice(0, max(1, h // 3))
    a, b, c = (slice(k * w // 7, max(k * w // 7 + 1, (k + 2) * w // 7)) for k in (0, 2, 5))
    sid[top, a] = NO_SUCH_ID
    alpha[top, b] = F(1)
    normal[top, b] = -normal[top, b]
    alpha[top, c] = F(1)
    depth[top, c] = np.where(depth[top, c] < F(3.5), LAYERS[1], LAYERS[0])
    for y in np.nonzero((ty == 0) & (iy >= 0) & (iy + 1 < lh) & (np.arange(h) >= h // 3))[0]:
        right = slice(w // 2, w)
        sid[y, right] = l_id[iy[y] + 1, nx[0, right]]
        alpha[y, right] = F(0)
    guides = dict(normal=np.ascontiguousarray(normal), depth=depth, alpha=alpha, sphere_id=sid)
    for d in (lo, guides):
        for arr in d.values():
            arr.setflags(write=False)
    return lo, guides
