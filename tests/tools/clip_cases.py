"""TEST INFRASTRUCTURE: the synthetic planes of the history clamp's tests (rt_temporal_clip*, DESIGN.md
§4.17), shared by the CPU module (which checks that the cases say something) and the GPU module (which
compares the library with temporal_clip_ref bit for bit on them).

    cur, prev, cam, prev_cam = clip_cases.planes(w, h)
    now, was = clip_cases.tables()                      # the motion case's two sphere tables
    par = clip_cases.params(w, h)
    clip = clip_cases.clip(radius)

The sizes are chosen where the staging of a 64 x 4 workgroup's tile can fail: 5 x 3 is smaller than a
radius-2 window and a single partial workgroup, 70 x 37 has a partial column of workgroups and a ragged
last row, 129 x 9 has one lane in a third workgroup column.

Planes: random colours, so that a window's box is about 0.5 +- 0.29 gamma per channel; the history's
colours are drawn from [0.1, 0.9], which with GAMMA = 1 leaves a good part of the resampled colours
outside the box and a good part inside (both modules assert more than a tenth of each, at every size).
At 5 x 3 only 13 or 14 pixels have history and that range leaves 3 of them unchanged, one more than the
tenth asks for: there the history is drawn from [0.35, 0.65] (HISTORY_RANGE), which leaves 4 to 6
unchanged and 7 to 10 changed at the three radii. Ids lie in
blocks whose borders run at x = 20|21, 61|62, 66|67, 100|101 and y = 1|2, 5|6, 17|18, 30|31: they cross
the workgroup borders at x = 63|64 and y = 3|4, ..., so that windows on both sides of a tile edge hold
skipped taps, and one pixel in ten carries another id (9, which the motion case's tables of 8 rows do
not hold). One block of the beauty plane is flat (s2 = 0: the box is a point; 4 x 9 pixels, but a single
pixel at 5 x 3, where it would otherwise be half the image). The two cameras differ by
a small move, the surface depth is nearly constant, so most pixels find their history.
"""
import functools

import numpy as np

import raytracinginoneweekend_amd as rt
from support import STILL, shifted_camera

F = np.float32
SIZES = ((5, 3), (70, 37), (129, 9))
RADII = (1, 2, 3)
GAMMA = 1.0
HISTORY_RANGE = {None: (0.1, 0.9), (5, 3): (0.35, 0.65)}  # the history's colours, by size (None: every other)
N_SPHERES = 8
MOVE = ((0.1, 0.05, -0.05), (0.15, 0.05, 0.0))
X_BORDERS, Y_BORDERS = (21, 62, 67, 101), (2, 6, 18, 31)


def camera(w, h, shift=STILL):
    return shifted_camera(w, h, rt.CORRECTED, shift)


def _ids(w, h, g):
    ys, xs = np.mgrid[0:h, 0:w]
    block = np.searchsorted(X_BORDERS, xs, side="right") + np.searchsorted(Y_BORDERS, ys, side="right")
    ids = (block % 7).astype(np.uint32)
    ids[g.random((h, w)) < 0.1] = 9
    return ids


@functools.lru_cache(maxsize=None)
def planes(w, h):
    """(cur, prev, camera, prev_camera) of a size, once; the arrays are read-only."""
    g = np.random.default_rng(100 * w + h)
    up = np.zeros((h, w, 3), dtype=F)
    up[..., 1] = 1

    def guides():
        alpha = np.ones((h, w), dtype=F)
        alpha[g.random((h, w)) < 0.03] = F(0.5)                    # edge pixels: no history
        sky = np.zeros((h, w), dtype=bool)
        sky[:, w - max(1, w // 8):] = True                         # a band of sky at the right
        normal, depth, ids = up.copy(), (F(6) * (F(1) + F(0.01) * g.random((h, w), dtype=F))).astype(F), _ids(w, h, g)
        normal[g.random((h, w)) < 0.05] = (1, 0, 0)                # another normal: taps rejected
        normal[sky], depth[sky], ids[sky] = 0, 0, 0xffffffff
        alpha[sky & (alpha == 1)] = 0
        return alpha, dict(normal=normal, depth=depth, sphere_id=ids)

    alpha, gc = guides()
    _, gp = guides()
    beauty = g.random((h, w, 3), dtype=F)
    fh, fw = min(4, max(1, h // 2)), min(9, max(1, w // 3))           # 4 x 9 but at 5 x 3, where it is one pixel
    beauty[h // 2:h // 2 + fh, w // 3:w // 3 + fw] = (0.25, 0.5, 0.75)  # a flat block
    cur = dict(beauty=beauty, variance=g.random((h, w), dtype=F) * F(0.02), alpha=alpha, **gc)
    lo, hi = HISTORY_RANGE.get((w, h), HISTORY_RANGE[None])
    prev = dict(color=(g.random((h, w, 3), dtype=F) * F(hi - lo) + F(lo)).astype(F),
                variance=g.random((h, w), dtype=F) * F(0.02), history=g.integers(1, 40, (h, w)).astype(F), **gp)
    for a in list(cur.values()) + list(prev.values()):
        a.setflags(write=False)
    return cur, prev, camera(w, h, MOVE), camera(w, h)


def tables():
    """Eight spheres that moved a little; sphere 3 also changed its radius (it restarts)."""
    g = np.random.default_rng(11)
    now = np.empty((N_SPHERES, 4), dtype=F)
    now[:, :3] = g.normal(size=(N_SPHERES, 3)) * 0.05
    now[:, 3] = 0.5
    was = now.copy()
    was[:, :3] += (g.normal(size=(N_SPHERES, 3)) * 0.02).astype(F)
    was[3, 3] = 0.6
    return now, was


def params(w, h):
    return rt.temporal_params(w, h, alpha_min=0.2, max_history=32.0, normal_tol=0.1, depth_tol=0.1)


def clip(radius, gamma=GAMMA):
    return rt.temporal_clip(radius=radius, gamma=gamma)
