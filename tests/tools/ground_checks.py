"""TEST INFRASTRUCTURE: the ground class of a pass (rt_tile_ground) against the
reference's own closest hit, shared by tests/test_ground_cpu.py and tests/test_ground_gpu.py.

A ground tile's proof is that no primary ray of the tile gets a candidate from a clustered sphere.
Rays of every ground tile at the corners of its pixel range, with the jitter at both ends of
[0, 1), the lens offset at its extremes and at random points (tile_checks.py builds them in
binary32 the way camera.hxx:46-57 does) are tested against the scene WITHOUT its always-tested
spheres by the CPU restatement's brute force (oracle_kat_hit = raytracer.hxx:94-118): none may
hit. No GPU.

The scenes of tests/test_ground_edges_gpu.py too (n_big and LIST_CASES: always-tested lists of up to
nine spheres; grown: a sphere of the scene grown into the list), with what tests/test_ground_cpu.py
needs to show that they reach the list: the first hits inside ground tiles, and the ground samples
of three segments and more (those the redo launch renders).
"""
import numpy as np

import raytracinginoneweekend_amd as rt

import tile_checks as TC

f32 = np.float32
UP = (0, 1, 0)


def clustered(s, cluster_size=16):
    """The spheres build_blob clusters (rt_host_build.cpp: the others, non-finite or with |r| above
    64 times the median, are tested on every segment), and the mask of the always-tested ones."""
    r = np.abs(s["radius"]).astype(f32)
    if len(s) < 2 * cluster_size:
        return s[:0], np.ones(len(s), bool)
    med = np.sort(r)[len(r) // 2]
    finite = np.isfinite(s["center"]).all(axis=1) & np.isfinite(r)
    always = ~finite | (r > f32(64) * med)
    return s[~always], always


def ground_range(scene, params, camera):
    """(perm, n_lead, n_sky, n_ground): the pass's order and its ground blocks perm[n_lead : n_lead + n_ground]."""
    perm, n_lead, n_sky = rt.tile_order(scene, params, camera)
    return perm, n_lead, n_sky, rt.tile_ground(scene, params, camera)


def check(s, m, cam, W, H, row_offset=0, row_stride=1, num_rows=0, depth=64):
    """The pass's ground blocks are tiles, in ascending order between the lead and the untiled
    blocks, and no ray of theirs meets a clustered sphere. Returns (n_ground, n_mid)."""
    p = rt.make_params(W, H, 4, depth, 1234, row_offset=row_offset, row_stride=row_stride, num_rows=num_rows)
    perm, n_lead, n_sky, n_ground = ground_range((s, m), p, cam)
    rows = num_rows or (H - row_offset + row_stride - 1) // row_stride
    n_tiles = (W // 8) * (rows // 8) if W % 8 == 0 else 0
    assert sorted(perm.tolist()) == list(range(len(perm)))  # a permutation of the blocks
    n_mid = len(perm) - n_lead - n_sky
    assert n_ground <= n_mid
    g = perm[n_lead:n_lead + n_ground]
    assert (g < n_tiles).all() and (np.diff(g.astype(np.int64)) > 0).all()
    if n_ground:
        # the blocks between the ground range and the sky tiles are the untiled ones, all of them
        rest = perm[n_lead + n_ground:len(perm) - n_sky]
        assert rest.tolist() == list(range(n_tiles, len(perm)))
        small, _ = clustered(s)
        c = cam.c if hasattr(cam, "c") else cam
        rays = TC._sky_rays(c, W, H, row_offset, row_stride, perm[:n_lead + n_ground], n_ground, np.random.default_rng(11))
        hit = TC._hits(np.ascontiguousarray(small), m, rays)
        assert not hit.any(), f"{int(hit.sum())} rays of ground tiles meet a clustered sphere"
    return n_ground, n_mid


def metal_ground(s, m):
    """The scene with its always-tested spheres re-pointed at an appended metal."""
    from raytracinginoneweekend_amd import _abi as abi
    _, always = clustered(s)
    m2 = np.concatenate([m, np.zeros(1, dtype=abi.MATERIAL_DTYPE)])
    m2[-1] = (abi.RT_METAL, (0.8, 0.8, 0.8), 0.1)
    s2 = s.copy()
    s2["material"][always] = len(m2) - 1
    return s2, m2


def two_big(s, m):
    """The scene with a second always-tested sphere: a lambert ball of radius 40 on the horizon
    behind the field, which the default camera sees above part of the ground."""
    from raytracinginoneweekend_amd import _abi as abi
    s2 = np.concatenate([s, np.zeros(1, dtype=s.dtype)])
    s2[-1] = ((0.0, 30.0, -120.0), 40.0, int(np.flatnonzero(m["kind"] == abi.RT_LAMBERT)[1]))
    assert int(clustered(s2)[1].sum()) == 2
    return s2, m


# n_big's balls: (pixel of the 128x72 frame under the default camera, radius). Each ball lies on that
# pixel's central ray at 18 radii from the camera, about 11 pixels across: two rows of four in the
# sky above the field, clear of each other, so that every one is the first hit of whole pixels of
# tiles whose beams meet no cluster. The radii differ (all above 64 times the huge scene's median
# radius 0.2), and the list is not sorted by distance.
BALLS = [((10, 8), 14.0), ((26, 8), 15.5), ((42, 8), 13.5), ((58, 8), 16.0),
         ((10, 24), 13.0), ((26, 24), 14.5), ((42, 24), 15.0), ((58, 24), 13.2)]


def ball(i):
    (x, y), r = BALLS[i]
    q = TC._rays(rt.Camera.default(128, 72).c, 128, 72, [x], [y], [0.5], [0.5], [(0, 0, 0)])[0].astype(np.float64)
    c = q[:3] + q[3:] / np.linalg.norm(q[3:]) * 18.0 * r
    return tuple(float(f32(v)) for v in c), r


def n_big(s, m, n, nan_centre=False, negative_radius=False, metal=None):
    """The scene with an always-tested list of n spheres: its own (the ground), then n - 1 appended
    lambert balls (BALLS) with |r| above 64 times the median radius, beyond the field, each with a
    lambert material of its own whose albedo no other material has: a shading record looked up
    under the wrong index changes the colours. nan_centre: the last ball's centre is not finite
    (build_blob lists it for that, and it never hits); negative_radius: the last ball's radius is
    negative (the normal (P - C) / r points inwards); metal = j: list member j (the ground is 0) is
    metal instead."""
    from raytracinginoneweekend_amd import _abi as abi
    k = n - int(clustered(s)[1].sum())
    assert 0 < k <= len(BALLS)
    s2 = np.concatenate([s, np.zeros(k, dtype=s.dtype)])
    m2 = np.concatenate([m, np.zeros(k, dtype=abi.MATERIAL_DTYPE)])
    for i in range(k):
        c, r = ball(i)
        m2[len(m) + i] = (abi.RT_LAMBERT, (0.15 + 0.1 * i, 0.9 - 0.1 * i, 0.3 + 0.05 * ((3 * i) % 8)), 0.0)
        s2[len(s) + i] = (c, r, len(m) + i)
    if nan_centre:
        s2["center"][-1, 0] = np.nan
    if negative_radius:
        s2["radius"][-1] = -s2["radius"][-1]
    if metal is not None:
        listed = np.flatnonzero(clustered(s2)[1])
        m2[s2["material"][listed[metal]]] = (abi.RT_METAL, (0.8, 0.8, 0.8), 0.1)
    assert int(clustered(s2)[1].sum()) == n
    return s2, m2


def ground_tile_mask(scene, params, camera):
    """(rows, W) bool: the pixels of the pass's ground tiles (8x8 tiles over the packed rows)."""
    from raytracinginoneweekend_amd import _abi as abi
    perm, n_lead, _, n_ground = ground_range(scene, params, camera)
    mask = np.zeros((abi.rows_of(params), params.width), bool)
    tiles_x = params.width // 8
    for b in perm[n_lead:n_lead + n_ground]:
        ty, tx = divmod(int(b), tiles_x)
        mask[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8] = True
    return mask


def first_hits_in_ground_tiles(scene, params, camera):
    """sphere index -> the samples of ground-tile pixels whose first hit it is (tests/tools/aov_ref's
    per-sample ids), and the number of samples of those pixels that reach the sky."""
    import aov_ref
    s, m = scene
    ids = aov_ref.render(s, m, camera, params, sample_ids=True)["sample_ids"]
    inside = ids[ground_tile_mask(scene, params, camera)]
    hit = inside[inside != 0xffffffff]
    idx, cnt = np.unique(hit, return_counts=True)
    return dict(zip(idx.tolist(), cnt.tolist())), int((inside == 0xffffffff).sum())


def long_paths_in_ground_rows(scene, params, camera, threads=8):
    """Segments beyond the second of the samples in the pass's tile rows that have no lead block and
    at least one ground tile: there every block is a sky tile (one segment per sample) or a ground
    tile, so a result above 0 is a ground sample of three or more segments, which the ground kernel
    cannot finish: it goes to the redo list. (Restatement's segments of those rows, minus one per
    sample, minus one per sample whose first hit is a sphere.)"""
    import aov_ref
    import oracle_binding as O
    from raytracinginoneweekend_amd import _abi as abi
    s, m = scene
    perm, n_lead, n_sky, n_ground = ground_range(scene, params, camera)
    tiles_x = params.width // 8
    lead_rows = {int(b) // tiles_x for b in perm[:n_lead]}
    ground_rows = {int(b) // tiles_x for b in perm[n_lead:n_lead + n_ground]}
    cam = camera.c if hasattr(camera, "c") else camera
    extra = 0
    for ty in sorted(ground_rows - lead_rows):
        p = abi.RtParams(params.width, params.height, params.spp, params.max_depth, params.seed,
                         params.row_offset + 8 * ty * params.row_stride, params.row_stride, 8, params.flags)
        _, seg = O.render_f32(s, m, cam, p, threads=threads)
        ids = aov_ref.render(s, m, cam, p, sample_ids=True)["sample_ids"]
        extra += int(seg) - ids.size - int((ids != 0xffffffff).sum())
    return extra


# The always-tested lists of tests/test_ground_edges_gpu.py (128x72, the default camera): name ->
# (n, n_big's keywords, whether the pass takes the ground class). A list of nine, and one with a
# metal member, keep the main launch (ground_scene_ok). So does a list with a non-finite sphere,
# though ground_scene_ok admits it: no beam is proven to miss such a sphere (rt_tiles.h
# sphere_missed: its interval arithmetic gives NaN, every comparison fails), so the pass has no
# sky tile, hence no sky kernel, which the class needs. tests/test_ground_cpu.py pins each.
LIST_CASES = {
    "n3": (3, {}, True), "n4": (4, {}, True), "n5": (5, {}, True), "n8": (8, {}, True),
    "n9": (9, {}, False),
    "nan_centre": (2, dict(nan_centre=True), False),
    "negative_radius": (2, dict(negative_radius=True), True),
    "metal_second": (3, dict(metal=1), False),
}


def list_case(s, m, name):
    n, kw, _ = LIST_CASES[name]
    return n_big(s, m, n, **kw)


GROWN_RADIUS = 13.0


def grown(s, m, cam_origin=(-4.0, 3.2, 5.0)):
    """The scene with one of its own lambert spheres grown past 64 times the median radius: the
    small lambert sphere at the field's (-x, -z) corner, which the default camera (well outside the
    grown ball) then sees above the field. The always-tested list goes from 1 to 2 with the sphere
    count fixed (an rt_scene_update); spheres of the corner now lie inside the ball."""
    from raytracinginoneweekend_amd import _abi as abi
    _, always = clustered(s)
    lambert = (m["kind"][s["material"]] == abi.RT_LAMBERT) & ~always
    c = s["center"].astype(np.float64)
    i = int(np.argmin(np.where(lambert, c[:, 0] + c[:, 2], np.inf)))
    assert np.linalg.norm(c[i] - np.array(cam_origin)) > GROWN_RADIUS + 1.0
    s2 = s.copy()
    s2["radius"][i] = GROWN_RADIUS
    assert int(clustered(s2)[1].sum()) == int(always.sum()) + 1
    return s2, m, i


def redo_camera(aspect):
    """From a corner of the huge scene's sphere field (|x|, |z| <= 11), half a unit above the
    ground, looking along the field's edge: the strip of ground a unit outside it, whose scattered
    rays that turn towards the field pass the box over it. At 128x72: 23 lead, 85 ground and 36 sky
    tiles (test_ground_cpu.py)."""
    return rt.Camera((12.3, 0.5, -12), (12.6, 0.0, 12), UP, aspect, 60.0, 0.05, 10.0, rt.CORRECTED)
