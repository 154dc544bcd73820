"""TEST INFRASTRUCTURE: the ground class of a pass (rt_tile_ground) against the
reference's own closest hit, shared by tests/test_ground_cpu.py and tests/test_ground_gpu.py.

A ground tile's proof is that no primary ray of the tile gets a candidate from a clustered sphere.
Rays of every ground tile at the corners of its pixel range, with the jitter at both ends of
[0, 1), the lens offset at its extremes and at random points (tile_checks.py builds them in
binary32 the way camera.hxx:46-57 does) are tested against the scene WITHOUT its always-tested
spheres by the CPU restatement's brute force (oracle_kat_hit = raytracer.hxx:94-118): none may
hit. No GPU.
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


def redo_camera(aspect):
    """From a corner of the huge scene's sphere field (|x|, |z| <= 11), half a unit above the
    ground, looking along the field's edge: the strip of ground a unit outside it, whose scattered
    rays that turn towards the field pass the box over it. At 128x72: 23 lead, 85 ground and 36 sky
    tiles (test_ground_cpu.py)."""
    return rt.Camera((12.3, 0.5, -12), (12.6, 0.0, 12), UP, aspect, 60.0, 0.05, 10.0, rt.CORRECTED)
