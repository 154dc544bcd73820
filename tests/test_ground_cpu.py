"""The ground class of a pass (rt_tile_ground) on the CPU: its proof, its counts,
the rules that keep a pass out of it, and its place in the dealing order.

The proof (tests/tools/ground_checks.py): for every ground tile, corner rays (the jitter at both
ends, the lens at its extremes) and random rays get no candidate from any clustered sphere under
the CPU restatement's brute-force hit, as tests/tools/tile_checks.py does for the sky tiles. The
order: rt_tile_order's permutation is what it was; the ground blocks are its positions
[n_lead, n_lead + n_ground), tiles in ascending order, and every untiled block follows them. The
device's classification runs the same rt_tiles.h functions and the same stable partition
(tests/test_tile_device_gpu.py compares the two entry for entry), so the range is the same there;
tests/test_ground_gpu.py renders through it.

The cases of tests/test_ground_edges_gpu.py are what they claim to be: each list of
ground_checks.LIST_CASES has its size, takes the class or not as the table says, shows every listed
sphere as the first hit of samples inside ground tiles (tests/tools/aov_ref's per-sample ids) and
has ground samples of three segments and more (they are redone) beside ground samples that reach the
sky (they are not); the grown sphere lengthens the list by one; the constants the sample counts and
the frame counts straddle are the source's.
"""
import functools
import os
import re
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import camera_cases as CC  # noqa: E402
import golden_io as G  # noqa: E402
import ground_checks as GC  # noqa: E402

W3, H3 = 1280, 720  # config 3


def huge():
    return G.scene("huge")


@pytest.mark.parametrize("mode", [rt.REFERENCE, rt.CORRECTED], ids=["reference", "corrected"])
def test_config3_frame(mode):
    s, m = huge()
    n_ground, n_mid = GC.check(s, m, rt.Camera.default(W3, H3, mode), W3, H3)
    print(f"config 3, camera mode {mode}: {n_ground} ground tiles of {W3 * H3 // 64}")
    assert n_ground == n_mid > 0  # every row is tiled: the whole middle class
    if mode == rt.REFERENCE:
        assert n_ground == 1912


@pytest.mark.parametrize("world", [2, 8])
def test_config3_row_shares(world):
    """Rank 1's rows of an N-way share. The 8-way share's 90 rows leave two untiled rows: of the
    412 blocks of its middle class 40 are untiled and stay in the main launch."""
    s, m = huge()
    cam = rt.Camera.default(W3, H3)
    for rank in (0, world - 1):
        n_ground, n_mid = GC.check(s, m, cam, W3, H3, row_offset=rank, row_stride=world)
        print(f"{world}-way share, rank {rank}: {n_ground} ground tiles, {n_mid} blocks in the middle class")
        assert n_ground > 0
        if world == 8:
            assert n_mid - n_ground == 2 * W3 // 64
            if rank == 0:
                assert (n_mid, n_ground) == (412, 372)
        else:
            assert n_mid == n_ground


def test_small_frames_are_not_vacuous():
    s, m = huge()
    assert GC.check(s, m, rt.Camera.default(128, 72), 128, 72)[0] == 20
    assert GC.check(s, m, rt.Camera.default(128, 72, rt.CORRECTED), 128, 72)[0] == 15
    assert GC.check(s, m, rt.Camera.default(64, 40), 64, 40)[0] == 4
    n_ground, n_mid = GC.check(s, m, GC.redo_camera(128 / 72), 128, 72)
    assert n_ground == n_mid == 85


@pytest.mark.parametrize("name", CC.NAMES)
def test_adversarial_cameras(name):
    """Every 64x40 case of tests/tools/camera_cases.py: whatever ground tiles it has are proven."""
    c = CC.case(name)
    n_ground, n_mid = GC.check(c.spheres, c.materials, c.camera, c.W, c.H, c.row_offset, c.row_stride, depth=c.depth)
    print(f"{name}: {n_ground} ground tiles, {n_mid} blocks in the middle class")


def test_some_adversarial_camera_has_ground_tiles():
    with_ground = [n for n in CC.NAMES
                   if rt.tile_ground(CC.scene(n), CC.params(n), CC.case(n).camera) > 0]
    print("cases with ground tiles:", with_ground)
    assert len(with_ground) >= 3


def test_pass_rules(opts):
    s, m = huge()
    cam = rt.Camera.default(128, 72)
    p = rt.make_params(128, 72, 4, 64, 1234)
    assert rt.tile_ground((s, m), p, cam) == 20
    assert rt.tile_ground((s, m), rt.make_params(128, 72, 4, 2, 1234), cam) == 20
    # a metal ground, max_depth 0 and 1, and the flags of the kernels without tile classes
    assert rt.tile_ground(GC.metal_ground(s, m), p, cam) == 0
    for depth in (0, 1):
        assert rt.tile_ground((s, m), rt.make_params(128, 72, 4, depth, 1234), cam) == 0
    for flag in ("brute_force", "scalar_scene", "wavefront", "cuda_compat"):
        assert rt.tile_ground((s, m), rt.make_params(128, 72, 4, 64, 1234, **{flag: True}), cam) == 0
    # a width that is no multiple of 8 has no tiles; the simple scene has no clusters
    assert rt.tile_ground((s, m), rt.make_params(100, 64, 4, 64, 1234), rt.Camera.default(100, 64)) == 0
    assert rt.tile_ground(G.scene("simple"), p, cam) == 0
    # the options that take the sky kernel or the root gate away
    for name in ("no_sky", "natural_order", "no_root_box", "pairs"):
        opts.set(**{name: True})
        assert rt.tile_ground((s, m), p, cam) == 0, name
        opts.clear(name)
    assert rt.tile_ground((s, m), p, cam) == 20


def test_order_is_unchanged_by_the_class():
    """rt_tile_order's signature and meaning: a permutation, lead blocks first, sky blocks last, the
    middle class in ascending order (its tiles, i.e. the ground range, before its untiled blocks)."""
    s, m = huge()
    p = rt.make_params(64, 36, 4, 64, 1234)  # four tile rows and four untiled rows
    perm, n_lead, n_sky = rt.tile_order((s, m), p, rt.Camera.default(64, 36))
    n_ground = rt.tile_ground((s, m), p, rt.Camera.default(64, 36))
    mid = perm[n_lead:len(perm) - n_sky]
    assert sorted(perm.tolist()) == list(range(36)) and (np.diff(mid.astype(np.int64)) > 0).all()
    assert (n_ground, len(mid)) == (4, 8)
    assert (mid[:n_ground] < 32).all() and mid[n_ground:].tolist() == [32, 33, 34, 35]


# ---- the cases of tests/test_ground_edges_gpu.py ---------------------------------------------------
EDGE = dict(W=128, H=72, spp=5)


@functools.lru_cache(maxsize=None)
def edge_census(which, camera="reference", spp=EDGE["spp"]):
    """(ground tiles, {sphere: samples of ground-tile pixels whose first hit it is}, sky samples of
    those pixels, segments past the second of ground samples in tile rows without lead blocks)."""
    s, m = huge()
    W, H = EDGE["W"], EDGE["H"]
    scene = {"huge": lambda: (s, m), "grown": lambda: GC.grown(s, m)[:2]}.get(which, lambda: GC.list_case(s, m, which))()
    cam = {"reference": rt.Camera.default(W, H), "redo": GC.redo_camera(W / H)}[camera]
    p = rt.make_params(W, H, spp, 64, 1234)
    n_ground = rt.tile_ground(scene, p, cam)
    if not n_ground:
        return 0, {}, 0, 0
    hits, sky = GC.first_hits_in_ground_tiles(scene, p, cam)
    return n_ground, hits, sky, GC.long_paths_in_ground_rows(scene, p, cam)


@pytest.mark.parametrize("name", list(GC.LIST_CASES))
def test_list_cases_reach_the_list(name):
    s, m = huge()
    n, kw, takes = GC.LIST_CASES[name]
    s2, m2 = GC.list_case(s, m, name)
    _, always = GC.clustered(s2)
    listed = np.flatnonzero(always)
    assert len(listed) == n and len(s2) == len(s) + n - 1
    # the appended balls have materials, and albedos, of their own
    own = m2[s2["material"][listed]]
    assert len({tuple(a) for a in own["albedo"].tolist()}) == n and len(set(s2["material"][listed].tolist())) == n
    cam = rt.Camera.default(EDGE["W"], EDGE["H"])
    n_ground, hits, sky, long_paths = edge_census(name)
    print(f"{name}: {n_ground} ground tiles, first hits {hits}, {sky} sky samples, {long_paths} segments past the second")
    if not takes:
        assert n_ground == 0
        if name == "nan_centre":
            # ground_scene_ok admits the list, but no tile is proven sky beside a non-finite sphere:
            # no sky kernel, so no class
            assert rt.tile_order((s2, m2), rt.make_params(EDGE["W"], EDGE["H"], 4, 64, 1234), cam)[2] == 0
            assert (m2["kind"][s2["material"][listed]] == rt.abi.RT_LAMBERT).all()
            assert not np.isfinite(s2["center"][listed[-1]]).all()
        return
    assert GC.check(s2, m2, cam, EDGE["W"], EDGE["H"])[0] == n_ground > 0
    # every listed sphere is the first hit of samples inside ground tiles, and nothing else is
    assert sorted(hits) == listed.tolist(), (hits, listed)
    assert min(hits.values()) >= 64  # a pixel's worth and more each
    # some ground samples are redone (three segments and more), some are not (they reach the sky)
    assert long_paths > 0 and sky > 0
    if kw.get("negative_radius"):
        assert s2["radius"][listed[-1]] < 0


def test_list_cases_cover_the_sizes():
    sizes = sorted(n for n, _, takes in GC.LIST_CASES.values() if takes)
    assert sizes == [2, 3, 4, 5, 8]
    assert GC.LIST_CASES["n9"][0] == 9 and not GC.LIST_CASES["n9"][2]


def test_grown_sphere_lengthens_the_list():
    s, m = huge()
    s2, m2, i = GC.grown(s, m)
    assert len(s2) == len(s) and m2 is m
    assert int(GC.clustered(s)[1].sum()) == 1 and int(GC.clustered(s2)[1].sum()) == 2 and GC.clustered(s2)[1][i]
    assert m["kind"][s["material"][i]] == rt.abi.RT_LAMBERT
    n_ground, hits, sky, long_paths = edge_census("grown")
    print(f"grown: sphere {i}, {n_ground} ground tiles, first hits {hits}, {long_paths} segments past the second")
    assert n_ground == 57 and sorted(hits) == np.flatnonzero(GC.clustered(s2)[1]).tolist()
    assert long_paths > 0 and sky > 0


@pytest.mark.parametrize("spp", [1, 5])
def test_redo_camera_redoes_some_samples(spp):
    """The redo camera's bottom tile rows are ground tiles alone, and some of their paths have three
    segments and more, at 1 spp (the count ring's frame) as at 5."""
    n_ground, hits, sky, long_paths = edge_census("huge", "redo", spp)
    assert n_ground == 85 and long_paths > 0 and sky > 0 and list(hits) == [1]


def test_constants_the_edge_cases_straddle():
    """31 / 32 / 64 / 65 samples straddle RT_GROUND_SPT, lists of 8 and 9 kGroundAlways, frames 128,
    129, 256, 257 the half and the whole of rt_scene::kRing."""
    src = os.path.join(os.path.dirname(os.path.abspath(rt.__file__)), "csrc")
    host = open(os.path.join(src, "rt_host.cpp")).read()
    scene = open(os.path.join(src, "rt_scene.h")).read()
    ground = open(os.path.join(src, "rt_ground.hip")).read()
    assert re.search(r"#\s*define\s+RT_GROUND_SPT\s+32u?\b", host)
    assert re.search(r"\bkRing\s*=\s*256u?\b", scene)
    assert re.search(r"\bkGroundAlways\s*=\s*8u?\b", ground)
    assert re.search(r"#\s*define\s+RT_GROUND_RING\s+8u?\b", ground)
