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
"""
import os
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
