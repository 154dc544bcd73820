"""The dealing order of a pass (rt_tile_order): its 64-pixel blocks as a
permutation, lead tiles first, and the tiles proven to send every primary ray to the sky last.

The sky proof is what lets those samples skip the closest-hit test, so it is checked against
the reference's own closest hit (the CPU restatement, oracle_kat_hit = raytracer.hxx:94-118
brute force over every sphere): rays of every sky tile at the corners of its pixel range, with
the jitter at both ends of [0, 1), the lens offset at its extremes and at random points, built
in binary32 the way camera.hxx:46-57 builds them, must meet no sphere. Cameras: the reference's
(as shipped and corrected), row shares, and adversarial ones whose rays graze the ground and
the scene's spheres at the horizon. No GPU.
"""
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
from tile_checks import _check, _hits, _rays, _sky_rays  # noqa: E402,F401


def test_reference_camera_config3_sky_tiles_meet_nothing():
    s, m = rt.huge_scene_arrays(1234)
    perm, n_lead, n_sky = _check(s, m, rt.Camera.default(1280, 720), 1280, 720, min_sky=10000)
    # the oracle's own classification (profiles/r06/deep_sources.txt): 10 567 tiles whose primaries
    # all reached the sky at 16 spp; the proof is conservative
    assert n_sky <= 10567 and n_lead >= 161


def test_row_shares_and_corrected_camera():
    s, m = rt.huge_scene_arrays(1234)
    for r, n in ((0, 8), (5, 8), (1, 2)):
        _check(s, m, rt.Camera.default(1280, 720), 1280, 720, row_offset=r, row_stride=n, min_sky=100)
    _check(s, m, rt.Camera.default(640, 360, rt.CORRECTED), 640, 360, min_sky=100)


@pytest.mark.parametrize("case", range(6))
def test_adversarial_cameras(case):
    """Cameras near the ground and among the spheres, looking at the horizon, up, and down: rays
    that graze the ground or pass just over a sphere must not be taken for sky."""
    s, m = rt.huge_scene_arrays(1234)
    rng = np.random.default_rng(100 + case)
    W, H = 320, 176
    pos = [(-4, 0.35, 5), (0, 0.05, 0), (6, 1.2, -3), (-11, 0.25, -11), (3, 2.5, 3), (0.5, 0.41, 0.7)][case]
    look = (float(rng.uniform(-8, 8)), float(rng.uniform(-0.5, 1.5)), float(rng.uniform(-8, 8)))
    cam = rt.Camera(pos, look, (0, 1, 0), W / H, float(rng.uniform(20, 90)), float(rng.uniform(0, 0.3)),
                    float(rng.uniform(0.5, 12)), rt.CORRECTED if case % 2 else rt.REFERENCE)
    _check(s, m, cam, W, H, min_sky=0)


def test_natural_order_without_whole_blocks():
    s, m = rt.huge_scene_arrays(1234)
    perm, n_lead, n_sky = rt.tile_order((s, m), rt.make_params(200, 100, 1), rt.Camera.default(200, 100))
    assert len(perm) == 0 and n_lead == 0 and n_sky == 0  # 20 000 pixels: not whole blocks of 64
