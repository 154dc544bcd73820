"""The conditions that tests/test_gpu_cameras.py relies on, fixed from the reference alone
(tests/tools/camera_cases.py builds the cases; the CPU restatement renders them). No GPU.

* every case's frame is finite and not flat;
* the range census: which cases send part of their primaries outside a = |d|^2 in [2^-40, 2^40]
  while the host's camera_in_fast_range holds, so that the kernels' per-wave fallback from the
  short root forms (rt_trace.h ray_div) runs with KParams::fast_roots on;
* the material census: every extreme parameter of the `materials` case is hit by primaries;
* the sky proof of rt_tile_order under these cameras, and that enough cases reach the sky kernel.

Run with -s for the census numbers per case.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import camera_cases as CC  # noqa: E402
from tile_checks import _check  # noqa: E402

TILED = [n for n in CC.NAMES if n != "natural"]  # the 64 x 40 frames: whole 64-pixel blocks


@pytest.mark.parametrize("name", CC.NAMES)
def test_reference_frame_is_finite_and_not_flat(name):
    c = CC.case(name)
    for v in (*c.camera.origin, *c.camera.lower_left_corner, *c.camera.horizontal, *c.camera.vertical,
              c.camera.lens_radius):
        assert np.isfinite(v)
    img, seg = CC.beauty_ref(name)
    rows = len(range(c.row_offset, c.H, c.row_stride))
    assert img.shape == (rows, c.W, 3)
    distinct = len(np.unique(img.view(np.uint32)))
    print(f"{name}: {distinct} distinct values, {seg / (rows * c.W * c.spp):.2f} segments per primary, "
          f"range [{img.min():.3g}, {img.max():.3g}]")
    assert np.isfinite(img).all()
    assert distinct > 1000
    aov = CC.aov_reference(name)
    assert all(np.isfinite(aov[n]).all() for n in ("albedo", "normal", "depth", "alpha"))


@pytest.mark.parametrize("name", CC.NAMES)
def test_range_census(name):
    """Pixel-centre primaries in binary32 as camera_ray forms d: the range cases have between 10%
    and 90% of them outside [2^-40, 2^40] under a camera the host takes for in range (measured:
    tiny, tiny_lens and tiny_sky 49.4% below 2^-40; wide and wide_lens 37.0%, wide_sky 29.1% above
    2^40); `subnormal` and `subnormal_sky` have all of them below 2^-40 and half below 2^-126;
    far_camera is out of range as a whole; no other case has a primary outside."""
    c = CC.case(name)
    share, lo, hi = CC.census(name)
    in_range = CC.camera_in_fast_range(c.camera)
    print(f"{name}: {share:.1%} of primaries outside [2^-40, 2^40], a in [{lo:.3g}, {hi:.3g}], "
          f"camera_in_fast_range {in_range}")
    assert np.isfinite([lo, hi]).all() and lo > 0  # no zero-length direction
    if name in CC.RANGE_CASES:
        assert in_range and 0.10 <= share <= 0.90
        assert np.abs(c.spheres["center"]).max() <= 2.0 ** 19 and np.abs(c.spheres["radius"]).max() <= 2.0 ** 19
    elif name in CC.SUBNORMAL_CASES:  # all outside, and a crosses the smallest normal number (49.4% below it)
        assert in_range and share == 1 and lo < 2.0 ** -126 < hi
    else:
        assert share == 0
        assert in_range == (name != "far_camera")


@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_extreme_rays_meet_geometry(name):
    c = CC.case(name)
    _, seg = CC.beauty_ref(name)
    per_primary = seg / (c.W * c.H * c.spp)
    hits = float(CC.aov_reference(name)["alpha"].mean())
    print(f"{name}: {per_primary:.2f} segments per primary, {hits:.1%} of primaries hit a sphere")
    assert per_primary > 2


def test_material_census():
    """Each altered parameter of `materials` (fuzz 0, 1, 2.5; albedo 0, 1; index 1, 0.75, 2.4,
    1.0000001) is the first hit of at least 20 of the frame's 12 800 samples."""
    s, m, where = CC.extreme_materials()
    assert len(where) == 9
    for label, mats in where.items():
        kind = label.split()[0]
        value = np.float32(label.split()[1])
        col = m["albedo"][mats] if kind == "albedo" else m["param"][mats]
        assert (col == value).all(), label  # the table carries what the label says
    for name in CC.MATERIAL_CASES:
        ids = CC.aov_reference(name)["sample_ids"]
        mats = s["material"][ids[ids != 0xffffffff]]
        count = {label: int(np.isin(mats, idx).sum()) for label, idx in where.items()}
        print(f"{name}: first hits per altered value: {count}")
        if name == "materials":
            assert min(count.values()) >= 20, count
    img, _ = CC.beauty_ref("materials")
    assert img.min() >= 0 and img.max() <= 1


@pytest.mark.parametrize("name", TILED)
def test_sky_tiles_meet_nothing(name):
    """tests/test_tiles_cpu.py's check under every 64 x 40 case: corner and random rays of the tiles
    rt_tile_order proves sky meet no sphere."""
    c = CC.case(name)
    perm, n_lead, n_sky = _check(c.spheres, c.materials, c.camera, c.W, c.H, row_offset=c.row_offset,
                                 row_stride=c.row_stride, min_sky=0)
    print(f"{name}: {len(perm)} blocks, n_lead {n_lead}, n_sky {n_sky}")


def test_enough_cases_reach_the_sky_kernel():
    """At least three cases have proven-sky tiles. Of the cameras first thought of, `rolled` has
    them (22 of 40 blocks) and `up` does not: it starts inside a cluster's box, where every tile's
    beam meets a box. So the table has three more on the huge scene: `up_clear`, the up camera
    raised to y = 2.2 above every ball (all 40 blocks sky: the main launch gets no item), `up_tilt`
    (5 lead, 30 sky) and `horizon` (17 lead, 16 sky). None of tiny, tiny_lens, wide and wide_lens
    has a sky tile either (seen from among the balls, and from 50 above a ground of radius 2^18,
    the proof fails for the ground), so the range gate of the sky kernel gets a pair of its own:
    `tiny_sky` (18 sky blocks) and `wide_sky` (24), and `subnormal_sky` (18) beside `subnormal`."""
    from raytracinginoneweekend_amd import tile_order
    n_sky = {}
    for name in TILED:
        c = CC.case(name)
        perm, _, n_sky[name] = tile_order((c.spheres, c.materials), CC.params(name), c.camera)
        assert len(perm) == c.W * len(range(c.row_offset, c.H, c.row_stride)) // 64
    print("n_sky per case:", n_sky)
    assert sum(v > 0 for v in n_sky.values()) >= 3
    assert n_sky["rolled"] > 0 and n_sky["up_tilt"] > 0 and n_sky["horizon"] > 0
    assert n_sky["up_clear"] == 40
    assert n_sky["tiny_sky"] > 0 and n_sky["wide_sky"] > 0 and n_sky["subnormal_sky"] > 0
