"""The sky kernel's sample loop where its parts meet: the ring of lens points a
lane draws ahead, the blocks of 4 of the blocked sum and the tail samples.

The other GPU suites render sky blocks at 5 samples per pixel (tests/tools/camera_cases.py) and at
the full configurations. Here the cameras with proven-sky blocks render at sample counts below
and at the block size, with tails of 1 to 3, with fewer samples than any ring depth and with more
than any: `up_clear` (all 40 blocks sky, the main launch gets no item), `rolled` (22 sky blocks:
five and a half workgroups, so the last one has dead waves), `horizon`, and `tiny_sky`, `wide_sky`,
`subnormal_sky` (sky waves partly or wholly outside the range of the short-form unit direction).

Every comparison is on uint32 views with zero mismatches allowed, against the CPU restatement
(tests/oracle_binding.py), and the segment counts are equal. References and default renders are
computed once per module and shared.
"""
import functools
import os
import sys

import pytest

import raytracinginoneweekend_amd as rt

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import camera_cases as CC  # noqa: E402
import oracle_binding as O  # noqa: E402
from support import assert_bits  # noqa: E402

pytestmark = pytest.mark.gpu

SKY_CASES = ("up_clear", "rolled", "horizon", "tiny_sky", "wide_sky", "subnormal_sky")
SPPS = (1, 2, 3, 4, 7, 8, 9, 13, 33)
NO_SKY_SPPS = (4, 9, 33)
SHARE_CASE, SHARE_SPP, SHARE_OFFSET, SHARE_STRIDE = "up_clear", 9, 1, 3  # 8 of the share's 13 blocks are sky


def params(name, spp, **kw):
    """The case's frame at `spp` samples per pixel (camera_cases.py keeps its own 5)."""
    c = CC.case(name)
    return rt.make_params(c.W, c.H, spp, c.depth, c.seed, **kw)


@functools.lru_cache(maxsize=None)
def oracle(name, spp):
    c = CC.case(name)
    img, seg = O.render_f32(c.spheres, c.materials, c.camera, params(name, spp))
    img.flags.writeable = False
    return img, int(seg)


@functools.lru_cache(maxsize=None)
def gpu_default(name, spp):
    c = CC.case(name)
    img, st = rt.render_f32(CC.scene(name), params(name, spp), c.camera)
    img.flags.writeable = False
    return img, int(st.segments), int(st.primaries)


def sky_blocks(name, p):
    c = CC.case(name)
    perm, _, n_sky = rt.tile_order(CC.scene(name), p, c.camera)
    return len(perm), int(n_sky)


@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("name", SKY_CASES)
def test_beauty_matches_oracle(name, spp):
    c = CC.case(name)
    n_blocks, n_sky = sky_blocks(name, params(name, spp))
    print(f"{name} spp {spp}: {n_sky} sky blocks of {n_blocks}")
    assert n_blocks == c.W * c.H // 64 and n_sky > 0
    if name == "up_clear":
        assert n_sky == 40
    if name == "rolled":
        assert n_sky % 4 != 0  # 256-thread workgroups of 4 blocks: the last one is not full
    ref, ref_seg = oracle(name, spp)
    img, seg, prim = gpu_default(name, spp)
    assert_bits(img, ref, f"{name} spp {spp}")
    assert seg == ref_seg
    assert prim == c.H * c.W * spp


@pytest.mark.parametrize("spp", NO_SKY_SPPS)
@pytest.mark.parametrize("name", SKY_CASES)
def test_main_launch_renders_the_same_bits(name, spp, opts):
    """The `no_sky` option hands the proven-sky tiles to the main launch: the default render's bits."""
    c = CC.case(name)
    img, seg, _ = gpu_default(name, spp)
    opts.set(no_sky=True)
    got, st = rt.render_f32(CC.scene(name), params(name, spp), c.camera)
    assert_bits(got, img, f"{name} spp {spp} no_sky against the default render")
    assert_bits(got, oracle(name, spp)[0], f"{name} spp {spp} no_sky against the oracle")
    assert st.segments == seg == oracle(name, spp)[1]


def test_row_share_with_sky_blocks():
    """Rows 1, 4, 7, ... of a frame with sky blocks, packed: the oracle's rows of the whole frame
    (streams are keyed by the global pixel and sample)."""
    c = CC.case(SHARE_CASE)
    p = params(SHARE_CASE, SHARE_SPP, row_offset=SHARE_OFFSET, row_stride=SHARE_STRIDE)
    rows = slice(SHARE_OFFSET, c.H, SHARE_STRIDE)
    n_blocks, n_sky = sky_blocks(SHARE_CASE, p)
    print(f"{SHARE_CASE} share: {n_sky} sky blocks of {n_blocks}")
    assert n_blocks == len(range(c.H)[rows]) * c.W // 64 and n_sky > 0
    ref = oracle(SHARE_CASE, SHARE_SPP)[0][rows]
    packed, packed_seg = O.render_f32(c.spheres, c.materials, c.camera, p)
    assert_bits(packed, ref, "oracle: the share against the whole frame's rows")
    got, st = rt.render_f32(CC.scene(SHARE_CASE), p, c.camera)
    assert_bits(got, ref, f"{SHARE_CASE} share packed")
    assert st.segments == packed_seg
