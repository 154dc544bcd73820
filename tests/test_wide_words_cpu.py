"""The cases of tests/tools/wide_cases.py are what they claim to be, from the reference side alone
(the CPU restatement, which tests/test_oracle_golden.py pins to the reference itself on a seed above
2^32 and on a row of a 2^32 - 65536 pixel frame; the per-sample tools over it; the host's tile
classification). tests/test_wide_words_gpu.py compares the kernels with these references; a case
that stopped reaching its words or its code path fails here, not silently there. No GPU.

Measured, 16 threads on 8 cores: the restatement renders split/reference in 0.9 - 1.4 s,
split/corrected in 2.3 - 3.9 s, deep/reference in 0.2 s, deep/corrected in 2.1 - 5.0 s and
ground/reference (a sky tile row and a row of far ground: 1.2 segments per sample) in 0.2 s (the
spread is the machine's other load).
"""
import os
import sys

import numpy as np
import pytest

import golden_io as G
import raytracinginoneweekend_amd as rt

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import wide_cases as WC  # noqa: E402
from support import assert_bits, words as u32  # noqa: E402

# "A few seconds" per band on 16 threads. The slowest band measured 2.1 s alone and 5.0 s beside a
# compiler on the same 8 cores; three times that is the bound, so that only a band that has become
# several times dearer fails, not a busy machine.
BAND_SECONDS = 15.0


def test_frame_and_bands_reach_the_wide_words():
    assert 2 ** 32 - 2 ** 20 <= WC.W * WC.H < 2 ** 32 and WC.W <= 8192
    assert WC.SPP == 5  # one block of 4 samples and a single-sample tail
    for band, b in WC.BANDS.items():
        assert b["num_rows"] <= 16 and max(WC.rows_of(band)) < WC.H
        lo, hi = WC.key_range(band)
        print(band, "keys 2^%.2f .. 2^%.2f" % (np.log2(lo), np.log2(hi)), "pixel indices", WC.index_range(band))
        assert lo >= 2 ** 32 and hi < 2 ** 64
        assert WC.index_range(band)[1] < 2 ** 32
    assert all(WC.index_range(band)[0] >= 2 ** 31 for band in WC.BANDS)
    # both increments of SEED have a high word; those of bit63 have bit 63 set
    for name in WC.WIDE_SEEDS:
        s = WC.SEEDS[name]
        assert (((2 * s) << 1) | 1) % 2 ** 64 >> 32 and (((2 * s + 1) << 1) | 1) % 2 ** 64 >> 32, name
    assert ((2 * WC.SEEDS["bit63"]) << 1) >> 63 & 1
    assert WC.SEED == WC.SEEDS["hi32"]
    # the cuda-compat band: the 32-bit engine state x + y W + seed wraps inside it
    y0 = WC.COMPAT_ROWS["row_offset"]
    first, last = y0 * WC.W + WC.COMPAT_SEED, (WC.H - 1) * WC.W + WC.W - 1 + WC.COMPAT_SEED
    assert first < 2 ** 32 <= last


@pytest.mark.parametrize("band,mode", WC.BAND_MODES)
def test_band_renders_in_a_few_seconds(band, mode):
    img, seg, seconds = WC.band_ref(band, mode)
    n = img.shape[0] * WC.W * WC.SPP
    print(f"{band} {mode}: {seconds:.2f} s, {seg / n:.2f} segments per sample")
    assert img.shape == (WC.BANDS[band]["num_rows"], WC.W, 3) and seg >= n
    assert seconds < BAND_SECONDS


def test_split_band_census():
    """Under the reference camera the split band has sky pixels and surface pixels, every material
    kind among its first hits, and the host's classification deals it as lead tiles and sky tiles."""
    aov = WC.band_aov_ref("split", "reference")
    sky, surface = int((aov["alpha"] == 0).sum()), int((aov["alpha"] == 1).sum())
    kinds = WC.first_hit_kinds(aov)
    perm, n_lead, n_sky = rt.tile_order(WC.scene(), WC.params("split"), WC.camera("reference"))
    print("sky pixels", sky, "surface pixels", surface, "kinds", kinds, "blocks", len(perm), "lead", n_lead, "sky", n_sky)
    assert sky > 0 and surface > 0
    assert kinds == WC.ALL_KINDS
    assert len(perm) == 16 * WC.W // 64 and n_lead > 0 and n_sky > 0


def test_ground_band_census():
    """Under the reference camera the ground band's first tile row is sky and its second is the far
    ground: 817 ground tiles, proven as tests/test_ground_cpu.py proves them (no ray of theirs meets
    a clustered sphere), beside 207 tiles that meet the field. Every pixel index is >= 2^31 and
    every key > 2^33; the only first hit inside ground tiles is the ground (a list of one), and
    part of their samples reach the sky (those are never redone)."""
    import ground_checks as GC
    b = WC.BANDS["ground"]
    assert b["num_rows"] == 16 and 1000 <= b["row_stride"] <= WC.BANDS["split"]["row_stride"]
    assert WC.band_tiles("ground", "reference") == (2048, 207, 817, 1024)
    lo, hi = WC.key_range("ground")
    assert 2 ** 33 < lo < hi < 2 ** 34 and WC.index_range("ground")[0] >= 2 ** 31
    s, m = WC.scene()
    assert GC.check(s, m, WC.camera("reference"), WC.W, WC.H, **b) == (817, 817)
    hits, sky = GC.first_hits_in_ground_tiles(WC.scene(), WC.params("ground"), WC.camera("reference"))
    print("first hits in ground tiles", hits, "sky samples", sky)
    assert list(hits) == np.flatnonzero(GC.clustered(s)[1]).tolist() and len(hits) == 1
    assert hits[next(iter(hits))] > 64 * WC.SPP * 64 and sky > 0


def test_small_frame_has_ground_tiles():
    """64 x 36: four tile rows, 4 ground tiles (tests/test_ground_cpu.py), whatever the seed."""
    assert WC.small_ground_tiles() == 4
    for seed in WC.SEEDS.values():
        assert rt.tile_ground(WC.scene(), WC.small_params(seed), WC.small_camera()) == 4


@pytest.mark.parametrize("name", WC.WIDE_SEEDS)
def test_redo_frame_redoes_samples_under_the_wide_seeds(name):
    """The redo frame has 85 ground tiles whatever the seed, and under each wide seed ground samples
    of three segments and more (they go to the redo launch) beside ground samples that reach the sky
    (they never do)."""
    import ground_checks as GC
    p, cam = WC.redo_params(WC.SEEDS[name]), WC.redo_camera()
    assert rt.tile_ground(WC.scene(), p, cam) == 85
    long_paths = GC.long_paths_in_ground_rows(WC.scene(), p, cam)
    hits, sky = GC.first_hits_in_ground_tiles(WC.scene(), p, cam)
    print(f"seed {name}: {long_paths} segments past the second, first hits {hits}, {sky} sky samples")
    assert long_paths > 0 and sky > 0 and len(hits) == 1


def test_deep_band_census():
    """Under the corrected camera the deep band's paths are long (trapped in glass: what the deep
    launch exists for); under the reference camera every primary ray of it reaches the sky."""
    img, seg, _ = WC.band_ref("deep", "corrected")
    n = img.shape[0] * WC.W * WC.SPP
    print("deep corrected: segments per sample", seg / n)
    assert seg / n > 8
    _, seg_ref, _ = WC.band_ref("deep", "reference")
    assert seg_ref == n


def test_wide_seeds_draw_other_streams_and_aliases_the_same():
    """The wide seeds change more than half of the small frame's values; s + 2^62 and s + 2^63 change
    none (the increments' shift drops the seed's top two bits)."""
    base, base_seg = WC.small_ref(WC.BASE_SEED)
    meta, f32, _ = G.render("huge_64x36_s4")
    assert (meta["width"], meta["height"], meta["spp"], meta["seed"]) == (*WC.SMALL, WC.BASE_SEED)
    assert_bits(base, f32)  # the reference's own frame
    for name in WC.WIDE_SEEDS:
        img, _ = WC.small_ref(WC.SEEDS[name])
        changed = int(np.count_nonzero(u32(img) != u32(base)))
        print(name, "changes", changed, "of", base.size)
        assert changed > base.size // 2, name
    for name in WC.ALIAS_SEEDS:
        img, seg = WC.small_ref(WC.SEEDS[name])
        assert np.array_equal(u32(img), u32(base)) and seg == base_seg, name
    # the wide seeds differ from each other too
    imgs = [WC.small_ref(WC.SEEDS[n])[0] for n in WC.WIDE_SEEDS]
    for i in range(len(imgs)):
        for j in range(i):
            assert np.count_nonzero(u32(imgs[i]) != u32(imgs[j])) > base.size // 2


def test_reference_fixture_of_the_wide_seed_is_the_small_case():
    """tests/golden/huge_64x36_s4_seedhi is the reference's own render of the small frame with SEED."""
    meta, f32, _ = G.render("huge_64x36_s4_seedhi")
    assert (meta["width"], meta["height"], meta["spp"], meta["seed"]) == (*WC.SMALL, WC.SEED)
    assert_bits(WC.small_ref(WC.SEED)[0], f32)
    wide = G.manifest()["renders"]["wide_huge_4096x1048560_row838848_s5_seedhi"]
    assert wide["seed"] == WC.SEED and wide["width"] <= 4096 and wide["num_rows"] == 1
    assert 2 ** 32 - 2 ** 20 <= wide["width"] * wide["height"] < 2 ** 32
    assert wide["row_offset"] * wide["width"] >= 2 ** 31 and wide["row_offset"] * wide["width"] * wide["spp"] >= 2 ** 32


def test_compat_seed_is_32_bits_wide():
    """oracle_render_cuda_compat: seed 7 + 2^32 gives seed 7's frame, and the band that wraps has
    pixels on both sides of the wrap that are not black."""
    s, m = WC.compat_scene()
    import oracle_binding as O
    cam = rt.Camera.cuda(64, 36).c
    a, _ = O.render_cuda_compat(s, m, cam, rt.make_params(64, 36, 4, 32, 7, cuda_compat=True))
    b, _ = O.render_cuda_compat(s, m, cam, rt.make_params(64, 36, 4, 32, 7 + 2 ** 32, cuda_compat=True))
    assert np.array_equal(u32(a), u32(b)) and a.any()
    img, seg = WC.compat_ref()
    assert img.shape == (8, WC.W, 3) and seg >= 8 * WC.W * WC.COMPAT_SPP and img[0].any() and img[-1].any()
