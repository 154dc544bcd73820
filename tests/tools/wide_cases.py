"""TEST INFRASTRUCTURE: the cases of the 64-bit seed and stream-key tests, shared by
tests/test_wide_words_cpu.py (which fixes, from the reference side alone, that the cases are what
they claim to be) and tests/test_wide_words_gpu.py.

Every sample owns two PCG32 streams: key = (y W + x) spp + s, increments ((2 seed) << 1) | 1 and
((2 seed + 1) << 1) | 1 (include/rt_api.h). The other suites keep the key and both increments below
2^32. Here:

  the frame    8192 x 524280 (W H = 2^32 - 65536, the host's limit is W H < 2^32), 5 spp: one block
               of 4 samples (a sample pair block) and a single-sample tail
  the bands    `split`: 16 rows 270000, 279800, ... (stride 9800) across the reference camera's
               horizon: the first tile row is sky, the second meets the scene; every pixel index
               y W + x >= 2^31, keys 2^33.4 .. 2^34.0
               `deep`: the 8 rows from 366992; under the corrected camera its paths are trapped in
               glass (16.7 segments per sample), under the reference camera it is sky
               `ground`: 16 rows 348000, 350000, ... (stride 2000) just under that horizon: the first
               tile row is sky; of the second, the far ground, 817 tiles are ground tiles (their
               beams meet no cluster: ground_kernel and the redo launch render them when the pass
               is split) and 207 meet the field; keys 2^33.7 .. 2^33.8
  the seeds    SEED = 1234 + 2^32 on the bands; on the small frame (the huge scene at 64 x 36, 4 spp)
               every seed of SEEDS, among them the aliases: the increments drop the seed's top two
               bits, so s and s + 2^62 name the same streams
               and on the redo frame (128 x 72, 5 spp, the redo camera: 85 ground tiles) the wide ones
  cuda-compat  the engine state x + y W + seed is 32 bits wide: the last 8 rows of the frame with
               seed 100000 wrap 2^32 inside the band

References come from the CPU restatement (oracle/rt_oracle.cpp) and its per-sample tools, once per
process (functools.lru_cache), read-only.
"""
import functools
import os
import sys
import time

import numpy as np

import oracle_binding as O
import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aov_ref  # noqa: E402
import moments_ref  # noqa: E402

THREADS = 16
W, H, SPP, DEPTH = 8192, 524280, 5, 64
SEED = 1234 + 2 ** 32
BANDS = {"split": dict(row_offset=270000, row_stride=9800, num_rows=16),
         "deep": dict(row_offset=366992, row_stride=1, num_rows=8),
         "ground": dict(row_offset=348000, row_stride=2000, num_rows=16)}
# the (band, camera) pairs the suites render; the ground band is for the reference camera only
BAND_MODES = [("deep", "corrected"), ("deep", "reference"), ("split", "corrected"), ("split", "reference"),
              ("ground", "reference")]
MODES = {"reference": rt.REFERENCE, "corrected": rt.CORRECTED}

SMALL = (64, 36, 4)  # W, H, spp of the small frame (the golden render huge_64x36_s4's)
BASE_SEED = 1234
SEEDS = {"hi32": 1234 + 2 ** 32, "max": 2 ** 64 - 1, "bit63": 2 ** 61 + 1234,
         "alias62": 1234 + 2 ** 62, "alias63": 1234 + 2 ** 63}
WIDE_SEEDS = ("hi32", "max", "bit63")     # other streams than BASE_SEED's
ALIAS_SEEDS = ("alias62", "alias63")      # BASE_SEED's streams

COMPAT_SEED = 100000
COMPAT_ROWS = dict(row_offset=H - 8, row_stride=1, num_rows=8)
COMPAT_SPP, COMPAT_DEPTH = 4, 32


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def scene():
    return _frozen(*rt.huge_scene_arrays(1234))


def rows_of(band):
    b = BANDS[band]
    return [b["row_offset"] + i * b["row_stride"] for i in range(b["num_rows"])]


def key_range(band):
    """(smallest, largest) stream key of the band's samples."""
    ys = rows_of(band)
    return min(ys) * W * SPP, (max(ys) * W + W - 1) * SPP + SPP - 1


def index_range(band):
    """(smallest, largest) pixel index y W + x of the band."""
    ys = rows_of(band)
    return min(ys) * W, max(ys) * W + W - 1


def camera(mode):
    return rt.Camera.default(W, H, MODES[mode])


@functools.lru_cache(maxsize=None)
def band_tiles(band, mode):
    """(blocks, lead tiles, ground tiles, sky tiles) of the band's pass, from the host's
    classification (rt.tile_order, rt.tile_ground)."""
    perm, n_lead, n_sky = rt.tile_order(scene(), params(band), camera(mode))
    return len(perm), n_lead, rt.tile_ground(scene(), params(band), camera(mode)), n_sky


@functools.lru_cache(maxsize=None)
def small_ground_tiles():
    """The small frame's ground tiles (the class does not depend on the seed)."""
    return rt.tile_ground(scene(), small_params(BASE_SEED), small_camera())


def params(band, seed=SEED, rows=None, **kw):
    """The band's pass; rows = (first, count): that part of the band's rows."""
    b = dict(BANDS[band])
    if rows is not None:
        b["row_offset"] += rows[0] * b["row_stride"]
        b["num_rows"] = rows[1]
    return rt.make_params(W, H, SPP, DEPTH, seed, **b, **kw)


@functools.lru_cache(maxsize=None)
def band_ref(band, mode):
    """(image (rows, W, 3), segments, seconds the restatement took on THREADS threads)."""
    t = time.perf_counter()
    img, seg = O.render_f32(*scene(), camera(mode).c, params(band), threads=THREADS)
    dt = time.perf_counter() - t
    return _frozen(img)[0], seg, dt


@functools.lru_cache(maxsize=None)
def band_aov_ref(band, mode):
    """tests/tools/aov_ref's planes of the band, with the per-sample first-hit ids."""
    out = aov_ref.render(*scene(), camera(mode), params(band), sample_ids=True)
    _frozen(*out.values())
    return out


@functools.lru_cache(maxsize=None)
def band_moments_ref(band, mode):
    """(rgb, var) of tests/tools/moments_ref."""
    rgb, var, _ = moments_ref.render(*scene(), camera(mode), params(band))
    return _frozen(rgb, var)


def small_camera(mode="reference"):
    return rt.Camera.default(SMALL[0], SMALL[1], MODES[mode])


def small_params(seed, **kw):
    return rt.make_params(SMALL[0], SMALL[1], SMALL[2], DEPTH, seed, **kw)


@functools.lru_cache(maxsize=None)
def small_ref(seed):
    """(image (36, 64, 3), segments) of the small frame with `seed`."""
    img, seg = O.render_f32(*scene(), small_camera().c, small_params(seed), threads=THREADS)
    return _frozen(img)[0], seg


# the redo frame: the huge scene at 128 x 72, 5 spp, under tests/tools/ground_checks.py's redo camera
# (85 ground tiles, about a tenth of whose samples go to the redo launch): render_list_kernel under
# the wide seeds, which the small frame's 4 ground tiles barely reach
REDO = (128, 72, 5)


def redo_camera():
    import ground_checks as GC
    return GC.redo_camera(REDO[0] / REDO[1])


def redo_params(seed, **kw):
    return rt.make_params(REDO[0], REDO[1], REDO[2], DEPTH, seed, **kw)


@functools.lru_cache(maxsize=None)
def redo_ref(seed):
    """(image (72, 128, 3), segments) of the redo frame with `seed`."""
    img, seg = O.render_f32(*scene(), redo_camera().c, redo_params(seed), threads=THREADS)
    return _frozen(img)[0], seg


@functools.lru_cache(maxsize=None)
def small_aov_ref(seed):
    out = aov_ref.render(*scene(), small_camera(), small_params(seed))
    _frozen(*out.values())
    return out


@functools.lru_cache(maxsize=None)
def small_moments_ref(seed):
    rgb, var, _ = moments_ref.render(*scene(), small_camera(), small_params(seed))
    return _frozen(rgb, var)


@functools.lru_cache(maxsize=None)
def compat_scene():
    return _frozen(*rt.cuda_scene_arrays())


def compat_params(seed=COMPAT_SEED):
    return rt.make_params(W, H, COMPAT_SPP, COMPAT_DEPTH, seed, cuda_compat=True, **COMPAT_ROWS)


@functools.lru_cache(maxsize=None)
def compat_ref(seed=COMPAT_SEED):
    img, seg = O.render_cuda_compat(*compat_scene(), rt.Camera.cuda(W, H).c, compat_params(seed), threads=THREADS)
    return _frozen(img)[0], seg


def first_hit_kinds(aov):
    """The material kinds among the per-sample first hits of an aov_ref result."""
    s, m = scene()
    ids = aov["sample_ids"]
    return set(m["kind"][s["material"][ids[ids != 0xffffffff]]].tolist())


ALL_KINDS = {abi.RT_LAMBERT, abi.RT_METAL, abi.RT_DIELECTRIC}
