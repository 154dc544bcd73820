"""The proof check of the trap windows, on the CPU.

tests/tools/trap_census.cpp traces paths in full with the restatement's brute-force hit_world and
the library's own host routine for the windows (rt_host_build.cpp trap_windows, compiled in). At
every hit where the kernels' trigger would fire, the rest of the trace must stay in that ball on
the total-reflection branch, use up depth 64 and return exactly 0: zero violations. Coverage is
asserted too, so windows that never fire do not pass, and the largest drift of the cosine along
trapped runs is set against the margin's constant (rt_consts.h kTrapDriftK, which the tool prints:
at least 8 x the drift, both in units of the margin's scale)."""
import os
import re
import subprocess

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(REPO, "tests", "tools", "trap_census.cpp"),
       os.path.join(REPO, "raytracinginoneweekend_amd", "csrc", "rt_host_build.cpp")]
DEPS = SRC + [os.path.join(REPO, "oracle", "rt_oracle.cpp"),
              os.path.join(REPO, "raytracinginoneweekend_amd", "csrc", "rt_host_build.h"),
              os.path.join(REPO, "raytracinginoneweekend_amd", "csrc", "rt_consts.h")]
BUILD = os.path.join(REPO, "tests", "tools", "_build")
THREADS = min(8, os.cpu_count() or 1)
# -ffp-contract=off as in the product and oracle builds: the restatement's bits
BASE = ["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-Wall"]


def _build(name, flags):
    out = os.path.join(BUILD, name)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in DEPS):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run([*BASE, *flags, "-o", out + ".tmp", *SRC], check=True)
        os.replace(out + ".tmp", out)
    return out


@pytest.fixture(scope="module")
def census():
    return _build("trap_census", ["-O2"])


def _run(exe, *args, env=None):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    rows = []
    for line in r.stdout.splitlines():
        rec = {"tag": line.split()[0]}
        for k, v in re.findall(r"(\w+)=(\S+)", line):
            rec[k] = v if ".." in v else float(v)
        rows.append(rec)
    return rows, r


@pytest.mark.parametrize("spp,corrected", [(8, 0), (2, 1)])
def test_every_trigger_holds_on_config_3(census, spp, corrected):
    """Config 3's frame (the huge scene, 1280x720, depth 64) at 8 spp with the reference camera and
    at 2 spp with the corrected one: every path the trigger ends runs to depth 64 inside its ball
    with colour 0; at the reference camera the trigger ends at least 85% of the max-depth paths."""
    rows, r = _run(census, "frame", 1280, 720, spp, corrected, THREADS)
    scene, frame = rows[0], rows[1]
    print(r.stdout)
    assert scene["tag"] == "scene" and frame["tag"] == "frame"
    assert scene["windows"] >= 100                      # most of the 157 glass balls are isolated
    assert frame["violations"] == 0 and frame["fired"] == frame["fired_maxdepth"] > 0
    assert frame["paths"] == 1280 * 720 * spp
    if not corrected:
        cover = frame["fired"] / frame["maxdepth_paths"]
        assert cover >= 0.85, f"the trigger ends {cover:.1%} of the max-depth paths"
    # the margin is at least 8 x the largest drift seen, both in units of D 2^-23 (|C|_inf + r) / kMIN
    assert scene["drift_k"] >= 8.0 * frame["drift_scaled"], (scene["drift_k"], frame["drift"], frame["drift_scaled"])


def test_adversarial_states(census):
    """Rays started on single balls a few ulp off the surface, cosines on, just inside and just
    outside both window ends and across the window; ior 1.33 and 1.5, radii 0.1, 0.2 and 1, centres
    at the origin, a few units out and at |C| ~ 500 (where a window is empty or still holds)."""
    rows, r = _run(census, "adversarial")
    print(r.stdout)
    assert len(rows) == 18
    for rec in rows:
        assert rec["violations"] == 0 and rec["fired"] == rec["fired_maxdepth"], rec
        assert rec["paths"] >= 2000
        lo, hi = map(float, rec["window"].split(".."))
        if lo <= hi:
            assert rec["fired"] > 1000, rec       # the in-window states do fire
            assert 0.0 < lo and hi < np.sqrt(1.0 - 1.0 / rec["ior"] ** 2)
        else:
            assert rec["fired"] == 0, rec
        if rec["c"] == 0:
            assert lo <= hi                        # a ball at the origin keeps its window


def test_windows_under_asan_ubsan():
    """The host routine and the census under AddressSanitizer + UndefinedBehaviorSanitizer, as a
    stand-alone program (no sanitizer on anything loaded into Python): a small frame and the
    adversarial states run clean."""
    exe = _build("trap_census_asan", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                                      "-fno-sanitize-recover=all"])
    env = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1:abort_on_error=0", "UBSAN_OPTIONS": "halt_on_error=1"}
    for args in (("frame", 160, 90, 2, 0, 4), ("adversarial",)):
        _, r = _run(exe, *args, env=env)
        assert not [x for x in ("AddressSanitizer", "runtime error:", "LeakSanitizer") if x in r.stderr], r.stderr[-3000:]


# ---- the windows' structure --------------------------------------------------------------------
def _glass_scene(rng, n, spread):
    """Small glass balls resting on the ground, touching and overlapping neighbours, a ball with a
    bubble (negative radius), exact duplicates, a big glass sphere off the ground with a ball
    inside it, lambert and metal balls."""
    s = np.zeros(n, dtype=abi.SPHERE_DTYPE)
    m = np.zeros(5, dtype=abi.MATERIAL_DTYPE)
    m[0] = (0, [0.5, 0.5, 0.5], 0.0)
    m[1] = (1, [0.7, 0.6, 0.5], 0.1)
    m[2] = (2, [1.0, 1.0, 1.0], 1.5)
    m[3] = (2, [1.0, 1.0, 1.0], 1.33)
    m[4] = (0, [0.8, 0.3, 0.2], 0.0)
    r = rng.choice([0.2, 0.2, 0.2, 0.1, 0.35], n).astype(np.float32)
    c = np.zeros((n, 3), dtype=np.float32)
    c[:, 0] = rng.uniform(-spread, spread, n)
    c[:, 2] = rng.uniform(-spread, spread, n)
    # resting on the ground sphere (centre (0, -1000, 0), radius 1000) where they stand
    c[:, 1] = np.sqrt((1000.0 + r.astype(np.float64)) ** 2 - c[:, 0].astype(np.float64) ** 2
                      - c[:, 2].astype(np.float64) ** 2) - 1000.0
    mat = rng.choice([2, 2, 3, 3, 2, 0, 1, 4], n)
    k = n // 8
    c[4:4 + k:2] = c[5:5 + k:2]
    c[4:4 + k:2, 0] += r[4:4 + k:2] + r[5:5 + k:2]                     # touching pairs
    c[4 + k:4 + 2 * k:2] = c[5 + k:5 + 2 * k:2]
    r[4 + k:4 + 2 * k:2] = r[5 + k:5 + 2 * k:2]     # equal radii: each cuts the other's shell
    c[4 + k:4 + 2 * k:2, 0] += 0.5 * (r[4 + k:4 + 2 * k:2] + r[5 + k:5 + 2 * k:2])  # overlapping pairs
    c[5 * k], r[5 * k], mat[5 * k] = c[5 * k + 1], -0.8 * r[5 * k + 1], 2  # a bubble in ball 5k + 1
    mat[5 * k + 1] = 2
    c[6 * k], r[6 * k], mat[6 * k] = c[6 * k + 1], r[6 * k + 1], mat[6 * k + 1]  # exact duplicates
    s["center"], s["radius"], s["material"] = c, r, mat
    s["center"][0], s["radius"][0], s["material"][0] = (0, -1000, 0), 1000.0, 0
    s["center"][1], s["radius"][1], s["material"][1] = (spread + 3, 1.5, 0), 1.0, 2   # the big glass sphere
    s["center"][2], s["radius"][2], s["material"][2] = (spread + 3.2, 1.6, 0.1), 0.2, 2  # a ball inside it
    s["center"][3], s["radius"][3], s["material"][3] = (spread + 6, 1.5, 0), 0.2, 0   # lambert, isolated
    return s, m


@pytest.mark.parametrize("seed,n,spread", [(7, 300, 12.0), (8, 500, 14.0), (9, 200, 8.0), (7, 400, 6.0)])
def test_window_structure_on_glass_scenes(seed, n, spread):
    """Balls resting on the ground, touching and overlapping pairs, a ball with a bubble, exact
    duplicates, the big glass sphere (a ball lies inside it) and everything that is not glass have
    empty windows; the ball inside the big glass sphere has one, within the TIR bound of its ior."""
    s, m = _glass_scene(np.random.default_rng(seed), n, spread)
    w = rt.trap_windows((s, m))
    assert w.shape == (n, 2) and w.dtype == np.float32
    has = w[:, 0] <= w[:, 1]
    assert list(np.flatnonzero(has)) == [2], np.flatnonzero(has)
    assert (w[~has] == np.float32([1, 0])).all()
    lo, hi = map(float, w[2])
    assert 0.008 / 0.4 < lo < 0.05 and 0.70 < hi < np.sqrt(1 - 1 / 1.5 ** 2)
    # lifted off the ground by 5% of its radius, a ball that has no other neighbour gets a window
    s2 = s.copy()
    s2["center"][:, 1][4:] += 0.05 * np.abs(s2["radius"][4:])
    has2 = (lambda v: v[:, 0] <= v[:, 1])(rt.trap_windows((s2, m)))
    glass = np.isin(s2["material"], [2, 3]) & (s2["radius"] > 0)
    assert has2.sum() > 10 and not has2[~glass].any()
    k = n // 8
    for i in (*range(4, 4 + 2 * k), 5 * k, 5 * k + 1, 6 * k, 6 * k + 1):
        assert not has2[i], i                      # pairs, bubble and its ball, duplicates: still none


def test_window_margins_scale_with_the_centre():
    """The drift margin grows with |C|_inf + r: the window narrows away from the origin and is
    empty where the margins meet (a tiny ball, a ball at large coordinates)."""
    m = np.zeros(1, dtype=abi.MATERIAL_DTYPE)
    m[0] = (2, [1, 1, 1], 1.5)

    def window(c, r):
        s = np.zeros(1, dtype=abi.SPHERE_DTYPE)
        s[0] = (c, r, 0)
        return tuple(map(float, rt.trap_windows((s, m))[0]))
    a, b, far = window((0, 0, 0), 0.2), window((10, 0, 0), 0.2), window((1e4, 0, 0), 0.2)
    assert a[0] < b[0] < b[1] < a[1] and far == (1.0, 0.0)
    assert window((0, 0, 0), 0.005) == (1.0, 0.0)       # 2 r < kMIN / cos for every cosine in reach
    assert window((0, 0, 0), -0.2) == (1.0, 0.0) and window((0, 0, 0), float("nan")) == (1.0, 0.0)
    m[0] = (2, [1, 1, 1], 1.0)
    assert window((0, 0, 0), 0.2) == (1.0, 0.0)         # ior 1: no total reflection
    m[0] = (2, [1, 1, 1], 0.8)
    assert window((0, 0, 0), 0.2) == (1.0, 0.0)


def test_no_trap_end_option():
    o = rt.parse_options("no_trap_end=1")
    assert o.diag == abi.RT_DIAG["no_trap_end"]
    assert rt.parse_options(f"diag={abi.RT_DIAG['no_trap_end']}").diag == abi.RT_DIAG["no_trap_end"]
    assert rt.parse_options("no_trap_end=0", o).diag == 0
