"""The device functions of rt_trace.h one by one on the MI355X: each short exact form at the edges of
its stated domain, against the plain references of tests/tools/probe_cases.py (whose tables
tests/test_primitives_cpu.py fixes without a GPU), through the test-only probe library
(tests/device/rt_probe.hip, which instantiates the header's own functions). Every comparison is on
the 32-bit words of outputs that start as a sentinel, 0 mismatches allowed; a failure names the first
mismatching input with the bits it got and wanted.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import probe  # noqa: E402
import probe_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu
U = np.uint32


def check(name, t, out, planes=None):
    """Output planes `planes` (default: all of the table's) against the table; returns the counts."""
    counts = []
    for p in (range(len(t.want)) if planes is None else planes):
        got = pc.canon(out[p]) if t.is_float[p] else out[p]
        bad = got != t.want[p]
        if t.mask[p] is not None:
            bad &= t.mask[p]
        nb = int(np.count_nonzero(bad))
        print(f"{name}: output {p}: {nb} of {t.n if t.mask[p] is None else int(t.mask[p].sum())} mismatch")
        if nb:
            i = int(np.flatnonzero(bad)[0])
            ins = " ".join(f"{int(probe.words(pl)[i]):08x}" for pl in t.planes)
            pytest.fail(f"{name}: output {p}: {nb} mismatches; first at lane {i} (wave {i // 64}, lane {i % 64}): "
                        f"inputs {ins}: got {int(out[p][i]):08x}, want {int(t.want[p][i]):08x}")
        counts.append(nb)
    return counts


def test_sqrt_scaled():
    t = pc.sqrt_table()
    check("sqrt_scaled", t, probe.run("sqrt_scaled", t.planes, 1))


def reciprocal_is_admissible(name, t, out):
    """rd.y is the reciprocal refined from a seed within an ulp of the correctly rounded one (what
    v_rcp_f32 promises); the count of lanes where it is not the correctly rounded seed's is printed."""
    a = t.planes[0]
    y = pc.canon(out[2])
    ys = [pc.canon(pc.host_call("rcp", [a], off=off)) for off in (-1, 0, 1)]
    ok = (y == ys[0]) | (y == ys[1]) | (y == ys[2])
    m = t.mask[2] if t.mask[2] is not None else np.ones(t.n, dtype=bool)
    print(f"{name}: rd.y: {int((m & ~ok).sum())} outside the admissible seeds' values, "
          f"{int((m & (y != ys[1])).sum())} of {int(m.sum())} not the correctly rounded seed's")
    if np.any(m & ~ok):
        i = int(np.flatnonzero(m & ~ok)[0])
        pytest.fail(f"{name}: rd.y of a = {int(pc.bf(a)[i]):08x}: got {int(out[2][i]):08x}, want one of "
                    f"{[f'{int(v[i]):08x}' for v in ys]}")


def test_ray_div_quotients():
    """div_ray on a in [2^-40, 2^40], |n| in [2^-60, 2^64): fd is 1 and the quotient is numpy's, at both
    ends of both ranges and at a = 2^k (1 - 2^-24), where the proof rests on v_rcp_f32's value
    (tests/test_primitives_cpu.py short_division)."""
    t = pc.ray_div_table()
    out = probe.run("ray_div", t.planes, 3, arg=1)
    check("ray_div", t, out, planes=(0, 1))
    reciprocal_is_admissible("ray_div", t, out)
    off = probe.run("ray_div", t.planes, 3, arg=0)
    assert not off[0].any(), "fast_roots = 0 must give fd = 0"


def test_ray_div_gate():
    """One active lane outside [2^-40, 2^40] (an ulp outside, NaN, subnormal, the `subnormal` camera's
    range) turns the wave's fd off in every lane; the same value in an inactive lane does not."""
    t = pc.ray_div_gate_table()
    out = probe.run("ray_div", t.planes, 3, arg=1)
    fd = out[0].reshape(-1, 64)
    assert np.all(fd == fd[:, :1]), "fd differs across a wave"
    if np.any(out[0] != t.want[0]):
        w = int(np.flatnonzero(out[0] != t.want[0])[0]) // 64
        pytest.fail(f"ray_div gate: wave {w} {t.info['names'][w]} (value, lane, active): fd {int(fd[w][0])}, "
                    f"want {int(t.want[0][64 * w])}")
    check("ray_div gate", t, out, planes=(0, 1))
    reciprocal_is_admissible("ray_div gate", t, out)
    assert not probe.run("ray_div", t.planes, 3, arg=0)[0].any(), "fast_roots = 0 must give fd = 0"


def test_roots():
    """near_root and far_root, the short forms (FD = 1) and the IEEE ones (FD = 0), against numpy and so
    against each other."""
    t = pc.roots_table()
    check("roots", t, probe.run("roots", t.planes, 6))


def test_div3_short():
    t = pc.div3_table()
    check("div3_short", t, probe.run("div3", t.planes, 4))


def test_div3_short_after_sqrt_scaled():
    t = pc.div3_sqrt_table()
    check("div3_short(d, sqrt_scaled(a))", t, probe.run("div3", t.planes, 4, arg=1))


def test_all_lanes_min_abs_ok():
    t = pc.div3_vote_table()
    out = probe.run("div3", t.planes, 4)
    if np.any(out[0] != t.want[0]):
        w = int(np.flatnonzero(out[0] != t.want[0])[0]) // 64
        pytest.fail(f"all_lanes_min_abs_ok: wave {w} {t.info['names'][w]} (value, component, lane, active): "
                    f"got {out[0][64 * w:64 * w + 64].tolist()}")
    check("all_lanes_min_abs_ok", t, out)


def test_div_const():
    """Both forms give numpy's quotient for every divisor of the table; the short one is what the host
    selects for each of them (tests/test_primitives_cpu.py asserts exact_by_reciprocal for all; a few
    are asked again here, through the library the device code is linked with)."""
    t = pc.div_const_table()
    for d in (1, 3, 720, 1280, 4096, 65536, 7 << 17):
        assert probe.exact_by_reciprocal(float(d)), d
    for fast in (1, 0):
        out = probe.run("div_const", t.planes + [np.full(t.n, fast, dtype=U)], 1)
        check(f"div_const fast={fast}", t, out)


def test_sphere_key():
    """sphere_key<false> against the reference's per-sphere candidate with the short roots (fd = 1: every
    |d|^2 of the table is in range) and the IEEE ones."""
    t = pc.sphere_table()
    for fast_roots in (1, 0):
        out = probe.run("sphere_key", t.planes, 3, arg=fast_roots)
        assert np.all(out[2] == fast_roots), "fd"
        bad = np.flatnonzero((out[0] != t.want[0]) | (out[1] != t.want[1]))
        print(f"sphere_key fast_roots={fast_roots}: {len(bad)} of {t.n} keys mismatch")
        if len(bad):
            i = int(bad[0])
            pytest.fail(f"sphere_key fast_roots={fast_roots}: {len(bad)} mismatches; first at wave {i // 64} "
                        f"({t.info['wave_names'][i // 64]}) lane {i % 64}, case {t.info['tag'][i]}, want {int(t.planes[0][i])}: "
                        f"inputs {' '.join(f'{int(probe.words(p)[i]):08x}' for p in t.planes[1:])}: "
                        f"got {int(out[1][i]):08x}:{int(out[0][i]):08x}, want {int(t.want[1][i]):08x}:{int(t.want[0][i]):08x}")


def test_in_range_and_hit_key():
    t = pc.in_range_table()
    check("in_range, hit_key", t, probe.run("in_range", t.planes, 3))


def test_min16_key():
    t = pc.min16_table()
    out = probe.run("min16_key", t.planes, 2)
    bad = np.flatnonzero((out[0] != t.want[0]) | (out[1] != t.want[1]))
    print(f"min16_key: {len(bad)} of {t.n} lanes mismatch")
    if len(bad):
        r = int(bad[0]) // 16
        keys = [f"{int(k):016x}" for k in t.info["keys"][16 * r:16 * r + 16]]
        got = [f"{int(k):016x}" for k in probe.join64(out[0], out[1])[16 * r:16 * r + 16]]
        pytest.fail(f"min16_key: {len(bad)} lanes mismatch; first in row {r} ({t.info['row_names'][r]}), row {r % 4} "
                    f"of its wave: keys {keys}: got {got}, want {int(probe.join64(t.want[0], t.want[1])[16 * r]):016x}")


def test_pcg_streams():
    t = pc.pcg_stream_table()
    check("pcg_seed, pcg_next", t, probe.run("pcg_stream", t.planes, pc.PCG_DRAWS + 2, arg=pc.PCG_DRAWS))


def test_canonical():
    """canonical and canonical_pm1 on chosen engine words (0, 2^24 +- 1, the clamp's two sides, words
    whose conversion rounds up) against libstdc++'s generate_canonical."""
    tc, tp = pc.canonical_table()
    check("canonical", tc, probe.run("canonical", tc.planes, 3, arg=0))
    check("canonical_pm1", tp, probe.run("canonical", tp.planes, 3, arg=1))


def test_random_in_unit_sphere_capped():
    """The capped form resumed call after call returns the uncapped form's point and state (and both the
    reference's), with 0..7 rejected attempts mixed within every wave."""
    t = pc.unit_sphere_table()
    check("random_in_unit_sphere", t, probe.run("unit_sphere", t.planes, 11))


def test_refract():
    t = pc.refract_table()
    check("refract", t, probe.run("refract", t.planes, 3))


def test_normalize():
    t = pc.normalize_table()
    check("normalize", t, probe.run("normalize", t.planes, 3))


def test_schlick_x():
    t = pc.schlick_table()
    check("schlick_x", t, probe.run("schlick_x", t.planes, 1))


def test_udiv():
    t = pc.udiv_table(probe.make_udiv)
    check("udiv", t, probe.run("udiv", t.planes, 1))


def test_probe_refuses_partial_waves():
    """The launchers' own guard: a length that is not whole waves is refused before any launch."""
    import torch
    buf = torch.zeros(256, dtype=torch.int32, device="cuda:0")
    for n in (0, 1, 63, 65):
        assert probe.lib().rt_probe_sqrt_scaled(buf.data_ptr(), buf.data_ptr(), n, 0, None) != 0
    torch.cuda.synchronize()
    assert not buf.any()
