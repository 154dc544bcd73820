"""The probe tables (tests/tools/probe_cases.py) are what they claim, fixed on the CPU: every binade,
edge and named case is present (counts printed), a host restatement of each short sequence
(tests/tools/probe_host.cpp) gives the reference's bits on the whole table for each admissible
hardware seed (the correctly rounded 1/a or sqrt and its neighbours one ulp below and above), and the
same restatement with its gate ignored differs from IEEE outside the domain. No GPU.
tests/test_primitives_gpu.py runs the same tables through the product's device functions."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import probe  # noqa: E402
import probe_cases as pc  # noqa: E402

F, U = np.float32, np.uint32
SEEDS = (-1, 0, 1)


def mism(got, want, mask=None):
    got, want = [pc.canon(v) if v.dtype == np.float32 else v for v in (np.asarray(got), np.asarray(want))]
    bad = got != want
    if mask is not None:
        bad &= mask
    return int(np.count_nonzero(bad))


def short_division(n, a, want, what):
    """The short division's restatement on (n, a) against the reference's bits `want`: exact from the
    correctly rounded seed; from a neighbouring seed exact wherever the refined reciprocal y is the one
    refined from the correctly rounded seed. Where y depends on the seed (a = 2^k (1 - 2^-24): 1 / a lies
    2^-48 relative above a rounding midpoint, and only the correctly rounded seed refines to the upper
    neighbour) a power-of-two numerator's quotient is a tie that only the right y breaks correctly, e.g.
    a = 0x1.fffffep39, n = 0x1p-60: 0x1.000002p-100, from the seeds 0x1p-40 and 0x1.000004p-40
    0x1p-100 (and a = 0xfffffd, n = 0xd55553 from the seed above). The compiler's IEEE sequence has the same two corrections on the same y, so it rests on
    v_rcp_f32's value there as well; the device's y is pinned on these tables' a by
    tests/test_primitives_gpu.py test_ray_div_quotients. Returns the number of seed-dependent quotients."""
    y0 = pc.canon(pc.host_call("rcp", [a], off=0))
    assert mism(pc.host_call("div", [n, a], off=0), want) == 0, what
    dep = 0
    for off in (-1, 1):
        same_y = pc.canon(pc.host_call("rcp", [a], off=off)) == y0
        assert mism(pc.host_call("div", [n, a], off=off), want, same_y) == 0, f"{what}, seed {off:+d}"
        dep = max(dep, mism(pc.host_call("div", [n, a], off=off), want))
    return dep


def test_sqrt_table_and_restatement():
    t = pc.sqrt_table()
    x = t.planes[0]
    print(f"sqrt_scaled: {t.n} inputs: {t.info['n_binade']} over {len(t.info['binades'])} binades, "
          f"{t.info['n_square']} around squares, {t.info['n_special']} special")
    assert t.info["binades"] == set(range(-149, 96))
    # every binade: its lowest and highest mantissas
    b = set(x.view(U).tolist())
    for e in range(-126, 96):
        lo = (e + 127) << 23
        assert {lo, lo + 63, lo + (1 << 23) - 1, lo + (1 << 23) - 64} <= b, e
    assert {1, 2, 3, 0x007FFFFF} <= b
    # the special values as the callers meet them
    want = dict(zip(x.view(U).tolist(), t.want[0].tolist()))
    assert want[0] == 0 and all(want[int(s)] == pc.QNAN for s in t.info["special"][1:])
    # the reference root is the correctly rounded one: the double root of a float rounds once
    pos = x > 0
    assert mism(np.sqrt(x[pos].astype(np.float64)).astype(F), pc.fb(t.want[0])[pos]) == 0
    # squares' neighbours straddle midpoints: the roots of RN(s^2) +- 1 ulp differ from s somewhere
    assert t.info["n_square"] == 5 << 14
    dom = pos & (x < pc.p2(96))
    for off in SEEDS:
        got = pc.host_call("sqrt", [x], off=off)
        assert mism(got, t.want[0], dom) == 0, f"seed {off:+d}"
    # +0 and the NaN cases through the restatement as well
    assert mism(pc.host_call("sqrt", [x], off=0), t.want[0]) == 0


def test_division_tables_and_restatement():
    t = pc.ray_div_table()
    a, _, n = t.planes
    print(f"ray_div: {t.n} quotients, a over {len(t.info['a_binades'])} binades, |n| over {len(t.info['n_binades'])}")
    assert set(range(-40, 40)) <= t.info["a_binades"] <= set(range(-40, 41))
    assert t.info["n_binades"] == set(range(-60, 64))
    assert np.all((a >= pc.A_LO) & (a <= pc.A_HI) & (np.abs(n) >= pc.p2(-60)) & (np.abs(n) < pc.p2(64)))
    for ea in t.info["edges_a"]:
        for en in t.info["edges_n"]:
            assert np.any((a == ea) & (n == en))
    assert {x.hex() for x in map(float, t.info["edges_a"])} == {"0x1.0000000000000p-40", "0x1.0000020000000p-40",
                                                                "0x1.fffffe0000000p+39", "0x1.0000000000000p+40"}
    sens = pc.seed_sensitive_mantissas()
    print(f"ray_div: {len(sens)} divisor mantissas whose refined reciprocal depends on the seed: "
          f"{[hex(m) for m in sens[:4]]} .. {[hex(m) for m in sens[-2:]]}, each at {len(t.info['sensitive']) // len(sens)} exponents")
    assert 0xFFFFFF in sens and 0xFFFFFD in sens and len(sens) <= 64
    assert set((pc.bf(t.info["sensitive"]) & 0x7FFFFF | 0x800000).tolist()) == set(sens)
    assert np.all(np.isin(t.info["sensitive"], a))
    # div_ray's second correction changes no quotient of the table, from any seed: with y = RN(1 / a) the first
    # one already rounds correctly (Markstein), and where y is not, both forms miss the same quotients. So
    # no table can tell a div_ray without it from div_ray (profiles/primitives/mutations.txt, mutant 1).
    for off in SEEDS:
        assert mism(pc.host_call("div_one_correction", [n, a], off=off), pc.host_call("div", [n, a], off=off)) == 0
    dep = short_division(n, a, t.want[1], "ray_div")
    print(f"ray_div: {dep} quotients rest on the hardware's reciprocal of such a divisor")
    assert dep > 0      # the table holds such inputs: the device test pins them

    t3 = pc.div3_table()
    x, y, z, r, _ = t3.planes
    print(f"div3_short: {t3.n} vectors, r over {len(t3.info['r_binades'])} binades ({t3.info['n_neg_r']} negative), "
          f"components over {len(t3.info['n_binades'])}")
    assert set(range(-40, 20)) <= t3.info["r_binades"] <= set(range(-40, 21))
    assert set(range(-100, 21)) <= t3.info["n_binades"] <= set(range(-100, 22))
    assert t3.info["n_neg_r"] > t3.n // 3
    ar = np.abs(r)
    assert np.all((ar >= pc.R_LO) & (ar <= pc.R_HI))
    for c in (x, y, z):
        assert np.all((np.abs(c) >= pc.N_LO) & (np.abs(c) <= pc.N_HI))
    for er in t3.info["edges_r"]:
        for en in t3.info["edges_n"]:
            assert np.any((r == er) & (x == en)), (er, en)
    for en in t3.info["edges_n"]:
        assert np.any(y == en) and np.any(z == en)
    for c, w in zip((x, y, z), t3.want[1:]):
        short_division(c, r, w, "div3_short")

    ts = pc.div3_sqrt_table()
    x, y, z, a, _ = ts.planes
    print(f"div3_short(d, sqrt_scaled(a)): {ts.n} directions, a over {len(ts.info['a_binades'])} binades")
    assert len(ts.info["a_binades"]) >= 70 and ts.n >= 1 << 15
    for off in SEEDS:
        l = pc.host_call("sqrt", [a], off=off)
        for c, w in zip((x, y, z), ts.want[1:]):
            short_division(c, l, w, f"div3_short after sqrt seed {off:+d}")


def test_gate_tables_and_teeth():
    t = pc.ray_div_gate_table()
    a, act, n = t.planes
    fd = t.want[0].reshape(-1, 64)
    names = t.info["names"]
    print(f"ray_div gate: {len(names)} waves over {len(t.info['bad'])} values outside the range")
    assert {"below", "above", "nan", "subnormal_max", "subnormal_min"} <= set(t.info["bad"])
    assert float(t.info["bad"]["below"]).hex() == "0x1.fffffe0000000p-41" and float(t.info["bad"]["above"]).hex() == "0x1.0000020000000p+40"
    cam = [v for k, v in t.info["bad"].items() if k.startswith("subnormal_camera")]
    assert sum(v < pc.FLT_MIN for v in cam) >= 4 and sum(v >= pc.FLT_MIN for v in cam) >= 4 and max(cam) < pc.p2(-119)
    outside = ~((a >= pc.A_LO) & (a <= pc.A_HI))
    for w, (name, lane, on) in enumerate(names):
        sl = slice(64 * w, 64 * w + 64)
        assert np.flatnonzero(outside[sl]).tolist() == [lane] and act[sl][lane] == on
        assert np.all(fd[w] == (0 if on else 1))     # one answer per wave
    for name in t.info["bad"]:
        assert {(lane, on) for nm, lane, on in names if nm == name} == {(l, o) for l in (0, 21, 63) for o in (0, 1)}
    # teeth: the short division with the gate ignored differs from IEEE on part of what the gate refuses
    sub = pc.fb(np.random.default_rng(7).integers(1, 1 << 23, 4096).astype(U))
    num = pc.rnd(np.random.default_rng(8), 4096, -60, 64, True)
    with np.errstate(all="ignore"):
        want = num / sub
    differ = [mism(pc.host_call("div", [num, sub], off=off), want) for off in SEEDS]
    print(f"gate ignored, subnormal a: {differ} of 4096 quotients differ from IEEE (seeds -1, 0, +1)")
    assert all(d > 0 for d in differ)

    tv = pc.div3_vote_table()
    vote = tv.want[0].reshape(-1, 64)
    act = tv.planes[4].reshape(-1, 64)
    print(f"all_lanes_min_abs_ok: {len(tv.info['names'])} waves over {len(pc.VOTE_BAD)} values")
    assert {"zero", "minus_zero", "2^-101", "nan"} <= set(pc.VOTE_BAD)
    comps = np.stack([np.abs(p) for p in tv.planes[:3]])
    bad = ~(comps.min(axis=0) >= pc.N_LO) | np.isnan(comps).any(axis=0)
    for w, (name, comp, lane, on) in enumerate(tv.info["names"]):
        assert np.flatnonzero(bad[64 * w:64 * w + 64]).tolist() == [lane] and act[w][lane] == on
        assert np.all(vote[w][act[w] == 1] == (0 if on else 1)) and np.all(vote[w][act[w] == 0] == 2)
    # teeth: a zero numerator's sign is what the short form can lose
    z = np.full(64, -0.0, dtype=F)
    got = pc.host_call("div", [z, np.full(64, 3, dtype=F)], off=0)
    assert mism(got, z / F(3)) == 64


def test_roots_table():
    t = pc.roots_table()
    b, disc, a = t.planes
    print(f"roots: {t.n} (b, disc, a), a over {len(t.info['a_binades'])} binades, disc over {len(t.info['disc_binades'])}")
    assert t.n >= 1 << 16 and len(t.info["a_binades"]) == 80 and len(t.info["disc_binades"]) >= 120
    for off in SEEDS:
        q = pc.host_call("sqrt", [disc], off=off)
        assert mism(q, t.want[1]) == 0
        short_division(-b - q, a, t.want[0], "near root")
        short_division(-b + q, a, t.want[2], "far root")


@pytest.mark.slow
def test_div_const_table_and_host_check():
    from concurrent.futures import ThreadPoolExecutor
    t = pc.div_const_table()
    a, b, rb = t.planes
    divs = t.info["divisors"]
    print(f"div_const: {t.n} quotients over {len(divs)} divisors")
    assert set(range(1, 4097)) | {65536} <= set(divs)
    for k in (3, 5, 7):
        assert {k << s for s in range(0, 18)} <= set(divs)
    for d in (1, 2, 3, 1280, 4096):      # every pixel index below the divisor, and the draws' ends
        av = set(a[b == d].tolist())
        assert set(range(d)) <= av and {float(pc.CANON_MIN), float(pc.CANON_MAX), 0.0} <= av
    assert np.sum(b == 65536) >= 4096
    # every integer divisor 1..4096 passes the host's check (the library's own function)
    probe.lib()         # loaded (and built, where it is missing) before the threads ask for it
    with ThreadPoolExecutor(16) as ex:
        fast = dict(zip(divs, ex.map(probe.exact_by_reciprocal, [float(d) for d in divs])))
    assert all(fast[d] for d in range(1, 4097)), [d for d in range(1, 4097) if not fast[d]][:8]
    # and so does every other divisor of the table: the device test runs them all with fast on and off
    assert all(fast.values()), [d for d in divs if not fast[d]]
    print(f"exact_by_reciprocal: {sum(fast.values())} of {len(divs)} divisors pass")
    ok = np.array([fast[int(d)] for d in divs])[np.searchsorted(np.array(divs), b.astype(np.int64))]
    got = pc.host_call("div_const", [a, b, rb])
    assert mism(got, t.want[0], ok) == 0


def test_sphere_table():
    t = pc.sphere_table()
    i = t.info
    cls, want, tag = i["cls"], i["lane_want"], i["tag"]
    print(f"sphere_key: {t.n} lanes in {t.n // 64} waves; classes none/near/far/out of range: "
          f"{[int((cls == k).sum()) for k in range(4)]}; tags {dict(zip(*np.unique(tag, return_counts=True)))}")
    for name in ("outside", "inside", "surface", "away", "tangent0", "tangent+", "near_kmin", "far_kmin"):
        assert np.sum(tag == name) >= 30, name
    assert np.all(i["disc"][tag == "tangent0"] == 0) and np.all(i["disc"][tag == "tangent+"] > 0)
    sw = t.planes[4]
    assert np.sum(sw == 0) >= 16                       # zero radius; a negative one has the positive's r r
    assert sorted(set(i["off_near"].tolist())) == [-2, -1, 0, 1, 2] == sorted(set(i["off_far"].tolist()))
    nk = tag == "near_kmin"
    assert set((pc.bf(i["t1"][nk]).astype(np.int64) - pc.KMIN_BITS).tolist()) == {-2, -1, 0, 1, 2}
    assert np.all(cls[nk & (pc.bf(i["t1"]) > pc.KMIN_BITS)] == 1) and np.all(cls[nk & (pc.bf(i["t1"]) <= pc.KMIN_BITS)] == 2)
    fk = tag == "far_kmin"
    assert np.all(cls[fk & (pc.bf(i["t2"]) > pc.KMIN_BITS)] == 2) and np.all(cls[fk & (pc.bf(i["t2"]) <= pc.KMIN_BITS)] == 3)
    # the waves of the two uniform early-outs
    pos = ((cls != 0) & (want == 1)).reshape(-1, 64).sum(axis=1)
    far = (((cls == 2) | (cls == 3)) & (want == 1)).reshape(-1, 64).sum(axis=1)
    for name, cnt, k in (("no lane positive", pos, 0), ("one lane positive", pos, 1),
                         ("all lanes positive, none needs the far root", pos, 64),
                         ("all lanes positive, none needs the far root", far, 0),
                         ("one lane needs the far root", far, 1), ("all lanes need the far root", far, 64)):
        ws = [w for w, nm in enumerate(i["wave_names"]) if nm == name]
        assert len(ws) >= 4 and all(cnt[w] == k for w in ws), (name, [cnt[w] for w in ws])
    assert np.all(i["key"][want == 0] == pc.KNOHIT)
    assert np.sum((want == 0) & (cls == 1)) >= 100     # lanes that do not ask and would have a candidate
    assert np.sum(i["key"] != pc.KNOHIT) >= 2000


def test_in_range_and_min16_tables():
    t = pc.in_range_table()
    bits = t.planes[0]
    print(f"in_range: {t.n} patterns, {t.info['n_near']} within 2^12 of an anchor, {t.info['n_true']} in range")
    have = set(bits[:t.info["n_near"]].tolist())
    for a in pc.IN_RANGE_ANCHORS:
        assert {(a + k) % (1 << 32) for k in (-4096, -1, 0, 1, 4096)} <= have
    assert t.n >= 1 << 20
    assert mism(pc.host_call("in_range", [bits], out_dtype=U), t.want[0]) == 0
    # teeth: the same compare with lo in place of lo + 1 admits kMIN itself
    assert t.want[0][bits == pc.KMIN_BITS][0] == 0 and t.want[0][bits == pc.KMIN_BITS + 1][0] == 1
    assert t.want[0][bits == pc.KMAX_BITS][0] == 0 and t.want[0][bits == pc.KMAX_BITS - 1][0] == 1

    m = pc.min16_table()
    names = m.info["row_names"]
    print(f"min16_key: {len(names)} rows in {m.n // 64} waves")
    for p in range(16):
        assert f"min at {p}" in names and f"equal t, smallest index at {p}" in names
    for nm in ("all no hit", "nan keys only", "nan keys and one hit", "all lanes equal"):
        assert nm in names and nm + ", smaller keys in the neighbouring rows" in names
    keys = m.info["keys"].reshape(-1, 16)
    want = probe.join64(m.want[0], m.want[1]).reshape(-1, 16)
    assert np.all(want == keys.min(axis=1)[:, None])
    # the two passes are not independent: in some rows the smallest index is not at the smallest t
    tb, ix = keys >> np.uint64(32), keys & np.uint64(0xFFFFFFFF)
    assert np.sum(ix.min(axis=1) != (want[:, 0] & np.uint64(0xFFFFFFFF))) >= 32
    for r, nm in enumerate(names):
        if nm.endswith("neighbouring rows"):
            nb = [r + d for d in (-1, 1) if 0 <= r + d < len(names) and (r + d) // 4 == r // 4]
            assert nb and all(keys[q].max() < keys[r].min() for q in nb)


def test_pcg_and_canonical_tables():
    tc, tp = pc.canonical_table()
    w = tc.info["words"]
    chosen = tc.info["chosen"]
    print(f"canonical: {tc.n} states, {len(chosen)} with a chosen word, {int((w >= (1 << 32) - 128).sum())} in the clamp")
    assert np.all(w[:len(chosen)] == chosen.astype(U))          # the inversion gives the chosen words
    assert set(pc.CHOSEN_WORDS) <= set(w.tolist())
    f = w.astype(F)
    assert np.sum(f.astype(np.float64) > w) >= 100 and np.sum(f == F(4294967296.0)) >= 30
    top = w >= (1 << 32) - 128
    assert np.all(pc.fb(tc.want[0])[top] == pc.CANON_MAX) and np.all(f[top] == F(4294967296.0))
    assert np.all(f[w == (1 << 32) - 129] < F(4294967296.0))
    assert np.all(pc.fb(tc.want[0]) < 1) and np.all(pc.fb(tp.want[0]) < 1) and np.all(pc.fb(tp.want[0]) >= -1)
    c, pm1 = pc.host_call("canonical", [w], n_out=2)
    assert mism(c, tc.want[0]) == 0 and mism(pm1, tp.want[0]) == 0
    # teeth: without the clamp the top words give 1
    assert np.all((f * F(2.0 ** -32))[top] == 1)
    # PCG32 against Python integers
    ts = pc.pcg_stream_table()
    print(f"pcg streams: {ts.n}, {ts.info['n_wide_init']} keys and {ts.info['n_wide_inc']} increments past 2^32")
    assert ts.info["n_wide_init"] >= 512 and ts.info["n_wide_inc"] >= 512
    init, inc = probe.join64(*ts.planes[0:2]), probe.join64(*ts.planes[2:4])
    for lane in (0, 65, 700, ts.n - 1):
        i, st = int(inc[lane]), 0
        st = (st * pc.PCG_MUL + i) & pc.M64
        st = (st + int(init[lane])) & pc.M64
        st = (st * pc.PCG_MUL + i) & pc.M64
        for j in range(pc.PCG_DRAWS):
            xs = (((st >> 18) ^ st) >> 27) & 0xFFFFFFFF
            rot = st >> 59
            assert int(ts.want[j][lane]) == ((xs >> rot) | (xs << ((-rot) & 31))) & 0xFFFFFFFF
            st = (st * pc.PCG_MUL + i) & pc.M64
        assert st == int(probe.join64(ts.want[-2], ts.want[-1])[lane])


def test_unit_sphere_table():
    t = pc.unit_sphere_table()
    k = t.info["k"]
    counts = np.bincount(k, minlength=8)
    print(f"random_in_unit_sphere: {t.n} states, by rejected attempts {counts.tolist()}")
    assert len(counts) == 8 and np.all(counts >= 8)
    assert all(len(set(k[w:w + 64].tolist())) >= 4 for w in range(0, t.n, 64))   # waves whose lanes differ
    p = [pc.fb(t.want[c]) for c in range(3)]
    assert np.all(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] <= F(1.0000002))
    assert set(t.want[5].tolist()) == {1, 2}


def test_refract_normalize_schlick_tables():
    t = pc.refract_table()
    i = t.info
    print(f"refract: {t.n} cases, k = 0: {i['n_zero']}, k < 0: {i['n_neg']}, k = 1: {i['n_one']}, "
          f"smallest positive k {i['k_min_pos']:.3g} ({i['n_min_pos']} times)")
    assert i["n_zero"] >= 8 and i["n_neg"] >= 1000 and i["n_one"] >= 8 and i["k_min_pos"] == 2.0 ** -24 and i["n_min_pos"] >= 8
    neg = i["k"] < 0
    assert all(np.all(w[neg] == pc.QNAN) for w in t.want)      # every component NaN, as the reference has it
    assert all(np.all(w[~neg] != pc.QNAN) for w in t.want)
    # the kernel's form: the scaled root and a select instead of the multiplication by the flag
    I, N, eta = t.planes[0:3], t.planes[3:6], t.planes[6]
    for off in SEEDS:
        with np.errstate(all="ignore"):
            d = N[0] * I[0] + N[1] * I[1] + N[2] * I[2]
            s = pc.host_call("sqrt", [i["k"]], off=off)
            for c in range(3):
                got = (I[c] * eta - (N[c] * s + d * eta)) * np.where(i["k"] >= 0, F(1), F(0))
                # (the root of k = 0 is the hardware's exact 0: it has no neighbours)
                assert mism(got, t.want[c], None if off == 0 else i["k"] != 0) == 0

    tn =pc.normalize_table()
    print(f"normalize: {tn.n} vectors, {tn.info['n_zero_len']} of length 0, smallest other length {tn.info['min_len']:.3g}, "
          f"{tn.info['n_small']} below 2^-70")
    assert tn.info["n_zero_len"] >= 100 and tn.info["min_len"] == float(np.sqrt(F(2.0 ** -149))) and tn.info["n_small"] >= 100

    ts = pc.schlick_table()
    xf, c = ts.planes
    print(f"schlick_x: {ts.n} (index, cosine) pairs over {len(ts.info['ris'])} indices")
    assert len(ts.info["ris"]) == 12 and ts.n <= 1 << 20 and len(np.unique(xf)) >= 11
    for x in np.unique(xf):
        cs = set(pc.bf(c[xf == x]).tolist())
        one = pc.bits1(1.0)
        assert {0, 1, 1024, one, one - 1024, one + 1024} <= cs
    assert mism(pc.host_call("schlick", [xf, c]), ts.want[0]) == 0
    sl = slice(0, None, 97)                                      # the C tool's reference against math.pow
    assert mism(pc.schlick_py(xf[sl], c[sl]), ts.want[0][sl]) == 0


def test_udiv_table():
    t = pc.udiv_table(probe.make_udiv)
    n, m, s1, s2 = t.planes
    d = t.info["divisors"]
    print(f"udiv: {t.n} (n, d) pairs over {len(set(d.tolist()))} divisors")
    assert {1, 2, 3, 5, 7, 64, 1280 * 720, 1 << 31, (1 << 32) - 1} <= set(d.tolist())
    assert all({(1 << k) - 1, (1 << k) + 1} <= set(d.tolist()) for k in range(2, 32))
    for dv in (1, 7, 1280 * 720, (1 << 32) - 1):
        nv = set(n[d == dv].tolist())
        assert {0, dv - 1, dv, (1 << 32) - 1} <= nv
    assert np.all(t.want[0] == (n.astype(np.uint64) // d.astype(np.uint64)).astype(U))
    assert mism(pc.host_call("udiv", [n, m, s1, s2], out_dtype=U), t.want[0]) == 0
