"""TEST INFRASTRUCTURE: the input tables of the device-function probes (tests/device/rt_probe.hip)
and their expected outputs, fixed on the CPU: seeded numpy, every expected value from a plain
reference (numpy float32 operations, one rounding each, for /, sqrt and the vector formulas;
float64 and the C library's pow for Schlick; Python integers for udiv and the key minima; a short
PCG32 for the draws). tests/test_primitives_cpu.py proves the tables are what they claim,
tests/test_primitives_gpu.py runs them on the device.

A table is a Table: `planes` (the probe's input planes, length a multiple of 64: the probes run whole
waves), `want` (the expected output planes as uint32 words; floats by their bits, every NaN as
QNAN), `mask` (per output plane: the lanes that are compared, None = all) and `info` (coverage
counts, asserted and printed by the CPU module).
"""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F = np.float32
U = np.uint32
QNAN = 0x7FC00000
KMIN_BITS, KMAX_BITS = 0x3C03126F, 0x7F7FFFFF
KMIN, KMAX = np.array([KMIN_BITS, KMAX_BITS], dtype=U).view(F)
KNOHIT = 0x7F7FFFFFFFFFFFFF
FLT_MIN = F(2.0 ** -126)
PCG_MUL = 6364136223846793005
M64 = (1 << 64) - 1


class Table:
    def __init__(self, planes, want, mask=None, **info):
        self.planes = [np.ascontiguousarray(p) for p in planes]
        self.is_float = [np.asarray(w).dtype == np.float32 for w in want]   # integer planes are compared raw
        self.want = [canon(w) if f else np.ascontiguousarray(w, dtype=U) for w, f in zip(want, self.is_float)]
        self.mask = list(mask) if mask is not None else [None] * len(self.want)
        self.info = info
        self.n = len(self.planes[0])
        assert self.n % 64 == 0 and all(len(p) == self.n for p in self.planes + self.want)


def fb(bits):
    return np.ascontiguousarray(bits, dtype=U).view(F)


def bf(x):
    return np.ascontiguousarray(x, dtype=F).view(U)


def canon(w):
    """Output words with every NaN as QNAN (the reference's NaN and the device's differ in sign and
    payload; what the callers read is that it is one)."""
    w = np.ascontiguousarray(w)
    if w.dtype == np.float32:
        w = w.view(U)
    w = w.astype(U).copy()
    w[(w & U(0x7FFFFFFF)) > U(0x7F800000)] = QNAN
    return w


def p2(e):
    return F(2.0 ** e)


def bits1(x):
    return int(bf([x])[0])


def f1(bits):
    return fb([bits])[0]


def up(x, k=1):
    """x moved k ulps away from zero (towards it for negative k)."""
    x = np.asarray(x, dtype=F)
    r = (x.reshape(-1).view(U).astype(np.int64) + k).astype(U).view(F).reshape(x.shape)
    return r[()] if x.ndim == 0 else r


def rnd(rng, n, e_lo, e_hi, signed=False):
    """n normal floats: seeded mantissa, exponent uniform in [e_lo, e_hi)."""
    e = rng.integers(e_lo, e_hi, n, dtype=np.int64)
    b = ((e + 127) << 23) | rng.integers(0, 1 << 23, n, dtype=np.int64)
    if signed:
        b |= rng.integers(0, 2, n, dtype=np.int64) << 31
    return fb(b.astype(U))


def pad64(arrs):
    """Elementwise tables as whole waves: element 0 repeated."""
    n = len(arrs[0])
    m = -n % 64
    return [np.concatenate([a, np.repeat(a[:1], m)]) for a in arrs]


def binades(x):
    x = np.abs(np.asarray(x, dtype=np.float64))
    return set(np.floor(np.log2(x[(x > 0) & np.isfinite(x)])).astype(int).tolist())


# ---- the host restatement (tests/tools/probe_host.cpp) ------------------------------------------
_host = None


def host():
    global _host
    if _host is None:
        out = os.path.join(REPO, "tests", "tools", "_build", "libprobe_host.so")
        src = os.path.join(REPO, "tests", "tools", "probe_host.cpp")
        if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            tmp = f"{out}.{os.getpid()}.tmp"
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-fPIC",
                            "-shared", "-o", tmp, src], check=True)
            os.replace(tmp, out)
        _host = C.CDLL(out)
    return _host


def host_call(name, ins, n_out=1, off=None, out_dtype=F):
    """ph_<name> on 32-bit arrays of one length; returns its output array(s)."""
    ins = [np.ascontiguousarray(a) for a in ins]
    n = len(ins[0])
    outs = [np.empty(n, dtype=out_dtype) for _ in range(n_out)]
    args = [a.ctypes.data_as(C.c_void_p) for a in ins] + [C.c_size_t(n)]
    if off is not None:
        args.append(C.c_int(off))
    args += [o.ctypes.data_as(C.c_void_p) for o in outs]
    f = getattr(host(), "ph_" + name)
    f.restype = None
    f(*args)
    return outs[0] if n_out == 1 else outs


# ---- sqrt_scaled ------------------------------------------------------------------------------------
@functools.lru_cache(None)
def sqrt_table():
    rng = np.random.default_rng(0x5157)
    parts = []
    for e in range(-149, 96):
        if e >= -126:
            base, span = (e + 127) << 23, 1 << 23
        else:
            base = span = 1 << (e + 149)
        m = np.concatenate([np.arange(min(64, span)), span - 1 - np.arange(min(64, span)),
                            rng.integers(0, span, 128)])
        parts.append(base + np.unique(m))
    binade_bits = np.concatenate(parts).astype(U)
    # squares of 24-bit s and their neighbours, which straddle the rounding midpoints of the root
    s = (rng.integers(1 << 23, 1 << 24, 1 << 14).astype(np.float64) * 2.0 ** rng.integers(-70, 24, 1 << 14)).astype(F)
    sq = bf(s * s).astype(np.int64)
    squares = np.concatenate([sq + k for k in (-2, -1, 0, 1, 2)]).astype(U)
    special = np.array([0, bits1(-1.0), bits1(-2.0 ** -149), 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001], dtype=U)
    x = fb(np.concatenate([special, binade_bits, squares]))
    assert np.all((x[len(special):] > 0) & (x[len(special):] < p2(96)))
    (x,) = pad64([x])
    with np.errstate(all="ignore"):
        want = np.sqrt(x)
    assert want.dtype == np.float32
    return Table([x], [want], binades=binades(fb(binade_bits)), n_binade=len(binade_bits), n_square=len(squares),
                 n_special=len(special), special=special)


# ---- ray_div / div_ray ----------------------------------------------------------------------------------
A_LO, A_HI = p2(-40), p2(40)


def _div_edges():
    ea = np.array([A_LO, up(A_LO), up(A_HI, -1), A_HI], dtype=F)
    en = np.array([p2(-60), up(p2(-60)), up(p2(64), -2), up(p2(64), -1)], dtype=F)
    en = np.concatenate([en, -en])
    return ea, en


@functools.lru_cache(None)
def seed_sensitive_mantissas():
    """The 24-bit divisor mantissas for which the reciprocal refined from a seed one ulp off the correctly
    rounded one is not the one refined from that (which is RN(1 / a) for every mantissa): 0xffffff from the
    seed below, and some thirty from the seed above."""
    am = np.arange(1 << 23, 1 << 24, dtype=F)
    y0 = host_call("rcp", [am], off=0)
    assert np.array_equal(y0, F(1) / am)
    out = set()
    for off in (-1, 1):
        out |= set(am[host_call("rcp", [am], off=off) != y0].astype(np.int64).tolist())
    return sorted(out)


@functools.lru_cache(None)
def ray_div_table():
    """Quotients on a in [2^-40, 2^40], |n| in [2^-60, 2^64): every lane active, fd = 1."""
    rng = np.random.default_rng(0xD1)
    ea, en = _div_edges()
    n_r = (1 << 18) - 64
    a = np.concatenate([np.repeat(ea, len(en)), rnd(rng, n_r, -40, 40), np.repeat(ea, 2048)])
    n = np.concatenate([np.tile(en, len(ea)), rnd(rng, n_r, -60, 64, True), rnd(rng, 4 * 2048, -60, 64, True)])
    # the divisors whose refined reciprocal depends on the seed, over the range, with the numerators that are
    # hardest to round there (powers of two, 0xd55553) and seeded ones
    sm = np.array(seed_sensitive_mantissas(), dtype=np.float64)
    es = np.array([-63, -56, -48, -40, -32, -24, -16, -8, 0, 8, 15], dtype=np.float64)     # a = m 2^e in [2^-40, 2^39)
    sa = (sm[:, None] * 2.0 ** es[None, :]).astype(F).ravel()
    hard = np.concatenate([[p2(-60), -p2(-60), p2(0), p2(63), fb([0x4B555553 - (40 << 23)])[0], -fb([0x4B555553])[0]],
                           rnd(rng, 18, -60, 64, True)]).astype(F)
    a = np.concatenate([a, np.repeat(sa, len(hard))])
    n = np.concatenate([n, np.tile(hard, len(sa))])
    a, n = pad64([a, n])
    act = np.ones(len(a), dtype=U)
    with np.errstate(all="ignore"):
        q = n / a
    # rd.y: the reciprocal refined from the correctly rounded seed (the host restatement)
    return Table([a, act, n], [np.ones(len(a), dtype=U), q, host_call("rcp", [a], off=0)], a_binades=binades(a),
                 n_binades=binades(n), edges_a=ea, edges_n=en, sensitive=sa)


GATE_BAD = {
    "below": up(A_LO, -1), "above": up(A_HI), "nan": f1(QNAN), "subnormal_max": f1(0x007FFFFF),
    "subnormal_min": f1(1), "zero": F(0), "inf": F(np.inf), "negative": F(-1),
}


@functools.lru_cache(None)
def ray_div_gate_table():
    """Waves with one lane outside the gate's range; want fd per lane (the wave's answer) and the
    quotient where fd is 1 and the lane is active."""
    rng = np.random.default_rng(0x6A7E)
    bad = dict(GATE_BAD)
    # the `subnormal` camera's a = |d|^2 (focus distance 2^-63.5: about 2^-127, half of them subnormal)
    for k, v in enumerate(rnd(rng, 8, -126, -120).tolist() + fb(rng.integers(1, 1 << 23, 8).astype(U)).tolist()):
        bad[f"subnormal_camera_{k}"] = F(v)
    names, a_w, act_w, fd_w = [], [], [], []
    for name, v in bad.items():
        for lane in (0, 21, 63):
            for on in (1, 0):
                a = rnd(rng, 64, -40, 40)
                act = rng.integers(0, 2, 64).astype(U)
                a[lane], act[lane] = v, on
                names.append((name, lane, on))
                a_w.append(a)
                act_w.append(act)
                fd_w.append(np.full(64, 0 if on else 1, dtype=U))
    a, act, fd = np.concatenate(a_w), np.concatenate(act_w), np.concatenate(fd_w)
    n = rnd(rng, len(a), -60, 64, True)
    with np.errstate(all="ignore"):
        q = n / a
        in_dom = (a >= A_LO) & (a <= A_HI)
    return Table([a, act, n], [fd, q, host_call("rcp", [a], off=0)], [None, (fd == 1) & (act == 1) & in_dom, in_dom],
                 names=names, bad=bad)


# ---- near_root / far_root -------------------------------------------------------------------------------
@functools.lru_cache(None)
def roots_table():
    rng = np.random.default_rng(0x2007)
    n = 1 << 18
    a = rnd(rng, n, -40, 40)
    b = rnd(rng, n, -30, 44, True)
    disc = rnd(rng, n, -60, 96)
    # half of them with the root near |b|, as a ray from outside a sphere has it
    half = slice(0, n // 2)
    with np.errstate(all="ignore"):
        disc[half] = (b[half] * b[half]) * rnd(rng, n // 2, -24, 0)
        q = np.sqrt(disc)
        nn, nf = -b - q, -b + q
        keep = (disc > 0) & (disc < p2(96))
        for x in (nn, nf):
            keep &= (np.abs(x) >= p2(-60)) & (np.abs(x) < p2(64))
        a, b, disc, q, nn, nf = pad64([v[keep] for v in (a, b, disc, q, nn, nf)])
        near, far = nn / a, nf / a
    return Table([b, disc, a], [near, q, far, near, q, far], a_binades=binades(a), disc_binades=binades(disc))


# ---- div3_short, all_lanes_min_abs_ok ---------------------------------------------------------------------
R_LO, R_HI, N_LO, N_HI = p2(-40), p2(20), p2(-100), p2(21)


@functools.lru_cache(None)
def div3_table():
    """n / r on |r| in [2^-40, 2^20] (both signs), |n_i| in [2^-100, 2^21]: every lane active."""
    rng = np.random.default_rng(0xD3)
    er = np.array([R_LO, up(R_LO), up(R_HI, -1), R_HI], dtype=F)
    er = np.concatenate([er, -er])
    en = np.array([N_LO, up(N_LO), up(N_HI, -1), N_HI], dtype=F)
    en = np.concatenate([en, -en])
    m = 1 << 17
    r = np.concatenate([np.repeat(er, 64), rnd(rng, m, -40, 20, True), np.repeat(er, 512)])
    comps = []
    for c in range(3):
        edge = np.tile(np.roll(en, c), 64)
        comps.append(np.concatenate([edge, rnd(rng, m, -100, 21, True), rnd(rng, 8 * 512, -100, 21, True)]))
    comps[0][512 + m:] = np.tile(en, 512)   # every edge component over every edge divisor
    r, x, y, z = pad64([r] + comps)
    with np.errstate(all="ignore"):
        want = [x / r, y / r, z / r]
    one = np.ones(len(r), dtype=U)
    return Table([x, y, z, r, one], [one] + want, r_binades=binades(r), n_binades=binades(np.concatenate([x, y, z])),
                 n_neg_r=int((r < 0).sum()), edges_r=er, edges_n=en)


@functools.lru_cache(None)
def div3_sqrt_table():
    """d / sqrt(a), a = |d|^2 in [2^-40, 2^40], as the render loop's unit direction composes it."""
    rng = np.random.default_rng(0xD35)
    m = 1 << 16
    s = p2(0) * (2.0 ** rng.integers(-20, 20, m)).astype(F)
    d = [(rng.uniform(-1, 1, m).astype(F)) * s for _ in range(3)]
    with np.errstate(all="ignore"):
        a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        keep = (a >= A_LO) & (a <= A_HI)
        for c in d:
            keep &= np.abs(c) >= N_LO
        x, y, z, a = pad64([v[keep] for v in d + [a]])
        l = np.sqrt(a)
        want = [x / l, y / l, z / l]
    one = np.ones(len(a), dtype=U)
    return Table([x, y, z, a, one], [one] + want, a_binades=binades(a))


VOTE_BAD = {"zero": F(0), "minus_zero": F(-0.0), "2^-101": p2(-101), "below": up(N_LO, -1), "nan": f1(QNAN),
            "-2^-101": -p2(-101)}


@functools.lru_cache(None)
def div3_vote_table():
    rng = np.random.default_rng(0x707E)
    names, rows = [], []
    for name, v in VOTE_BAD.items():
        for comp in range(3):
            for lane in (0, 40, 63):
                for on in (1, 0):
                    n = [rnd(rng, 64, -100, 21, True) for _ in range(3)]
                    act = rng.integers(0, 2, 64).astype(U)
                    n[comp][lane], act[lane] = v, on
                    names.append((name, comp, lane, on))
                    rows.append((n[0], n[1], n[2], rnd(rng, 64, -40, 20, True), act,
                                 np.where(act == 1, U(0 if on else 1), U(2))))
    x, y, z, r, act, vote = [np.concatenate(c) for c in zip(*rows)]
    with np.errstate(all="ignore"):
        want = [x / r, y / r, z / r]
    ok = vote == 1
    return Table([x, y, z, r, act], [vote] + want, [None, ok, ok, ok], names=names)


# ---- div_const ------------------------------------------------------------------------------------------
def div_const_divisors():
    d = list(range(1, 4097)) + [65536]
    for k in (3, 5, 7):
        v = k
        while v <= 1 << 20:
            d.append(v)
            v *= 2
    return sorted(set(d))


CANON_MIN, CANON_MAX = p2(-32), f1(0x3F7FFFFF)


@functools.lru_cache(None)
def div_const_table():
    """a over 0, every pixel index below the divisor (at most 4096 of them, seeded above that), the
    smallest and largest canonical draw and index + draw sums, for every divisor. Every index below each
    of 1..4096 is 8.4 million quotients by itself, so this one table is eight times the 2^20 entries the
    others keep to (8.55 million in all); the kernel is one division per lane, and the device test, with
    both of its passes and this table's construction, takes half a second. The CPU module's check of it
    is marked slow."""
    rng = np.random.default_rng(0xDC)
    divs = div_const_divisors()
    a_parts, b_parts = [], []
    for d in divs:
        idx = np.arange(d) if d <= 4096 else np.unique(np.concatenate([[0, 1, d - 2, d - 1], rng.choice(d, 4092, replace=False)]))
        idx = idx.astype(F)
        pick = idx[rng.integers(0, len(idx), 6)]
        draws = np.array([CANON_MIN, CANON_MAX, up(CANON_MIN), p2(-1), p2(-24), f1(int(rng.integers(0x2F800000, 0x3F800000)))],
                         dtype=F)
        a = np.concatenate([idx, draws, pick + draws, [F(d - 1) + CANON_MAX, F(d - 1) + CANON_MIN]]).astype(F)
        a_parts.append(a)
        b_parts.append(np.full(len(a), d, dtype=F))
    a, b = pad64([np.concatenate(a_parts), np.concatenate(b_parts)])
    rb = F(1) / b
    return Table([a, b, rb], [a / b], divisors=divs)


# ---- sphere_key<false> ------------------------------------------------------------------------------------
def sphere_ref(want, s, sid, o, d):
    """raytracer.hxx:52-90 on the geo entry s = {C, fl(r r)}, float32 op for op in the reference's
    order, as a key bits(t) << 32 | id, KNOHIT without a candidate. Returns key and a class per
    lane: 0 no positive discriminant, 1 near root, 2 far root, 3 positive but no root in range."""
    with np.errstate(all="ignore"):
        ocx, ocy, ocz = o[0] - s[0], o[1] - s[1], o[2] - s[2]
        a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        b = ocx * d[0] + ocy * d[1] + ocz * d[2]
        c = ocx * ocx + ocy * ocy + ocz * ocz - s[3]
        disc = b * b - a * c
        pos = disc > 0
        q = np.sqrt(np.where(pos, disc, F(1)))
        t1 = (-b - q) / a
        t2 = (-b + q) / a
        ok1 = pos & (t1 < KMAX) & (t1 > KMIN)
        ok2 = pos & ~ok1 & (t2 < KMAX) & (t2 > KMIN)
    t = np.where(ok1, t1, t2)
    assert a.dtype == b.dtype == c.dtype == disc.dtype == t.dtype == np.float32
    cls = np.where(ok1, 1, np.where(ok2, 2, np.where(pos, 3, 0)))
    key = np.where((want != 0) & (ok1 | ok2), (bf(t).astype(np.uint64) << np.uint64(32)) | sid.astype(np.uint64),
                   np.uint64(KNOHIT))
    return key, cls, disc, t1, t2


def _axis(cases, perm):
    """The coordinates of (s, o, d) cases permuted (zeros elsewhere: the same arithmetic)."""
    s, o, d = cases
    return [s[perm[0]], s[perm[1]], s[perm[2]], s[3]], [o[p] for p in perm], [d[p] for p in perm]


def _near_kmin(far):
    """Rays along z from the origin at a sphere on the axis whose near (far: far) root lies within 2 ulp
    of kMIN, found by scanning the bit patterns of the centre and the radius."""
    r0, c0 = (0.012, -0.004) if far else (0.004, 0.012)
    r = fb(bf(F(r0)).astype(np.int64) + np.arange(256))[:, None] + np.zeros((1, 4096), dtype=F)
    cz = fb(bf(F(c0)).astype(np.int64) + np.arange(-2048, 2048))[None, :] + np.zeros((256, 1), dtype=F)
    r, cz = r.ravel(), cz.ravel()
    z, one = np.zeros_like(r), np.ones_like(r)
    s, o, d = [z, z, cz, r * r], [z, z, z], [z, z, one]
    _, cls, _, t1, t2 = sphere_ref(one, s, np.zeros(len(r), dtype=U), o, d)
    off = bf(t2 if far else t1).astype(np.int64) - KMIN_BITS
    pick = []
    for k in (-2, -1, 0, 1, 2):
        hit = np.flatnonzero(off == k)[:24]
        assert len(hit) >= 8, (far, k, len(hit))
        pick.append(hit)
    pick = np.concatenate(pick)
    return [[v[pick] for v in s], [v[pick] for v in o], [v[pick] for v in d]], off[pick]


@functools.lru_cache(None)
def sphere_table():
    rng = np.random.default_rng(0x5BE2E)
    m = 4096
    u = lambda k: rng.uniform(-1, 1, k).astype(F)
    unit = lambda k: (lambda v: [c / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) for c in v])([u(k), u(k), u(k)])
    C = [u(m) * F(11), rng.uniform(0.2, 1, m).astype(F), u(m) * F(11)]
    r = np.where(rng.random(m) < 0.2, F(1), F(0.2)).astype(F)
    r[rng.random(m) < 0.1] *= F(-1)                      # the hollow ball's negative radius
    r[:32] = 0                                            # a zero radius
    dirn = unit(m)
    scale = rng.choice(np.array([1, 1, 1, 0.125, 10, 1e-4, 3e4], dtype=F), m)
    kind = rng.integers(0, 5, m)
    w = unit(m)
    dist = rng.uniform(1.5, 20, m).astype(F)
    ar = np.abs(r)
    o = []
    for c in range(3):
        outside = C[c] - dirn[c] * dist + w[c] * ar * F(0.9)    # aimed near the sphere, some missing
        inside = C[c] + w[c] * ar * F(0.5)
        surface = C[c] + w[c] * ar                                 # as after a bounce off it
        away = C[c] + dirn[c] * dist                               # pointing away
        o.append(np.select([kind == 0, kind == 1, kind == 2, kind == 3], [outside, inside, surface, away], outside).astype(F))
    d = [dirn[c] * scale for c in range(3)]
    pool = ([C[0], C[1], C[2], r * r], o, d)
    tags = [np.array(["outside", "inside", "surface", "away", "outside"])[kind]]
    # tangent rays: disc exactly 0, and the smallest positive disc the centre's bits allow
    z1 = np.zeros(64, dtype=F)
    rr = (2.0 ** rng.integers(-3, 4, 64)).astype(F)
    cz = rr * F(2)
    tang0 = ([rr, z1, cz, rr * rr], [z1, z1, z1], [z1, z1, z1 + 1])
    cx = rr.copy()
    for i in range(64):   # the first centre below r, in bit order, that gives a positive discriminant
        cand = fb(bf(rr[i:i + 1]).astype(np.int64) - np.arange(1, 64))
        zz = np.zeros(63, dtype=F)
        _, _, disc, _, _ = sphere_ref(zz + 1, [cand, zz, zz + cz[i], zz + rr[i] * rr[i]], zz.astype(U), [zz, zz, zz], [zz, zz, zz + 1])
        cx[i] = cand[np.flatnonzero(disc > 0)[0]]
    tang1 = ([cx, z1, cz, rr * rr], [z1, z1, z1], [z1, z1, z1 + 1])
    kn, off_n = _near_kmin(False)
    kf, off_f = _near_kmin(True)
    groups = [pool, tang0, tang1, kn, kf]
    gtags = ["pool", "tangent0", "tangent+", "near_kmin", "far_kmin"]
    parts = [_axis(g, [(0, 1, 2), (2, 0, 1), (1, 2, 0)][k % 3] if k else (0, 1, 2)) for k, g in enumerate(groups)]
    s = [np.concatenate([p[0][c] for p in parts]).astype(F) for c in range(4)]
    o = [np.concatenate([p[1][c] for p in parts]).astype(F) for c in range(3)]
    d = [np.concatenate([p[2][c] for p in parts]).astype(F) for c in range(3)]
    tag = np.concatenate([np.full(len(p[0][0]), t) if t != "pool" else tags[0] for p, t in zip(parts, gtags)])
    n_case = len(s[0])
    sid = rng.integers(0, 1 << 31, n_case).astype(U)
    _, cls, disc, t1, t2 = sphere_ref(np.ones(n_case), s, sid, o, d)
    by = {k: np.flatnonzero((cls == k) & (tag != "near_kmin") & (tag != "far_kmin")) for k in range(4)}
    pick = lambda k, cnt: rng.choice(by[k], cnt)
    nopos = lambda cnt: rng.choice(by[0], cnt)
    waves, wnames = [], []

    def wave(name, idx, want=None):
        wnames.append(name)
        waves.append((np.asarray(idx), np.ones(64, dtype=U) if want is None else want))

    some = (rng.random(64) < 0.5).astype(U)
    for rep in range(4):
        wave("no lane positive", nopos(64))
        wave("one lane positive", np.concatenate([nopos(rep * 20), pick(1, 1), nopos(63 - rep * 20)]))
        wave("all lanes positive, none needs the far root", pick(1, 64))
        wave("one lane needs the far root", np.concatenate([pick(1, 63 - rep * 20), pick(2, 1), pick(1, rep * 20)]))
        wave("all lanes need the far root", pick(2, 64))
        wave("positive, no root in range", np.concatenate([pick(3, 32), pick(1, 32)]))
        wave("want false among true", rng.integers(0, n_case, 64), (rng.random(64) < 0.5).astype(U))
        wave("no lane wants", pick(1, 64), np.zeros(64, dtype=U))
        wave("one lane wants", pick(2, 64), (np.arange(64) == 17 * rep).astype(U))
    rest = np.concatenate([np.arange(n_case), rng.integers(0, n_case, -n_case % 64)])   # every case once
    for k in range(0, len(rest), 64):
        wave("every case", rest[k:k + 64], None if (k // 64) % 4 else (rng.random(64) < 0.8).astype(U))
    idx = np.concatenate([w[0] for w in waves])
    want = np.concatenate([w[1] for w in waves])
    s, o, d = [v[idx] for v in s], [v[idx] for v in o], [v[idx] for v in d]
    sid = sid[idx]
    key, cls, disc, t1, t2 = sphere_ref(want, s, sid, o, d)
    with np.errstate(all="ignore"):
        a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    assert np.all((a >= A_LO) & (a <= A_HI))   # the short forms' range: fd follows fast_roots
    return Table([want] + s + [sid] + o + d, [key & np.uint64(0xFFFFFFFF), key >> np.uint64(32)],
                 tag=tag[idx], cls=cls, disc=disc, t1=t1, t2=t2, wave_names=wnames, key=key, lane_want=want,
                 off_near=off_n, off_far=off_f)


# ---- in_range, hit_key, min16_key -----------------------------------------------------------------------------
IN_RANGE_ANCHORS = (KMIN_BITS, KMAX_BITS, 0, 0x80000000, 0x7F800000)


@functools.lru_cache(None)
def in_range_table():
    rng = np.random.default_rng(0x12A)
    near = np.concatenate([(np.arange(-4096, 4097) + a) % (1 << 32) for a in IN_RANGE_ANCHORS])
    t = np.concatenate([near, rng.integers(0, 1 << 32, 1 << 20)]).astype(U)
    (t,) = pad64([t])
    sid = rng.integers(0, 1 << 32, len(t)).astype(U)
    x = fb(t)
    with np.errstate(all="ignore"):
        want = ((x > F(0.008)) & (x < np.finfo(F).max)).astype(U)
    return Table([t, sid], [want, sid, t], n_near=len(near), n_true=int(want.sum()))


@functools.lru_cache(None)
def min16_table():
    """Rows of 16 keys; the expected row minimum in Python integers."""
    rng = np.random.default_rng(0x316)
    rows, names = [], []

    def key(tb, i):
        return (int(tb) << 32) | int(i)

    def rnd_t():
        return int(rng.integers(KMIN_BITS + 1, KMAX_BITS))

    def add(name, row):
        assert len(row) == 16
        names.append(name)
        rows.append(row)

    for p in range(16):           # the minimum at each position, with the largest index of the row
        t = sorted(rnd_t() for _ in range(16))
        row = [key(t[1 + k % 15], rng.integers(0, 1 << 20)) for k in range(16)]
        row[p] = key(t[0], 0xFFFFFFF0)
        add(f"min at {p}", row)
    for p in range(16):           # equal t, different indices: the smallest index wins
        t = rnd_t()
        ids = rng.permutation(16) + 5
        row = [key(t, ids[k]) for k in range(16)]
        row[p] = key(t, 2)
        row[(p + 7) % 16] = key(t + 1, 0)    # a smaller index at a larger t must not win
        add(f"equal t, smallest index at {p}", row)
    add("all no hit", [KNOHIT] * 16)
    add("all none", [M64] * 16)
    add("nan keys and one hit", [key(QNAN, k) for k in range(15)] + [key(rnd_t(), 99)])
    add("nan keys only", [key(QNAN, 16 - k) for k in range(16)])
    add("all lanes equal", [key(rnd_t(), 1234)] * 16)
    add("no hit and one hit", [KNOHIT] * 9 + [key(rnd_t(), 7)] + [KNOHIT] * 6)
    for _ in range(64):
        t = [rnd_t() for _ in range(4)]
        add("seeded, few t", [key(t[rng.integers(0, 4)], rng.integers(0, 1 << 32)) for _ in range(16)])
    order = list(range(len(rows)))
    keys, want, wnames = [], [], []
    # waves of 4 rows; then the same rows between neighbours whose every key is smaller (no leak)
    small = lambda: [key(rng.integers(1, KMIN_BITS), rng.integers(0, 16)) for _ in range(16)]
    seq = [(names[k], rows[k]) for k in order]
    while len(seq) % 4:
        seq.append(("seeded", [key(rnd_t(), rng.integers(0, 1 << 32)) for _ in range(16)]))
    for k in order:   # as an inner row between two such rows, and as the wave's first and last row
        leak = (names[k] + ", smaller keys in the neighbouring rows", rows[k])
        seq += [("smaller neighbour", small()), leak, ("smaller neighbour", small()), ("smaller neighbour", small())]
        seq += [leak, ("smaller neighbour", small()), ("smaller neighbour", small()), leak]
    for name, row in seq:
        wnames.append(name)
        keys += row
        want += [min(row)] * 16
    keys, want = np.array(keys, dtype=np.uint64), np.array(want, dtype=np.uint64)
    lo = lambda v: (v & np.uint64(0xFFFFFFFF)).astype(U)
    hi = lambda v: (v >> np.uint64(32)).astype(U)
    return Table([lo(keys), hi(keys)], [lo(want), hi(want)], row_names=wnames, keys=keys)


# ---- PCG32, canonical ---------------------------------------------------------------------------------------
def pcg_out(old):
    old = np.asarray(old, dtype=np.uint64)
    xs = (((old >> np.uint64(18)) ^ old) >> np.uint64(27)).astype(U)
    rot = (old >> np.uint64(59)).astype(U)
    return (xs >> rot) | (xs << ((U(0) - rot) & U(31)))


def pcg_step(st, inc):
    with np.errstate(over="ignore"):
        return np.asarray(st, dtype=np.uint64) * np.uint64(PCG_MUL) + np.asarray(inc, dtype=np.uint64)


def pcg_seed(initstate, inc):
    with np.errstate(over="ignore"):
        return pcg_step(np.asarray(inc, dtype=np.uint64) + np.asarray(initstate, dtype=np.uint64), inc)


def state_for_word(w):
    """A state whose next output is w: with rot = 0 (bits 59-63 clear) the output is bits 27-58 of
    old ^ (old >> 18), an xorshift, inverted by iterating it."""
    v = (int(w) << 27) & M64
    old = v
    for _ in range(4):
        old = v ^ (old >> 18)
    return old


def canonical_ref(w):
    """libstdc++ generate_canonical<float, 24> over a 32-bit engine: float(x) / 2^32, kept below 1."""
    c = np.asarray(w, dtype=U).astype(F) / F(4294967296.0)
    return np.where(c >= F(1), np.nextafter(F(1), F(0)), c).astype(F)


def pm1_ref(w):
    return canonical_ref(w) * F(2) + F(-1)


CHOSEN_WORDS = (0, 1, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6, 0x80000080, 0x80000081,
                0x800000FF, 0x80000180, (1 << 32) - 257, (1 << 32) - 256, (1 << 32) - 255, (1 << 32) - 130, (1 << 32) - 129,
                (1 << 32) - 128, (1 << 32) - 127, (1 << 32) - 2, (1 << 32) - 1)


@functools.lru_cache(None)
def canonical_table():
    rng = np.random.default_rng(0xCA)
    words = list(CHOSEN_WORDS) + [int(x) for x in (1 << 32) - 1 - rng.integers(0, 128, 32)]
    for k in range(24, 32):       # around every power of two above 2^24: conversions that round
        words += [(1 << k) + int(x) for x in rng.integers(0, 1 << (k - 22), 32)]
    words += [int(x) for x in rng.integers(0, 1 << 32, 4096)]
    st = np.array([state_for_word(w) for w in words], dtype=np.uint64)
    st = np.concatenate([st, rng.integers(0, 1 << 63, 4096, dtype=np.uint64) * np.uint64(2) + np.uint64(1)])
    (st,) = pad64([st])
    inc = rng.integers(0, 1 << 63, len(st), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    w = pcg_out(st)
    nxt = pcg_step(st, inc)
    lo = lambda v: (v & np.uint64(0xFFFFFFFF)).astype(U)
    hi = lambda v: (v >> np.uint64(32)).astype(U)
    planes = [lo(st), hi(st), lo(inc), hi(inc)]
    return (Table(planes, [canonical_ref(w), lo(nxt), hi(nxt)], words=w, chosen=np.array(words, dtype=np.uint64)),
            Table(planes, [pm1_ref(w), lo(nxt), hi(nxt)], words=w))


PCG_DRAWS = 8


@functools.lru_cache(None)
def pcg_stream_table():
    """Streams from (initstate, inc) as the kernels seed them: stream keys and seeds past 2^32."""
    rng = np.random.default_rng(0x9C6)
    init = np.concatenate([np.arange(64, dtype=np.uint64), np.uint64(1 << 32) + np.arange(64, dtype=np.uint64),
                           rng.integers(0, 1 << 63, 1024, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 1024, dtype=np.uint64),
                           np.full(64, M64, dtype=np.uint64)])
    seed = np.concatenate([np.arange(len(init) // 2, dtype=np.uint64),
                           rng.integers(1 << 32, 1 << 61, len(init) - len(init) // 2, dtype=np.uint64)])
    seed = rng.permutation(seed)
    with np.errstate(over="ignore"):
        inc = ((np.uint64(2) * seed + rng.integers(0, 2, len(seed), dtype=np.uint64)) << np.uint64(1)) | np.uint64(1)
    st = pcg_seed(init, inc)
    outs = []
    for _ in range(PCG_DRAWS):
        outs.append(pcg_out(st))
        st = pcg_step(st, inc)
    lo = lambda v: (v & np.uint64(0xFFFFFFFF)).astype(U)
    hi = lambda v: (v >> np.uint64(32)).astype(U)
    return Table([lo(init), hi(init), lo(inc), hi(inc)], outs + [lo(st), hi(st)], n_wide_init=int((init >> np.uint64(32) != 0).sum()),
                 n_wide_inc=int((inc >> np.uint64(32) != 0).sum()))


# ---- random_in_unit_sphere ------------------------------------------------------------------------------------
@functools.lru_cache(None)
def unit_sphere_table():
    """States whose first k attempts are rejected, k = 0..7, by the reference's loop (raytracer.hxx:32-43,
    `length(v) > 1.f` with a float32 sqrt) over the reference PCG."""
    rng = np.random.default_rng(0x5F)
    m = 1 << 16
    st0 = rng.integers(0, 1 << 63, m, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, m, dtype=np.uint64)
    inc = rng.integers(0, 1 << 63, m, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    st = st0.copy()
    done = np.zeros(m, dtype=bool)
    k_of = np.full(m, -1)
    p = [np.zeros(m, dtype=F) for _ in range(3)]
    fin = st0.copy()
    for k in range(8):
        v = []
        for _ in range(3):
            v.append(pm1_ref(pcg_out(st)))
            st = pcg_step(st, inc)
        acc = ~done & ~(np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) > F(1))
        for c in range(3):
            p[c][acc] = v[c][acc]
        fin[acc] = st[acc]
        k_of[acc] = k
        done |= acc
    pick = np.concatenate([np.flatnonzero(k_of == k)[:128] for k in range(8)])
    pick = rng.permutation(pick)
    pick = pick[:len(pick) // 64 * 64]
    lo = lambda v: (v[pick] & np.uint64(0xFFFFFFFF)).astype(U)
    hi = lambda v: (v[pick] >> np.uint64(32)).astype(U)
    k = k_of[pick]
    res = [p[0][pick], p[1][pick], p[2][pick], lo(fin), hi(fin)]
    calls = (k // 4 + 1).astype(U)
    return Table([lo(st0), hi(st0), lo(inc), hi(inc)], res + [calls] + res, k=k)


# ---- refract, normalize ---------------------------------------------------------------------------------------
def refract_ref(I, N, eta):
    """math.hxx:300-309 in float32 with an IEEE sqrt."""
    with np.errstate(all="ignore"):
        dv = N[0] * I[0] + N[1] * I[1] + N[2] * I[2]
        k = F(1) - eta * eta * (F(1) - dv * dv)
        s = np.sqrt(k)
        flag = (k >= 0).astype(F)
        out = [(I[c] * eta - (N[c] * s + dv * eta)) * flag for c in range(3)]
    assert k.dtype == np.float32 and out[0].dtype == np.float32
    return out, k


@functools.lru_cache(None)
def refract_table():
    rng = np.random.default_rng(0x2EF)
    etas = np.array([1.5, 1 / 1.5, 1.33, 1 / 1.33, 2.4, 1 / 2.4, 0.75, 1 / 0.75, 1.0000001, 1 / 1.0000001, 1], dtype=F)
    I, N, E = [[], [], []], [[], [], []], []

    def add(i, n, e):
        for c in range(3):
            I[c].append(np.asarray(i[c], dtype=F))
            N[c].append(np.asarray(n[c], dtype=F))
        E.append(np.asarray(e, dtype=F))

    # k steered through eta and d = dot(N, I) with N an axis (d = I's component, exactly): a window of
    # consecutive d around the critical cosine sqrt(1 - 1 / eta^2), where k changes sign
    steered = 0
    for e in etas[etas > 1]:
        dstar = F(math.sqrt(1 - 1 / float(e) ** 2))
        dd = fb(bf(dstar).astype(np.int64) + np.arange(-256, 256))
        sx = np.sqrt(np.maximum(F(1) - dd * dd, 0)).astype(F)
        z = np.zeros_like(dd)
        for axis, sign in ((2, 1), (1, -1), (0, 1)):
            i = [sx, z, z] if axis != 0 else [z, sx, z]
            i[axis] = dd * F(sign)
            n = [z, z, z]
            n[axis] = z + F(sign)
            add(i, n, z + e)
            steered += len(dd)
    for e in etas:                  # d = 0 at eta = 1: k exactly 0; d = +-1: k exactly 1
        z = np.zeros(8, dtype=F)
        add([z + 1, z, z], [z, z, z + 1], z + F(1))
        add([z, z, z + 1], [z, z, z + 1], z + e)
        add([z, z, z - 1], [z, z, z + 1], z + e)
    m = 1 << 14                      # seeded unit vectors
    u = lambda: rng.uniform(-1, 1, m).astype(F)
    unit = lambda v: [c / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) for c in v]
    add(unit([u(), u(), u()]), unit([u(), u(), u()]), rng.choice(etas, m))
    I = [np.concatenate(c) for c in I]
    N = [np.concatenate(c) for c in N]
    E = np.concatenate(E)
    planes = pad64(I + N + [E])
    out, k = refract_ref(planes[0:3], planes[3:6], planes[6])
    pos = k[k > 0]
    return Table(planes, out, k=k, n_zero=int((k == 0).sum()), n_neg=int((k < 0).sum()), n_one=int((k == 1).sum()),
                 k_min_pos=float(pos.min()), n_min_pos=int((k == pos.min()).sum()), steered=steered)


def normalize_ref(v):
    with np.errstate(all="ignore"):
        l = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        big = np.abs(l) > FLT_MIN
        out = [np.where(big, c / np.where(big, l, F(1)), c) for c in v]
    return out, l


@functools.lru_cache(None)
def normalize_table():
    """A float32 length is 0 or at least 2^-74.5 (the squares underflow below that): lengths of 0 from zero,
    subnormal and tiny components, the smallest non-zero lengths, and seeded vectors."""
    rng = np.random.default_rng(0x40)
    tiny = np.array([0, -0.0, 2.0 ** -149, 2.0 ** -126, 2.0 ** -100, 2.0 ** -76, 2.0 ** -75, 1.5 * 2.0 ** -75, 2.0 ** -74.5,
                     2.0 ** -74, 2.0 ** -70, -(2.0 ** -75), -1.5 * 2.0 ** -75], dtype=F)
    g = np.stack(np.meshgrid(tiny, tiny, tiny, indexing="ij")).reshape(3, -1)
    m = 1 << 14
    s = (2.0 ** rng.integers(-80, 30, m)).astype(F)
    v = [np.concatenate([g[c], rng.uniform(-1, 1, m).astype(F) * s]) for c in range(3)]
    v = pad64(v)
    out, l = normalize_ref(v)
    return Table(v, out, n_zero_len=int((l == 0).sum()), min_len=float(l[l > 0].min()), n_small=int(((l > 0) & (l < p2(-70))).sum()))


# ---- schlick_x ------------------------------------------------------------------------------------------------
SCHLICK_RI = (1.5, 1.33, 2.4, 0.75, 1.0000001, 1.0)


@functools.lru_cache(None)
def schlick_table():
    rng = np.random.default_rng(0x5C)
    ris = []
    for ri in SCHLICK_RI:
        ris += [F(ri), F(1) / F(ri)]
    one = bits1(1.0)
    edge = np.concatenate([np.arange(0, 1025), one + np.arange(-1024, 1025)]).astype(U)
    xf, c = [], []
    for ri in ris:
        cc = np.concatenate([fb(edge), rng.random(1 << 16).astype(F), fb(rng.integers(0, one + 1, 1 << 12).astype(U))])
        c.append(cc)
        xf.append(np.full(len(cc), (F(1) - ri) / (F(1) + ri), dtype=F))
    xf, c = pad64([np.concatenate(xf), np.concatenate(c)])
    want = host_call("schlick_pow", [xf, c])
    # (tests/test_primitives_cpu.py checks the tool's pow against math.pow on a slice: schlick_py)
    return Table([xf, c], [want], ris=ris, n_edge=len(edge))


def schlick_py(xf, c):
    out = np.empty(len(xf), dtype=F)
    for i, (x, cc) in enumerate(zip(xf.tolist(), c.tolist())):
        r0 = x * x
        out[i] = r0 + (1.0 - r0) * math.pow(float(F(1) - F(cc)), 5)
    return out


# ---- udiv -----------------------------------------------------------------------------------------------------
def udiv_divisors():
    d = [1, 2, 3, 5, 7, 64, 1280 * 720, 1 << 31, (1 << 32) - 1]
    for k in range(1, 32):
        d += [(1 << k) - 1, (1 << k) + 1]
    return sorted(set(x for x in d if 1 <= x < 1 << 32))


def udiv_table(make_udiv):
    """make_udiv: the host's (probe.make_udiv). Expected quotients in Python integers."""
    rng = np.random.default_rng(0x0D)
    ns, ds = [], []
    for d in udiv_divisors():
        top = ((1 << 32) - 1) // d
        mult = {1, 2, 3, top, max(top - 1, 1), max(top // 2, 1)} | {int(x) for x in rng.integers(1, top + 1, 8)}
        n = {0, d - 1, d, (1 << 32) - 1, (1 << 32) - 2} | {int(x) for x in rng.integers(0, 1 << 32, 8)}
        for k in mult:
            n |= {k * d - 1, k * d, k * d + 1}
        n = sorted(x for x in n if 0 <= x < 1 << 32)
        ns += n
        ds += [d] * len(n)
    want = [n // d for n, d in zip(ns, ds)]
    u = {d: make_udiv(d) for d in set(ds)}
    cols = [np.array([u[d][k] for d in ds], dtype=U) for k in range(3)]
    n, m, s1, s2, w, dd = pad64([np.array(ns, dtype=U)] + cols + [np.array(want, dtype=U), np.array(ds, dtype=U)])
    return Table([n, m, s1, s2], [w], divisors=dd)
