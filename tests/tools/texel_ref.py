"""TEST INFRASTRUCTURE: the rgb8 texel as a table. Over the floats of its domain, words 0 .. LAST
(0x3f811b5e, the last float whose product 255.f * pow stays under 256), the contract's texel
(rt_texel.h, rt_api.h: pow((double)c, (double)(1 / 2.2f)), narrowed to float, times 255.f, truncated)
is monotone with 255 steps, so the 255 words at which it steps describe it on every float.
tests/golden/texel_steps.json holds those words as tests/tools/texel_sweep.cpp found them
(tests/test_texel_cpu.py reproduces them), with the reference form's words on the recording host.

    from texel_ref import texel, assert_texels, assert_reference_texels, windows

    assert_texels(got_u8, f32, "what")                      # got is the contract's texel, everywhere
    assert_reference_texels(got_u8, ref_u8, f32, "what")    # ... and the reference's where its powf agrees
"""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np

import oracle_binding as O
from support import words

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(REPO, "tests", "golden", "texel_steps.json")
F = np.float32
LAST = 0x3f811b5e              # the domain's last float (the fixture carries it too; steps() checks)
NEGATIVE_ZERO = 0x80000000
REFERENCE_DISAGREES_MAX = 2    # positions per frame where the reference's own powf leaves the contract
_lib = None


# ---- the sweep (CPU, every float) -------------------------------------------------------------------
def build():
    out = os.path.join(REPO, "tests", "tools", "_build", "libtexel_sweep.so")
    src = os.path.join(REPO, "tests", "tools", "texel_sweep.cpp")
    dep = os.path.join(REPO, "oracle", "rt_oracle.cpp")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(dep)):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-pthread",
                        "-shared", "-o", tmp, src], check=True)
        os.replace(tmp, out)
    return out


class _Result(C.Structure):
    _fields_ = [("n_steps", C.c_uint32 * 2), ("non_monotone", C.c_uint64 * 2), ("n_differ", C.c_uint32)]


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.texel_sweep.restype = C.c_int
        L.texel_sweep.argtypes = [C.c_uint32, C.c_uint32, C.c_float, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.POINTER(_Result)]
        L.texel_first_256.restype = C.c_int
        L.texel_first_256.argtypes = [C.c_uint32, C.c_float, C.c_void_p]
        _lib = L
    return _lib


def sweep(first=0, last=LAST, threads=None, cap=4096):
    """Both forms over the floats first..last (words): per form ("contract", "reference") the steps
    (word, texel) as two uint32 arrays, the number of steps and of non-monotone neighbours; and the
    floats at which the two forms' texels differ."""
    threads = threads or min(16, os.cpu_count() or 1)
    sw = np.zeros((2, cap), dtype=np.uint32)
    st = np.zeros((2, cap), dtype=np.uint32)
    df = np.zeros(cap, dtype=np.uint32)
    res = _Result()
    rc = lib().texel_sweep(first, last, float(F(1) / F(2.2)), threads, cap, sw.ctypes.data, st.ctypes.data,
                           df.ctypes.data, C.byref(res))
    assert rc == 0, rc
    out = {}
    for f, name in enumerate(("contract", "reference")):
        n = min(cap, res.n_steps[f])
        out[name] = dict(words=sw[f, :n].copy(), texels=st[f, :n].copy(), n_steps=int(res.n_steps[f]),
                         non_monotone=int(res.non_monotone[f]))
    out["n_differ"] = int(res.n_differ)
    out["differ"] = df[:min(cap, res.n_differ)].copy()
    return out


def first_256(start=0x3f800000):
    """Per form, the first float from `start` upward whose product reaches 256: (contract, reference)."""
    out = np.zeros(2, dtype=np.uint32)
    assert lib().texel_first_256(start, float(F(1) / F(2.2)), out.ctypes.data) == 0
    return int(out[0]), int(out[1])


# ---- the table ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def steps(form="contract"):
    """The 255 words at which the texel steps (word k-1: the first float whose texel is k), read-only
    uint32. form "reference": the reference form's words as recorded on the fixture's host."""
    fx = fixture()
    assert int(fx["domain_last"], 16) == LAST, fx["domain_last"]
    s = np.array([int(w, 16) for w in fx["steps" if form == "contract" else "reference_steps"]], dtype=np.uint32)
    assert s.size == 255 and (np.diff(s.astype(np.int64)) > 0).all() and s[-1] <= LAST
    s.setflags(write=False)
    return s


def reference_differs():
    """The floats (words) at which the reference form's texel left the contract's on the fixture's host."""
    return np.array([int(w, 16) for w in fixture()["reference_differs"]], dtype=np.uint32)


def texel(f32):
    """The contract's texel of every element of a float32 array, from the table: uint8 of its shape.
    -0.0 gives 0; every other element must lie in the domain."""
    f32 = np.asarray(f32)
    assert f32.dtype == np.float32, f32.dtype
    w = words(f32).reshape(f32.shape)
    w = np.where(w == NEGATIVE_ZERO, np.uint32(0), w)
    assert w.size == 0 or int(w.max()) <= LAST, f"texel(): word {int(w.max()):#010x} lies outside [0, {LAST:#010x}]"
    return np.searchsorted(steps(), w, side="right").astype(np.uint8)


def _first(bad, got, want, f32, n=8):
    i = np.flatnonzero(bad.reshape(-1))[:n]
    w = words(f32).reshape(-1)
    return [f"{int(w[k]):#010x} got {int(got.reshape(-1)[k])} want {int(want.reshape(-1)[k])}" for k in i]


def assert_texels(got_u8, f32, what=""):
    """got_u8 is the contract's texel of f32 on every element."""
    got_u8, f32 = np.asarray(got_u8), np.asarray(f32)
    assert got_u8.dtype == np.uint8 and got_u8.size == f32.size, (what, got_u8.dtype, got_u8.shape, f32.shape)
    got = got_u8.reshape(f32.shape)
    want = texel(f32)
    bad = got != want
    n = int(np.count_nonzero(bad))
    print(f"{what}: {n} of {want.size} texels differ from the table")
    assert n == 0, f"{what}: {n} of {want.size} texels differ from the table, first {_first(bad, got, want, f32)}"


def assert_reference_texels(got_u8, ref_u8, f32, what=""):
    """got_u8 is the contract's texel of f32 everywhere; it is the reference's texel ref_u8 wherever
    this host's reference form (O.epilogue_rgb8) gives the contract's texel; and the other positions,
    where the reference's own powf disagrees with a correctly rounded pow, number at most
    REFERENCE_DISAGREES_MAX (a condition, not a measurement: one float in 2^30 disagrees under glibc 2.35)."""
    got_u8, ref_u8, f32 = np.asarray(got_u8), np.asarray(ref_u8), np.asarray(f32)
    assert ref_u8.dtype == np.uint8 and ref_u8.size == f32.size, (what, ref_u8.dtype, ref_u8.shape, f32.shape)
    assert_texels(got_u8, f32, what)
    got, ref = got_u8.reshape(f32.shape), ref_u8.reshape(f32.shape)
    want = texel(f32)
    agrees = O.epilogue_rgb8(f32) == want
    bad = agrees & (got != ref)
    n = int(np.count_nonzero(bad))
    off = np.flatnonzero(~agrees.reshape(-1))
    w = words(f32).reshape(-1)
    print(f"{what}: {n} texels differ from the reference's where its powf agrees; its powf disagrees at "
          f"{off.size} positions, floats {sorted({f'{int(w[k]):#010x}' for k in off[:64]})}")
    assert n == 0, f"{what}: {n} texels differ from the reference's, first {_first(bad, got, ref, f32)}"
    assert off.size <= REFERENCE_DISAGREES_MAX, \
        f"{what}: the reference's powf leaves the contract at {off.size} positions (> {REFERENCE_DISAGREES_MAX})"


def windows(k=8):
    """Every float within +-k of each step, plus 0, -0.0, the smallest subnormal, FLT_MIN, the two
    largest floats under 1, 1.0f and the domain's last float: float32, sorted by word, no duplicates
    (so -0.0, the largest word, comes last)."""
    s = steps().astype(np.int64)
    near = (s[:, None] + np.arange(-k, k + 1, dtype=np.int64)[None, :]).reshape(-1)
    near = near[(near >= 0) & (near <= LAST)]
    extra = np.array([0, NEGATIVE_ZERO, 1, 0x00800000, 0x3f7ffffe, 0x3f7fffff, 0x3f800000, LAST], dtype=np.int64)
    return np.unique(np.concatenate([near, extra])).astype(np.uint32).view(F)
