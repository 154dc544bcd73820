"""The rgb8 texel as a table, on the CPU (tests/tools/texel_ref.py, tests/golden/texel_steps.json).

tests/tools/texel_sweep.cpp walks every float of the texel's domain, words 0 .. 0x3f811b5e, in the
contract's form (pow in double with the exponent (double)(1 / 2.2f), narrowed, times 255.f, truncated)
and in the reference's (this host's powf through oracle_epilogue_rgb8). The sweep must reproduce the
fixture's 255 step words; the table must then be what numpy's double pow gives (progressive_ref.texel,
the sessions' reference), what the restatement gives outside the floats at which this host's powf leaves
the contract (one float, 0x3c364a2a, under glibc 2.35), and what every golden .u8 holds.

Tolerance: none. Every comparison is exact; the floats where the reference's powf disagrees are
counted, named and capped at 8.
"""
import glob
import os
import sys
import time

import numpy as np
import pytest

import golden_io as G
import oracle_binding as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import progressive_ref  # noqa: E402
import texel_ref as T  # noqa: E402
from support import words  # noqa: E402

DIFFER_MAX = 8  # floats of the domain at which a host's powf may leave the correctly rounded pow


@pytest.fixture(scope="module")
def swept():
    t0 = time.perf_counter()
    r = T.sweep(0, T.LAST)
    print(f"texel sweep of {T.LAST + 1} floats, both forms: {time.perf_counter() - t0:.2f} s")
    return r


@pytest.fixture(scope="module")
def probes():
    """windows(64) and 2^20 seeded random floats of the domain (words uniform in 0 .. LAST), read-only."""
    g = np.random.default_rng(20261021)
    w = g.integers(0, T.LAST + 1, size=1 << 20, dtype=np.uint32)
    p = np.concatenate([T.windows(64), w.view(np.float32)])
    p.setflags(write=False)
    return p


def _named(ws):
    return [f"{int(w):#010x}" for w in ws]


def test_sweep_reproduces_the_table(swept):
    c = swept["contract"]
    assert c["non_monotone"] == 0
    assert c["n_steps"] == 255
    np.testing.assert_array_equal(c["texels"], np.arange(1, 256))
    np.testing.assert_array_equal(c["words"], T.steps())
    assert int(c["words"][0]) == 0x36aa5b87 and int(c["words"][-1]) == 0x3f7fffff
    # the domain ends where the product first reaches 256 (beyond it the cast to uint8_t is undefined)
    assert T.first_256()[0] == T.LAST + 1 == int(T.fixture()["first_256"], 16)


def test_reference_form_is_monotone_with_255_steps(swept):
    r = swept["reference"]
    assert r["non_monotone"] == 0
    assert r["n_steps"] == 255
    np.testing.assert_array_equal(r["texels"], np.arange(1, 256))
    assert T.first_256()[1] > T.LAST


def test_forms_differ_on_a_handful_of_floats(swept):
    host, recorded = _named(swept["differ"]), _named(T.reference_differs())
    fx = T.fixture()
    print(f"floats whose reference texel leaves the contract's: this host {host}; "
          f"recorded under glibc {fx['glibc']} on {fx['date']}: {recorded}")
    if host != recorded:
        print(f"this host's set differs from the record: host {host}, record {recorded}")
    assert swept["n_differ"] <= DIFFER_MAX, f"{swept['n_differ']} floats differ: host {host}, record {recorded}"
    # each differing float lies on a step: one of the two forms steps there
    both = np.concatenate([swept["contract"]["words"], swept["reference"]["words"]])
    for w in swept["differ"]:
        assert np.abs(both.astype(np.int64) - int(w)).min() <= 1, f"{int(w):#010x} differs away from any step"


def test_windows_hold_every_step_and_the_edges():
    w = words(T.windows(8))
    assert np.isin(T.steps(), w).all() and np.isin(T.steps() - 1, w).all()
    for edge in (0, 0x80000000, 1, 0x00800000, 0x3f7ffffe, 0x3f7fffff, 0x3f800000, T.LAST):
        assert edge in w, hex(edge)
    assert w.size == np.unique(w).size and 255 * 17 <= w.size <= 255 * 17 + 8
    t = T.texel(T.windows(8))
    assert t[-1] == 0 and words(T.windows(8))[-1] == 0x80000000   # -0.0 gives 0
    assert set(np.unique(t)) == set(range(256))


def test_table_is_numpys_double_pow(probes):
    """texel_ref.texel == progressive_ref.texel (the sessions' reference) on every probe."""
    np.testing.assert_array_equal(T.texel(probes), progressive_ref.texel(probes))


def test_restatement_is_the_table_outside_the_differing_set(swept, probes):
    inside = np.isin(words(probes), swept["differ"])
    got, want = O.epilogue_rgb8(probes), T.texel(probes)
    print(f"{int(inside.sum())} of {probes.size} probes lie in the differing set")
    np.testing.assert_array_equal(got[~inside], want[~inside])
    assert (got[inside] != want[inside]).all()  # the set is exactly where they differ


def test_goldens_are_the_table_outside_the_differing_set(swept):
    """Every .u8 under tests/golden (written by the reference's own binaries) against the table of its .f32."""
    names = sorted(glob.glob(os.path.join(G.GOLDEN, "*.u8")))
    assert len(names) >= 10
    for u8_path in names:
        f32 = np.fromfile(u8_path[:-3] + ".f32", dtype="<f4")
        u8 = np.fromfile(u8_path, dtype=np.uint8)
        assert f32.size == u8.size
        inside = np.isin(words(f32), swept["differ"])
        print(f"{os.path.basename(u8_path)}: {int(inside.sum())} of {u8.size} positions in the differing set")
        np.testing.assert_array_equal(u8[~inside], T.texel(f32)[~inside], err_msg=os.path.basename(u8_path))
        assert int(inside.sum()) <= T.REFERENCE_DISAGREES_MAX


def test_texel_refuses_floats_outside_the_domain():
    for w in (T.LAST + 1, 0x7f800000, 0xbf800000, 0x80000001):
        with pytest.raises(AssertionError):
            T.texel(np.array([w], dtype=np.uint32).view(np.float32))


def test_assert_reference_texels_separates_the_two_failures():
    """The helper against itself: a frame holding the differing float passes with the reference's u8 as
    it is on this host; one wrong texel fails; a reference that disagrees elsewhere fails."""
    f = np.union1d(words(T.windows(1)), T.reference_differs()).view(np.float32)
    ref = O.epilogue_rgb8(f)
    T.assert_reference_texels(T.texel(f), ref, f, "self")
    wrong = T.texel(f).copy()
    wrong[7] ^= 1
    with pytest.raises(AssertionError, match="differ from the table"):
        T.assert_reference_texels(wrong, ref, f, "wrong texel")
    k = int(np.flatnonzero(ref == T.texel(f))[5])
    ref2 = ref.copy()
    ref2[k] ^= 1
    with pytest.raises(AssertionError, match="differ from the reference"):
        T.assert_reference_texels(T.texel(f), ref2, f, "wrong reference")
