"""tests/tools/support.py itself: what assert_bits accepts and refuses, and the properties the moved
docstrings of orbit_camera and synthetic_planes state. No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import support as S  # noqa: E402

F = np.float32


def f32(*words):
    return np.array(words, dtype=np.uint32).view(F)


def test_equal_arrays_pass():
    a = np.arange(24, dtype=F).reshape(4, 6)
    S.assert_bits(a, a.copy(), "equal")
    S.assert_bits(a.T, np.ascontiguousarray(a.T), "a transposed view against its contiguous copy")
    S.assert_bits(a[:, ::2], a[:, ::2].copy(), "a strided view")
    S.assert_bits(f32(0x7fc00001, 0xffc00000), f32(0x7fc00001, 0xffc00000), "NaNs with equal payloads")
    S.assert_bits(np.arange(7, dtype=np.uint8), np.arange(7, dtype=np.uint8), "7 bytes")
    S.assert_bits(np.zeros((0, 3), dtype=F), np.zeros((0, 3), dtype=F), "empty")


ONE = np.ones(4, dtype=F)
REFUSED = {
    "one flipped low bit": (f32(0x3f800000, 0x3f800001), f32(0x3f800000, 0x3f800000)),
    "signed zeros": (np.array([0.0], dtype=F), np.array([-0.0], dtype=F)),
    "NaN payloads": (f32(0x7fc00001), f32(0x7fc00002)),
    "float64 against float32": (ONE.astype(np.float64), ONE),
    "uint8 against float32 of equal byte length": (ONE.view(np.uint8), ONE),
    "(4, 6) against (6, 4)": (np.zeros((4, 6), dtype=F), np.zeros((6, 4), dtype=F)),
    "empty against non-empty": (np.zeros(0, dtype=F), ONE),
    "a byte of seven": (np.arange(7, dtype=np.uint8), np.array([0, 1, 2, 3, 4, 5, 7], dtype=np.uint8)),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_differences_fail_and_name_the_case(case):
    got, ref = REFUSED[case]
    with pytest.raises(AssertionError, match="the case's name"):
        S.assert_bits(got, ref, "the case's name")
    with pytest.raises(AssertionError, match="second"):
        S.assert_all_bits(dict(first=ref, second=got), dict(first=ref, second=ref), "planes")
    with pytest.raises(AssertionError, match="variance"):
        S.assert_all_bits((ref, got, ref), (ref, ref, ref))


def test_words_never_converts():
    assert S.words(np.ones((2, 3), dtype=F)).dtype == np.uint32 and S.words(np.ones(5, dtype=np.int8)).dtype == np.uint8
    assert S.words(np.array([-1], dtype=np.int32))[0] == 0xffffffff
    for dtype in (np.float64, np.int64, np.float16):
        with pytest.raises(TypeError):
            S.words(np.ones(4, dtype=dtype))
    with pytest.raises(TypeError):
        S.assert_bits(np.ones(4), np.ones(4), "float64 on both sides")


def test_the_plural_form_compares_the_named_planes_only():
    a, b = dict(x=ONE, y=ONE, extra=ONE * 2), dict(x=ONE, y=ONE, extra=ONE)
    S.assert_all_bits(a, b, "named", ("x", "y"))
    with pytest.raises(AssertionError, match="extra"):
        S.assert_all_bits(a, b, "every key of ref")
    with pytest.raises(AssertionError):
        S.assert_all_bits((ONE, ONE), (ONE, ONE, ONE), "two outputs against three")


def test_orbit_camera_turns_about_the_vertical_axis_through_look():
    c0, c8 = S.orbit_camera(70, 37, 0), S.orbit_camera(70, 37, 8)
    assert c0 is S.orbit_camera(70, 37, 0)  # cached
    assert bytes(c0.c) == bytes(S.camera_at(70, 37).c) == bytes(S.shifted_camera(70, 37).c)
    assert bytes(c8.c) != bytes(c0.c)
    # the turned position keeps its height and its distance from the axis
    a = math.radians(8 * S.STEP_DEG)
    dx, dz = S.POS[0] - S.LOOK[0], S.POS[2] - S.LOOK[2]
    x, z = S.LOOK[0] + dx * math.cos(a) + dz * math.sin(a), S.LOOK[2] - dx * math.sin(a) + dz * math.cos(a)
    assert np.hypot(x - S.LOOK[0], z - S.LOOK[2]) == pytest.approx(np.hypot(dx, dz), rel=1e-12)
    assert bytes(c8.c) == bytes(S.camera_at(70, 37, (x, S.POS[1], z)).c)


@pytest.mark.parametrize("block", [False, True])
def test_synthetic_planes_are_what_the_docstring_says(block):
    w, h = 37, 19
    p = S.synthetic_planes(w, h, block, variance_scale=0.02)
    assert list(p) == ["beauty", "albedo", "normal", "depth", "variance"]
    assert all(a.dtype == F and not a.flags.writeable for a in p.values())
    right = slice(w // 2 if block else 0, None)
    assert np.abs(np.linalg.norm(p["normal"][:, right].astype(np.float64), axis=-1) - 1).max() < 1e-6  # unit normals
    assert 0 <= p["depth"].min() and p["depth"].max() < 4 and 0 <= p["variance"].min() and p["variance"].max() < 0.02
    if block:
        left = slice(0, w // 2)
        assert (p["beauty"][:, left] == (F(0.25), F(0.5), F(0.75))).all() and (p["albedo"][:, left] == (F(0.5), F(0.625), F(0.75))).all()
        assert not p["normal"][:, left].any() and not p["depth"][:, left].any() and not p["variance"][:, left].any()
    # the variance is drawn last: without it the other planes keep their bits; a seed of the caller's replaces w * 1000 + h
    S.assert_all_bits(S.synthetic_planes(w, h, block), {n: a for n, a in p.items() if n != "variance"}, "without a variance")
    S.assert_all_bits(S.synthetic_planes(w, h, block, 0.02, seed=w * 1000 + h), p, "the default seed")
