"""rt_options.sky_moments, without a GPU: the field that lets frames with per-pixel
moments hand their proven-sky tiles to sky_moments_kernel. Its default, its key in rt_options_parse,
its round trip through rt.options and the process default, and the refusal of every other value with
the field named. (What the option changes on the device is tests/test_sky_moments_gpu.py.)
"""
import ctypes as C

import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi


def test_sky_moments_defaults_to_off():
    assert rt.options().sky_moments == 0
    assert rt.parse_options("").sky_moments == 0
    lib_default = abi.RtOptions()
    assert rt.lib().rt_options_default(C.byref(lib_default)) == abi.RT_OK
    assert lib_default.sky_moments == 0


def test_sky_moments_parses_and_round_trips():
    assert rt.parse_options("sky_moments=1").sky_moments == 1
    both = rt.parse_options("sky_moments=1,tile_classes=1,render_streams=3")
    assert (both.sky_moments, both.tile_classes, both.render_streams) == (1, 1, 3)
    assert rt.parse_options("sky_moments=0", rt.options(sky_moments=1)).sky_moments == 0
    o = rt.options(sky_moments=1)
    assert o.sky_moments == 1 and o.tile_classes == 0
    assert rt.options(o).sky_moments == 1  # (a copy of the record keeps it)
    prev = rt.default_options()
    try:
        rt.set_default_options(o)
        assert rt.default_options().sky_moments == 1
        with rt.default_options_set(sky_moments=0):
            assert rt.default_options().sky_moments == 0
        assert rt.default_options().sky_moments == 1
    finally:
        rt.set_default_options(prev)
    assert rt.default_options().sky_moments == prev.sky_moments


def test_the_record_keeps_the_library_size():
    """The Python record and the library's agree on the record's size with the field in it."""
    o = rt.options(sky_moments=1)
    assert o.size == C.sizeof(abi.RtOptions)
    names = [n for n, _ in abi.RtOptions._fields_]
    assert names.index("sky_moments") == names.index("tile_classes") + 1
    assert abi.RtOptions.sky_moments.offset == abi.RtOptions.tile_classes.offset + 4


@pytest.mark.parametrize("text", ["sky_moments=2", "sky_moments=4294967296"])
def test_sky_moments_refused_with_the_field_named(text):
    base = rt.options(render_streams=3)
    before = bytes(base)
    with pytest.raises(rt.RtError) as e:
        rt.parse_options(text, base)
    assert e.value.status == abi.RT_ERR_INVALID and "sky_moments" in str(e.value)
    assert bytes(base) == before  # the record is left as it was
    bad = rt.options()
    bad.sky_moments = 2
    with pytest.raises(rt.RtError) as e:
        rt.set_default_options(bad)
    assert e.value.status == abi.RT_ERR_INVALID and "sky_moments" in str(e.value)
