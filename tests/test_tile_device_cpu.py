"""The device tile classes' host-side surface, without a GPU: the rt_options
field that selects them and the argument checks of rt_tile_order_device, which come before any HIP
call. That the shared beam arithmetic (csrc/rt_tiles.h) still gives the host's classes is what
tests/test_tiles_cpu.py and tests/test_camera_cases_cpu.py check, unchanged.
"""
import ctypes as C

import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi


def test_tile_classes_defaults_to_the_host():
    assert rt.options().tile_classes == 0
    assert rt.parse_options("").tile_classes == 0


def test_tile_classes_parses_and_builds():
    assert rt.parse_options("tile_classes=1").tile_classes == 1
    assert rt.parse_options("tile_classes=1,render_streams=3").render_streams == 3
    assert rt.parse_options("tile_classes=0", rt.options(tile_classes=1)).tile_classes == 0
    o = rt.options(tile_classes=1)
    assert o.tile_classes == 1 and o.size == C.sizeof(abi.RtOptions)
    prev = rt.default_options()  # (the record is accepted as the process default)
    try:
        rt.set_default_options(o)
        assert rt.default_options().tile_classes == 1
    finally:
        rt.set_default_options(prev)


@pytest.mark.parametrize("text", ["tile_classes=2", "tile_classes=4294967295", "tile_classes=4294967296",
                                  "tile_classes=-1", "tile_classes=x"])
def test_tile_classes_refused_with_the_field_named(text):
    base = rt.options(render_streams=3)
    before = bytes(base)
    with pytest.raises(rt.RtError) as e:
        rt.parse_options(text, base)
    assert e.value.status == abi.RT_ERR_INVALID and "tile_classes" in str(e.value)
    assert bytes(base) == before  # the record is left as it was
    bad = rt.options()
    bad.tile_classes = 2
    with pytest.raises(rt.RtError) as e:
        rt.set_default_options(bad)
    assert e.value.status == abi.RT_ERR_INVALID and "tile_classes" in str(e.value)


def test_tile_order_device_checks_its_arguments_before_any_device_call():
    """A null scene, camera, params or count pointer, or a capacity without a buffer, is
    RT_ERR_INVALID; the scene pointer is not followed before that (here it is not a scene)."""
    L = rt.lib()
    cam = rt.Camera.default(64, 40).c
    p = rt.make_params(64, 40, 1)
    not_a_scene = C.create_string_buffer(64)
    scene = C.cast(not_a_scene, C.c_void_p)
    nb, nl, ns = C.c_uint32(7), C.c_uint32(7), C.c_uint32(7)
    good = [scene, C.byref(cam), C.byref(p), None, 0, C.byref(nb), C.byref(nl), C.byref(ns), None]
    for k in (0, 1, 2, 5, 6, 7):
        args = list(good)
        args[k] = None
        assert L.rt_tile_order_device(*args) == abi.RT_ERR_INVALID, k
        assert b"rt_tile_order_device" in L.rt_last_error()
    args = list(good)
    args[4] = 16  # room for 16 entries, no buffer
    assert L.rt_tile_order_device(*args) == abi.RT_ERR_INVALID
    assert (nb.value, nl.value, ns.value) == (7, 7, 7)
    assert L.rt_scene_order_counts(None, None, None, None) == abi.RT_ERR_INVALID
