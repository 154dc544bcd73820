"""The synchronous host-buffer entry points share one cached context per device, and one device
arena in it that every call lays its planes out in from offset 0. What can go wrong there is one
call disturbing the next: a stale size, a stale offset, a plane not uploaded again. So every call is
made once alone on a fresh context (rt.release_cached() before it), then all of them in one mixed
sequence on one context, alternating two image sizes so that the arena's need shrinks and grows;
each output of the sequence must be its isolated twin bit for bit. Then rt.release_cached() twice.

The huge scene at 4 spp, depth 64, default camera; A = 64 x 36, B = 24 x 16 (no whole 8 x 8 tiles).
The filters' and the accumulation's inputs are the isolated renders' own outputs.
"""
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
from support import assert_all_bits, assert_bits  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, SPP, DEPTH = 1234, 4, 64
A, B = (64, 36), (24, 16)
GUIDES = ("albedo", "normal", "depth")
FULL_ROWS = dict(row_offset=1, row_stride=3, full_frame=True)


def params(size, **kw):
    return rt.make_params(size[0], size[1], SPP, DEPTH, SEED, **kw)


def calls(scene, done):
    """name -> (size, function returning (dict of output arrays, stats or None)); `done` holds the
    isolated outputs the filters and the accumulation read."""
    def render_f32(size):
        img, st = rt.render_f32(scene, params(size))
        return {"rgb": img}, st

    def render_rgb8(size):
        img, st = rt.render_rgb8(scene, params(size))
        return {"rgb8": img}, st

    def render_aov(size, planes):
        return rt.render_aov(scene, params(size), None, 0, planes), None

    def render_var(size, **kw):
        rgb, var, st = rt.render_var(scene, params(size, **kw))
        if kw:  # a full frame: the host call writes the rendered rows only
            rgb, var = rgb[kw["row_offset"]::kw["row_stride"]], var[kw["row_offset"]::kw["row_stride"]]
        return {"rgb": rgb, "var": var}, st

    def denoise(beauty, guides, **kw):
        st = abi.RtStats()
        out = rt.denoise(done[beauty]["rgb"], **{n: done[guides][n] for n in GUIDES if guides}, stats=st, **kw)
        return {"out": out}, st

    def denoise_var(var, guides, **kw):
        st = abi.RtStats()
        out, vout = rt.denoise_var(done[var]["rgb"], done[var]["var"], **{n: done[guides][n] for n in GUIDES},
                                   variance_out=True, stats=st, **kw)
        return {"out": out, "variance_out": vout}, st

    def temporal(size, var, aov, with_prev):
        st = abi.RtStats()
        v, g = done[var], done[aov]
        cur = dict(beauty=v["rgb"], variance=v["var"], normal=g["normal"], depth=g["depth"], alpha=g["alpha"],
                   sphere_id=g["sphere_id"])
        prev = dict(color=v["rgb"], variance=v["var"], history=np.ones(size[::-1], dtype=np.float32),
                    normal=g["normal"], depth=g["depth"], sphere_id=g["sphere_id"]) if with_prev else None
        cam = rt.Camera.default(*size)
        color, variance, history = rt.temporal(cur, prev, cam, cam if with_prev else None, stats=st)
        return {"color": color, "variance": variance, "history": history}, st

    return {
        "f32-A": lambda: render_f32(A),
        "rgb8-A": lambda: render_rgb8(A),
        "aov-A": lambda: render_aov(A, tuple(abi.AOV_PLANES)),
        "aov-depth-id-B": lambda: render_aov(B, ("depth", "sphere_id")),
        "var-A": lambda: render_var(A),
        "var-full-rows-A": lambda: render_var(A, **FULL_ROWS),
        "denoise-3-guided-A": lambda: denoise("f32-A", "aov-A", levels=3),
        "denoise-1-bare-B": lambda: denoise("f32-B", None, levels=1),
        "denoise-var-A": lambda: denoise_var("var-A", "aov-A"),
        "temporal-prev-A": lambda: temporal(A, "var-A", "aov-A", True),
        "temporal-first-B": lambda: temporal(B, "var-B", "aov-B", False),
        # the renders at B that the calls above read
        "f32-B": lambda: render_f32(B),
        "var-B": lambda: render_var(B),
        "aov-B": lambda: render_aov(B, tuple(abi.AOV_PLANES)),
    }


# the renders first: the other calls read their outputs
ISOLATED_ORDER = ("f32-A", "rgb8-A", "aov-A", "aov-depth-id-B", "var-A", "var-full-rows-A", "f32-B", "var-B", "aov-B",
                  "denoise-3-guided-A", "denoise-1-bare-B", "denoise-var-A", "temporal-prev-A", "temporal-first-B")
# A and B in turn (the arena's need shrinks, then grows), every call once, the first one again at the end
MIXED_ORDER = ("f32-A", "aov-depth-id-B", "denoise-var-A", "denoise-1-bare-B", "temporal-prev-A", "f32-B", "rgb8-A",
               "temporal-first-B", "aov-A", "var-B", "denoise-3-guided-A", "aov-B", "var-full-rows-A", "var-A", "f32-A")


@pytest.fixture(scope="module")
def runs():
    """(isolated, mixed): name -> (outputs, stats); mixed as a list in MIXED_ORDER. The context is
    left as the mixed sequence left it."""
    scene = rt.huge_scene_arrays(SEED)
    done = {}
    table = calls(scene, done)
    assert set(ISOLATED_ORDER) == set(table) == set(MIXED_ORDER)
    isolated = {}
    for name in ISOLATED_ORDER:
        rt.release_cached()
        isolated[name] = table[name]()
        done[name] = isolated[name][0]
        for a in done[name].values():
            a.setflags(write=False)
    rt.release_cached()
    mixed = [(name, *table[name]()) for name in MIXED_ORDER]
    return isolated, mixed


def test_every_call_of_the_mixed_sequence_equals_its_isolated_twin(runs):
    isolated, mixed = runs
    for name, outputs, _ in mixed:
        want = isolated[name][0]
        assert set(outputs) == set(want)
        assert_all_bits(outputs, want, name)
    # the renders are not trivially equal: something was rendered, and A is not B
    assert isolated["f32-A"][0]["rgb"].any() and isolated["rgb8-A"][0]["rgb8"].any()
    assert isolated["var-full-rows-A"][0]["rgb"].shape == (12, 64, 3)


def test_the_times_of_every_call_with_stats(runs):
    isolated, mixed = runs
    timed = 0
    for name, _, st in list(mixed) + [(n, *isolated[n]) for n in ISOLATED_ORDER]:
        if st is None:
            continue
        timed += 1
        print(f"{name}: kernel_ms {st.kernel_ms:.4f} wall_ms {st.wall_ms:.4f}")
        assert st.kernel_ms > 0 and st.wall_ms >= st.kernel_ms, name
    assert timed == 2 * 11 + 1  # every call but the three feature-buffer renders


def test_release_twice_then_a_render(runs):
    isolated, _ = runs
    rt.release_cached()
    rt.release_cached()
    img, st = rt.render_f32(rt.huge_scene_arrays(SEED), params(B))
    want = isolated["f32-B"][0]["rgb"]
    assert_bits(img, want, "a render after two releases")
    assert st.kernel_ms > 0 and st.wall_ms >= st.kernel_ms
