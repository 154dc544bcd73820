"""Trap windows on the device: a path that reflects totally inside an isolated
glass ball with its cosine in the ball's window is ended at once with colour 0, as if its depth
had run out. Every render here is at most 64x40 and is compared bit for bit with the CPU
restatement, its segment count included, with the trigger and without it (diag no_trap_end)."""
import functools
import os
import sys

import numpy as np
import pytest

import golden_io as G
import oracle_binding as O
import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
from support import assert_bits as _bits_equal  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 64, 40


def _materials():
    m = np.zeros(4, dtype=abi.MATERIAL_DTYPE)
    m[0] = (0, [0.5, 0.5, 0.5], 0.0)
    m[1] = (2, [1.0, 1.0, 1.0], 1.5)
    m[2] = (2, [1.0, 1.0, 1.0], 1.33)
    m[3] = (1, [0.7, 0.6, 0.5], 0.1)
    return m


def _one_ball(ior=1.5, resting=False):
    """A glass ball of radius 0.2 at (0, 0.2, 0) over the ground (half a unit below it, or touching it)."""
    s = np.zeros(2, dtype=abi.SPHERE_DTYPE)
    s[0] = ((0, -1000.0 if resting else -1000.5, 0), 1000.0, 0)
    s[1] = ((0, 0.2, 0), 0.2, 1 if ior == 1.5 else 2)
    return s, _materials()


def _ball_camera():
    """Looks at the ball from 1.24 away: it fills about three quarters of the frame's height."""
    pos, look = (0.0, 0.5, 1.2), (0.0, 0.2, 0.0)
    focus = float(np.linalg.norm(np.subtract(pos, look)))
    return rt.Camera(pos, look, (0, 1, 0), W / H, 24.0, 0.02, focus, rt.CORRECTED)


def _glass_scene():
    """Glass balls floating over the ground in front of the corrected default camera: isolated ones,
    touching and overlapping pairs, a ball with a bubble, exact duplicates, a ball inside the big
    glass sphere, a ball resting on the ground, lambert and metal balls."""
    rng = np.random.default_rng(11)
    balls = [((0, -1000.2, 0), 1000.0, 0), ((0, 1.2, 0), 1.0, 1), ((0.3, 1.3, 0.1), 0.2, 1)]
    for gx in range(-3, 4):
        for gz in range(-3, 4):
            if abs(gx) <= 1 and abs(gz) <= 1:
                continue
            r = float(rng.choice([0.2, 0.2, 0.1, 0.3]))
            c = (gx * 1.3 + float(rng.uniform(-0.2, 0.2)), r + 0.05, gz * 1.3 + float(rng.uniform(-0.2, 0.2)))
            balls.append((c, r, int(rng.choice([1, 1, 2, 0, 3]))))
    balls.append(((-0.4 + 0.4, 0.25, 1.9), 0.2, 1))   # touching pair
    balls.append(((-0.4, 0.25, 1.9), 0.2, 2))
    balls.append(((0.9 + 0.2, 0.25, 2.4), 0.2, 1))    # overlapping pair
    balls.append(((0.9, 0.25, 2.4), 0.2, 1))
    balls.append(((-1.2, 0.3, 2.6), 0.25, 1))         # a ball with a bubble
    balls.append(((-1.2, 0.3, 2.6), -0.2, 1))
    balls.append(((1.8, 0.3, 1.7), 0.2, 2))           # exact duplicates
    balls.append(((1.8, 0.3, 1.7), 0.2, 2))
    # resting on the ground (the ground sphere's surface at x = -2, z = 2 lies a little below y = -0.2)
    balls.append(((-2.0, -1000.2 + float(np.sqrt(1000.2 ** 2 - 8.0)), 2.0), 0.2, 1))
    s = np.zeros(len(balls), dtype=abi.SPHERE_DTYPE)
    for i, b in enumerate(balls):
        s[i] = b
    return s, _materials()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(spheres, materials), camera record"""
    if name == "ball":
        return _one_ball(), _ball_camera().c
    if name == "ball133":
        return _one_ball(ior=1.33), _ball_camera().c
    if name == "resting":
        return _one_ball(resting=True), _ball_camera().c
    if name == "glass":
        return _glass_scene(), O.camera_default(W, H, abi.RT_CAMERA_CORRECTED)
    assert name == "huge"
    return G.scene("huge"), O.camera_default(64, 36)


@functools.lru_cache(maxsize=None)
def _oracle(name, w, h, spp, depth, seed=21):
    (s, m), cam = _case(name)
    img, seg = O.render_f32(s, m, cam, rt.make_params(w, h, spp, depth, seed))
    img.setflags(write=False)
    return img, seg


def _both(name, w, h, spp, depth, opts, seed=21, **flags):
    """(stats with the trigger, stats without it); both frames equal the restatement's"""
    (s, m), cam = _case(name)
    want, seg = _oracle(name, w, h, spp, depth, seed)
    st = []
    for off in (False, True):
        opts.set(no_trap_end=off)
        img, stats = rt.render_f32((s, m), rt.make_params(w, h, spp, depth, seed, **flags), cam)
        _bits_equal(img, want, f"{name} no_trap_end={off}")
        assert stats.segments == seg, (name, off, stats.segments, seg)
        st.append(stats)
    opts.set(no_trap_end=False)
    return st


@pytest.mark.parametrize("name,w,h,spp,fires", [("ball", W, H, 16, True), ("ball133", W, H, 16, True),
                                                ("resting", W, H, 16, False), ("glass", W, H, 8, True),
                                                ("huge", 64, 36, 8, None)])
def test_frames_match_the_restatement(name, w, h, spp, fires, opts):
    on, off = _both(name, w, h, spp, 64, opts)
    assert on.sphere_tests <= off.sphere_tests
    if fires is True:
        assert on.sphere_tests < off.sphere_tests, "the trigger never fired"
    if fires is False:
        assert on.sphere_tests == off.sphere_tests and on.box_tests == off.box_tests


def test_windows_of_the_cases():
    """The scenes above have the windows they are meant to have (the host routine, no device)."""
    w = rt.trap_windows(_case("ball")[0])
    assert w[1, 0] < 0.03 and w[1, 1] > 0.73
    w = rt.trap_windows(_case("resting")[0])
    assert (w[:, 0] > w[:, 1]).all()
    w = rt.trap_windows(_case("glass")[0])
    assert w[2, 0] <= w[2, 1]                      # the ball inside the big glass sphere
    assert (w[-9:, 0] > w[-9:, 1]).all()           # pairs, bubble, duplicates, the resting ball


@pytest.mark.parametrize("depth", [1, 2, 3, 8, 9, 64, 65])
def test_depths_on_the_one_ball_scene(depth, opts):
    """Depth 8 / 9 is the split boundary (deep_split 8, passes of any size split); a trigger on the
    last shaded bounce adds one segment, the one the path would still trace; above the windows'
    depth bound (64) the trigger is off."""
    opts.set(deep_min_items=0)
    on, off = _both("ball", W, H, 16, depth, opts)
    if depth > 64:
        assert on.sphere_tests == off.sphere_tests
    elif depth >= 8:
        assert on.sphere_tests < off.sphere_tests


def test_executed_tests_drop_segments_do_not(opts):
    """The counting frame of a one-ball render: the device ran fewer sphere tests with the trigger
    (it ended paths), while `segments` stays the restatement's hit_world count."""
    on, off = _both("ball", W, H, 16, 64, opts)
    assert on.segments == off.segments
    assert on.sphere_tests < off.sphere_tests, (on.sphere_tests, off.sphere_tests)


@pytest.mark.parametrize("diag", [dict(pairs=True, in_flight=True, deep_split=3), dict(in_flight=True),
                                  dict(deep_split=3), dict(deep_split=0), dict(shade_global=True),
                                  dict(shade_lds=True), dict(stats=True)])
def test_variants_of_the_pass_plan(diag, opts):
    """The sample-pair instantiation, passes planned in flight, split depths around the trigger's
    usual segment, both placements of the shading records and the instrumented kernel."""
    opts.set(deep_min_items=0, **diag)
    for name, spp in (("ball", 16), ("glass", 8)):
        on, off = _both(name, W, H, spp, 64, opts)
        assert on.sphere_tests < off.sphere_tests


def test_brute_force_and_scalar_scene(opts):
    for flags in (dict(brute_force=True), dict(scalar_scene=True)):
        on, off = _both("glass", W, H, 8, 64, opts, **flags)
        assert on.sphere_tests < off.sphere_tests


def test_lone_split_pass_takes_the_deep_launch(opts):
    """A split pass of the huge scene issued alone with the shading records in global memory runs
    the 8-wave deep launch (rt_scene_usage.deep_launch 8 | 16; a small scene keeps the 4-wave one),
    split after 2 segments so that the trigger fires there: same frame, same segments."""
    torch = pytest.importorskip("torch")
    opts.set(deep_min_items=0, shade_global=True, deep_split=2)
    (s, m), cam = _case("huge")
    want, seg = _oracle("huge", 64, 36, 8, 64)
    stream = torch.cuda.current_stream().cuda_stream
    tests = []
    for off in (False, True):
        opts.set(no_trap_end=off)
        ds = rt.DeviceScene((s, m))
        out = torch.empty((36, 64, 3), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
        ds.render(cam, rt.make_params(64, 36, 8, 64, 21), out.data_ptr(), stream, cnt.data_ptr())
        torch.cuda.synchronize()
        u = ds.usage()
        ds.close()
        assert u["deep_launch"] == 8 | 16 and u["split_passes"] >= 1, u
        _bits_equal(out.cpu().numpy(), want, f"lone no_trap_end={off}")
        assert int(cnt[0]) == seg
        tests.append(int(cnt[1]))
    assert tests[0] < tests[1], tests


# the fast kernel's stated tolerance (tests/test_gpu_parity.py): >= 99% of pixels within 1e-4 on
# the linear frame, mean |d| <= 1e-4
def test_fast_variant_within_its_tolerance(opts):
    (s, m), cam = _case("huge")
    want, _ = _oracle("huge", 64, 36, 8, 64)
    for off in (False, True):
        opts.set(no_trap_end=off)
        img, _ = rt.render_f32((s, m), rt.make_params(64, 36, 8, 64, 21, fast_math=True), cam)
        d = np.abs(img - want)
        assert float((d.max(axis=-1) <= 1e-4).mean()) >= 0.99 and float(d.mean()) <= 1e-4
        assert np.isfinite(img).all()


def test_wavefront_variant_matches_megakernel(opts):
    for name, spp in (("ball", 16), ("glass", 8)):
        (s, m), cam = _case(name)
        a, sa = rt.render_f32((s, m), rt.make_params(W, H, spp, 64, 21), cam)
        b, sb = rt.render_f32((s, m), rt.make_params(W, H, spp, 64, 21, wavefront=True), cam)
        _bits_equal(a, b, name)
        assert sa.segments == sb.segments == _oracle(name, W, H, spp, 64)[1]
