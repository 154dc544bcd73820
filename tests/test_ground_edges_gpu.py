"""The ground kernel and the redo launch at their edges, on the GPU: every frame bit
for bit against the CPU restatement (tests/oracle_binding.py) of the scene it was rendered from, on
uint32 views with zero mismatches, the segment count equal to the restatement's, and the scene's
ground counts equal to tiles x 64 x spp with the tile count from the host's rt_tile_ground: a frame
that fell back to the main launch fails. tests/test_ground_gpu.py renders one scene family with
lists of one and two spheres, at most 33 samples, and a fresh scene per frame. Here:

  the list      3, 4, 5 and 8 always-tested spheres (kGroundAlways = 8 sizes the kernel's arrays), each
                ball with an albedo of its own (the lookup of the shading record), a ball with a
                negative radius (the normal is (P - C) / r), and the lists that keep the main launch:
                nine spheres, a metal second member, a non-finite sphere
  the parts     a thread takes RT_GROUND_SPT = 32 samples: 31, 32, 64 and 65 samples in one pass, and
                65 in passes of 32 (sample_begin 32 and 64, rotating workspaces)
  a live scene  updates that take the class away, give it back and lengthen the list; a stream of
                frames without host waits whose ground ranges grow and shrink; the 256-slot ring of
                redone counts over two revolutions; the bytes of the redo lists

tests/test_ground_cpu.py shows without a GPU that each case reaches what it claims. `in flight`
(render_streams=3, in_flight=1) plans every pass as beside other renders, all launches on the pass's
stream; `lone split` (deep_min_items=1) splits a pass issued alone, the ground kernel on a stream of
its own. References are computed once per module and shared.
"""
import ctypes as C
import functools
import os
import sys

import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import render as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import golden_io as G  # noqa: E402
import ground_checks as GC  # noqa: E402
import oracle_binding as O  # noqa: E402
from support import assert_bits  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, DEPTH, SEED = 128, 72, 64, 1234
CAMERAS = {"reference": lambda: rt.Camera.default(W, H), "corrected": lambda: rt.Camera.default(W, H, rt.CORRECTED),
           "redo": lambda: GC.redo_camera(W / H)}
LONE_SPLIT = dict(deep_min_items=1)
IN_FLIGHT = dict(render_streams=3, in_flight=1)
RING = 256  # rt_scene::kRing (tests/test_ground_cpu.py pins it)


@functools.lru_cache(maxsize=None)
def scene(which="huge"):
    s, m = G.scene("huge")
    if which == "huge":
        return s, m
    if which == "metal":
        return GC.metal_ground(s, m)
    if which == "grown":
        return GC.grown(s, m)[:2]
    return GC.list_case(s, m, which)


@functools.lru_cache(maxsize=None)
def oracle(which, camera, spp):
    s, m = scene(which)
    img, seg = O.render_f32(s, m, CAMERAS[camera]().c, rt.make_params(W, H, spp, DEPTH, SEED))
    img.flags.writeable = False
    return img, int(seg)


@functools.lru_cache(maxsize=None)
def tiles(which, camera):
    """The pass's ground tiles, from the host's classification (no GPU)."""
    return rt.tile_ground(scene(which), rt.make_params(W, H, 4, DEPTH, SEED), CAMERAS[camera]())


def violation(ds):
    """Word [15] of rt_scene_debug_counters: the instrumented kernels' first bounds violation, 0 = none."""
    dbg = (C.c_uint64 * 16)()
    R.check(rt.lib().rt_scene_debug_counters(ds.handle, dbg, 1))
    return int(dbg[15])


class Frames:
    """One live rt.DeviceScene and frames of it: render() enqueues, nothing here waits."""

    def __init__(self, which, options):
        self.ds = rt.DeviceScene(scene(which), device=0, options=rt.options(**options))
        self.held = []

    def render(self, camera, spp, stream=None, count=True):
        """(frame, segment counters or None: the kernels' instantiations without them, as a caller
        that passes no d_segments runs them)."""
        import torch
        st = stream or torch.cuda.current_stream()
        with torch.cuda.stream(st):
            out = torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda:0")
            seg = torch.zeros(3, dtype=torch.int64, device="cuda:0") if count else None
        self.ds.render(CAMERAS[camera](), rt.make_params(W, H, spp, DEPTH, SEED), out.data_ptr(), st.cuda_stream,
                       d_segments=seg.data_ptr() if count else None)
        self.held.append((out, seg))
        return out, seg

    def close(self):
        self.ds.close()


def check_frame(out, seg, which, camera, spp, what):
    ref, ref_seg = oracle(which, camera, spp)
    assert_bits(out.cpu().numpy(), ref, what)
    if seg is not None:
        assert int(seg[0].item()) == ref_seg, what


def one_frame(which, camera, spp, options, what, stats=False, uncounted_too=False):
    """A frame on a fresh scene with the segment counters, compared (bits and segments); returns
    ((ground, redone), usage). uncounted_too: then the same frame again on that scene without the
    counters (the kernels' instantiations a caller that passes no d_segments runs): the same bits
    and the same ground counts."""
    import torch
    f = Frames(which, dict(options, stats=True) if stats else options)
    try:
        out, seg = f.render(camera, spp)
        torch.cuda.synchronize()
        counts, usage = f.ds.ground_counts(), f.ds.usage()
        if stats:
            assert violation(f.ds) == 0
        if uncounted_too:
            out2, _ = f.render(camera, spp, count=False)
            torch.cuda.synchronize()
            counts2 = f.ds.ground_counts()
    finally:
        f.close()
    print(f"{what}: {counts[0]} ground samples, {counts[1]} redone, pass of {usage['pass_samples']} samples")
    check_frame(out, seg, which, camera, spp, what)
    if uncounted_too:
        check_frame(out2, None, which, camera, spp, what + ", without the counters")
        assert counts2 == counts
    return counts, usage


# ---- 1. sizes and members of the always-tested list ------------------------------------------------
@pytest.mark.parametrize("name", list(GC.LIST_CASES))
def test_always_tested_lists(name):
    """128x72, 5 spp, in flight, the default camera, which sees every ball in ground tiles
    (tests/test_ground_cpu.py::test_list_cases_reach_the_list). A list the class admits gives
    tiles x 64 x 5 ground samples, some of them redone (paths from a ball to the ground or the field
    have three segments and more) and some not (ground tiles have sky samples); the others (0, 0).
    (n4 and n8 a second time without the segment counters.)"""
    spp = 5
    takes = GC.LIST_CASES[name][2]
    n_tiles = tiles(name, "reference")
    assert (n_tiles > 0) == takes
    (ground, redone), _ = one_frame(name, "reference", spp, IN_FLIGHT, f"list {name}", uncounted_too=name in ("n4", "n8"))
    assert ground == n_tiles * 64 * spp
    if takes:
        assert 0 < redone < ground
    else:
        assert (ground, redone) == (0, 0)


# ---- 2. sample parts and rings -----------------------------------------------------------------------
PASS_32 = dict(IN_FLIGHT, max_pass_bytes=32 * W * H * 12)  # passes [0, 32), [32, 64), [64, 65)


@pytest.mark.parametrize("how,spp", [("lone", 31), ("lone", 32), ("lone", 64), ("lone", 65), ("passes", 65), ("stats", 65)])
def test_sample_parts(how, spp):
    """The redo camera (85 ground tiles, part of their samples redone). One pass of 31, 32, 64 and 65
    samples: one part short of full, one full, two full, and a third of a single sample; 65 samples
    in flight in passes of 32, the later ones with sample_begin 32 and 64 in the next workspaces; 65
    with the instrumented instantiations (BC_SLOT, BC_REDO_APPEND, BC_REDO_ITEM: no violation). (32 and
    64 in one pass a second time without the segment counters.)"""
    options = PASS_32 if how == "passes" else LONE_SPLIT
    (ground, redone), usage = one_frame("huge", "redo", spp, options, f"redo camera, {how}, spp {spp}", stats=how == "stats",
                                        uncounted_too=(how, spp) in (("lone", 32), ("lone", 64)))
    assert usage["pass_samples"] == (32 if how == "passes" else spp)
    assert tiles("huge", "redo") == 85
    assert ground == 85 * 64 * spp
    assert 0 < redone < ground


# ---- 3. one live scene, many frames -------------------------------------------------------------------
def test_updates_keep_the_class_in_step_with_the_scene():
    """rt_scene_update re-derives ground_ok: a metal ground takes the class away (the counts stay
    those of the last frame that used it, include/rt_api.h), the lambert ground gives it back with
    the first frame's bits and counts, a sphere grown past 64 times the median radius lengthens the
    list to two with the sphere count fixed, and shrinking it returns to the first frame again."""
    import torch
    spp = 5
    steps = ["huge", "metal", "huge", "grown", "huge"]
    assert [tiles(w, "reference") > 0 for w in steps] == [True, False, True, True, True]
    assert tiles("grown", "reference") != tiles("huge", "reference")
    f = Frames("huge", IN_FLIGHT)
    try:
        counts = []
        for i, which in enumerate(steps):
            if i:
                f.ds.update(scene(which))
            out, seg = f.render("reference", spp)
            torch.cuda.synchronize()
            counts.append(f.ds.ground_counts())
            print(f"step {i} ({which}): counts {counts[-1]}")
            check_frame(out, seg, which, "reference", spp, f"step {i} ({which})")
    finally:
        f.close()
    first = counts[0]
    assert first[0] == tiles("huge", "reference") * 64 * spp and first[1] < first[0]
    assert counts[1] == first  # the metal frame used no ground kernel
    assert counts[2] == first
    assert counts[3][0] == tiles("grown", "reference") * 64 * spp and 0 < counts[3][1] < counts[3][0]
    assert counts[3] != first
    assert counts[4] == first


@functools.lru_cache(maxsize=None)
def lone_counts(camera, spp):
    """The counts of that frame on a fresh scene (bit-exact frames redo the same samples)."""
    return one_frame("huge", camera, spp, IN_FLIGHT, f"{camera} camera alone")[0]


@pytest.mark.parametrize("capped", [False, True], ids=["uncapped", "capped"])
def test_frame_stream_without_host_waits(capped):
    """12 frames of 5 spp alternating over two caller streams, the cameras cycling through 20, 85 and
    15 ground tiles (the redo lists grow, then are reused smaller), a buffer per frame, one wait at
    the end. Capped: max_workspace_bytes for three workspaces of 4-sample passes (as
    tests/test_ground_gpu.py::test_several_passes derives its cap), so a frame is two passes and the
    workspaces and their redo lists go round across frames."""
    import torch
    spp, n_frames = 5, 12
    cams = ["reference", "redo", "corrected"]
    assert [tiles("huge", c) for c in cams] == [20, 85, 15]
    options = dict(IN_FLIGHT)
    if capped:
        options.update(max_workspace_bytes=3 * (4 * W * H * 12 + (256 << 10)) + 2 * W * H * 12, no_pairs=1)
    want_last = lone_counts(cams[(n_frames - 1) % 3], spp)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    f = Frames("huge", options)
    try:
        frames = [f.render(cams[k % 3], spp, streams[k % 2]) for k in range(n_frames)]
        torch.cuda.synchronize()
        counts, usage = f.ds.ground_counts(), f.ds.usage()
    finally:
        f.close()
    print("usage", usage, "counts", counts)
    for k, (out, seg) in enumerate(frames):
        check_frame(out, seg, "huge", cams[k % 3], spp, f"frame {k} ({cams[k % 3]})")
    if capped:
        assert usage["pass_samples"] < spp and usage["pair_passes"] == 0
    else:
        assert usage["pass_samples"] == spp
    assert counts[0] == tiles("huge", cams[(n_frames - 1) % 3]) * 64 * spp
    assert counts == want_last and counts[1] < counts[0]


def test_count_ring_over_two_revolutions():
    """The same 1-spp frame of the redo camera 2 x 256 + 3 times on one scene: the frame's slot of the
    256-slot ring of redone counts is zeroed half a ring ahead of its use. The counts after frames 1,
    128, 129, 256, 257 (the first reuse of a slot: one not zeroed gives twice the count) and the last
    are the first frame's; the device is waited for at those reads only."""
    import torch
    reads = (1, RING // 2, RING // 2 + 1, RING, RING + 1, 2 * RING + 3)
    f = Frames("huge", IN_FLIGHT)
    try:
        out = torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda:0")
        seg = torch.zeros(3, dtype=torch.int64, device="cuda:0")
        cam, p = CAMERAS["redo"](), rt.make_params(W, H, 1, DEPTH, SEED)
        st = torch.cuda.current_stream().cuda_stream
        got = {}
        for k in range(1, reads[-1] + 1):  # (the segment counters with the last frame only)
            f.ds.render(cam, p, out.data_ptr(), st, d_segments=seg.data_ptr() if k == reads[-1] else None)
            if k in reads:
                got[k] = f.ds.ground_counts()
        torch.cuda.synchronize()
    finally:
        f.close()
    print("counts", got)
    check_frame(out, seg, "huge", "redo", 1, "the last frame")
    assert got[1][0] == 85 * 64 and 0 < got[1][1] < got[1][0]
    assert all(got[k] == got[1] for k in reads), got


def test_redo_lists_are_counted_beside_the_workspaces():
    """rt_scene_usage: device_bytes - workspace_bytes holds the redo lists (4 B per ground sample of
    the largest pass) and the ring of counts (1 KiB), workspace_bytes does not.
    Against the same frame on a scene that keeps its ground tiles in the main launch (no_sky)."""
    import torch
    spp = 8
    grew = {}
    for name, options in (("ground", IN_FLIGHT), ("main launch", dict(IN_FLIGHT, no_sky=1))):
        f = Frames("huge", options)
        try:
            before = f.ds.usage()
            out, seg = f.render("redo", spp)
            torch.cuda.synchronize()
            after, counts = f.ds.usage(), f.ds.ground_counts()
        finally:
            f.close()
        check_frame(out, seg, "huge", "redo", spp, name)
        assert after["pass_samples"] == spp
        grew[name] = ((after["device_bytes"] - after["workspace_bytes"]) - (before["device_bytes"] - before["workspace_bytes"]),
                      after["workspace_bytes"] - before["workspace_bytes"], counts)
    print("bytes beside the workspaces, workspace bytes, counts:", grew)
    assert grew["main launch"][2] == (0, 0) and grew["ground"][2][0] == 85 * 64 * spp
    lists = 4 * 85 * 64 * spp + 4 * RING
    assert grew["ground"][0] >= lists and grew["ground"][0] - grew["main launch"][0] >= lists
    assert grew["ground"][1] == grew["main launch"][1]
