"""The temporal stage with object motion on the GPU (rt_temporal_motion, rt_temporal_motion_device,
DESIGN.md §4.16) against its numpy restatement (tests/tools/temporal_motion_ref.py) and against the
static stage.

Every comparison is on uint32 views with zero mismatches allowed. Frames are rendered once per module
and shared; the conditions that make a case meaningful are checked on the restatement's result alone.
"""
import functools
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import temporal_motion_ref as M  # noqa: E402
import temporal_ref as T  # noqa: E402
from device_io import SENTINEL  # noqa: E402
from support import STILL, frame_planes, shifted_camera  # noqa: E402
from support import assert_all_bits as assert_all_same, words as u32  # noqa: E402
from support import census as reason_census  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SCENE_SEED = 1234
SPP = 4
MODES = {"reference": rt.REFERENCE, "corrected": rt.CORRECTED}
# The default camera's position and look-at point. In REFERENCE mode a ray's direction is the image-plane
# point itself and that camera sees none of the moved spheres: there the camera stands in front of the
# three large spheres and looks at a far point below them, which puts spheres 2 and 3 on some 400 pixels
# each at 64 x 36 (found with a first-hit tracer on the CPU).
VIEW = {rt.CORRECTED: ((-4.0, 3.2, 5.0), (0.0, 1.0, 0.0)), rt.REFERENCE: ((0.0, 1.5, 3.0), (0.0, -2.0, -12.0))}
CAMERA_MOVE = ((0.1, 0.05, -0.05), (0.15, 0.05, 0.0))  # a small move: most of the frame stays on screen
MOVED_IDS = (2, 3, 4)               # the metal sphere, the glass sphere and its bubble
SHIFT = (0.0, 0.0, 0.15)            # about one pixel at 64x36
CUR = ("beauty", "variance", "normal", "depth", "alpha", "sphere_id")
PREV = ("color", "variance", "history", "normal", "depth", "sphere_id")
SIZES = ((64, 36), (48, 27))


@functools.lru_cache(maxsize=None)
def records(which):
    """A: the huge scene. B: spheres 2, 3 and 4 shifted by SHIFT. R: B with sphere 2's radius changed too."""
    s, m = rt.huge_scene_arrays(SCENE_SEED)
    if which != "A":
        s = s.copy()
        for i in MOVED_IDS:
            s["center"][i] = s["center"][i] + np.array(SHIFT, dtype=F)
        if which == "R":
            s["radius"][2] = F(0.9)
    return s, m


def camera(w, h, mode, shift=STILL):
    return shifted_camera(w, h, mode, shift, VIEW[mode])


@functools.lru_cache(maxsize=None)
def frame(which, w, h, mode, seed, shift=STILL):
    return frame_planes(records(which), rt.make_params(w, h, SPP, 64, seed), camera(w, h, mode, shift), SPP,
                        ("normal", "depth", "alpha", "sphere_id"))


def cur_of(f):
    return {n: f[n] for n in CUR}


def prev_of(f):
    h, w = f["variance"].shape
    return dict(color=f["beauty"], variance=f["variance"], history=np.full((h, w), F(2)),
                normal=f["normal"], depth=f["depth"], sphere_id=f["sphere_id"])


census = functools.partial(reason_census, reasons=M.REASONS)


def device_call(cur, prev, cam, prev_cam, par, tables, same_table=False, static=False):
    """rt_temporal_motion_device (static: rt_temporal_device) on a torch stream of its own into
    sentinel-filled outputs; the tables are device tensors."""
    import torch
    h, w = cur["variance"].shape

    def up(a):
        a = np.array(a)
        return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")

    t = {n: up(cur[n]) for n in CUR}
    if prev is not None:
        t.update({"prev_" + n: up(prev[n]) for n in PREV})
    out = {n: torch.full((h, w, 3) if n == "out_color" else (h, w), SENTINEL, dtype=torch.float32, device="cuda:0")
           for n in ("out_color", "out_variance", "out_history")}
    now = up(tables[0])
    was = now if same_table else up(tables[1])
    motion = None if static else (now.data_ptr() if len(tables[0]) else 0, was.data_ptr() if len(tables[0]) else 0,
                                  len(tables[0]))
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        rt.temporal_device({n: a.data_ptr() for n, a in {**t, **out}.items()}, par, cam, prev_cam, st.cuda_stream,
                           motion=motion)
    st.synchronize()
    return tuple(out[n].cpu().numpy() for n in ("out_color", "out_variance", "out_history"))


def params(w, h):
    return rt.temporal_params(w, h, alpha_min=0.2, max_history=32.0, normal_tol=0.1, depth_tol=0.1)


# ---- 1: zero motion ------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_zero_motion_is_the_static_stage_bit_for_bit(w, h):
    m = rt.CORRECTED
    f1, f2 = frame("A", w, h, m, 1), frame("A", w, h, m, 2, CAMERA_MOVE)
    cam, prev_cam, par = camera(w, h, m, CAMERA_MOVE), camera(w, h, m), params(w, h)
    table = rt.sphere_table(records("A"))
    want = rt.temporal(cur_of(f2), prev_of(f1), cam, prev_cam, par)
    assert (want[2] > 1).sum() > 100          # histories are kept: the case says something
    assert_all_same(rt.temporal(cur_of(f2), prev_of(f1), cam, prev_cam, par, motion=(table, table.copy())), want, "host")
    want_d = device_call(cur_of(f2), prev_of(f1), cam, prev_cam, par, (table, table), static=True)
    assert_all_same(want_d, want, "static device")
    assert_all_same(device_call(cur_of(f2), prev_of(f1), cam, prev_cam, par, (table, table.copy())), want, "device")
    assert_all_same(device_call(cur_of(f2), prev_of(f1), cam, prev_cam, par, (table, table), same_table=True), want,
                    "device, one table twice")


# ---- 2: moved spheres ----------------------------------------------------------------------------------
CASES = [(mode, w, h, move) for mode in sorted(MODES) for (w, h) in SIZES for move in ("still", "moved-camera")
         if (w, h) == SIZES[0] or move == "still"]


@pytest.mark.parametrize("mode,w,h,move", CASES)
def test_moved_spheres(mode, w, h, move):
    m, shift = MODES[mode], CAMERA_MOVE if move == "moved-camera" else STILL
    f1, f2 = frame("A", w, h, m, 1), frame("B", w, h, m, 2, shift)
    cam, prev_cam, par = camera(w, h, m, shift), camera(w, h, m), params(w, h)
    now, was = rt.sphere_table(records("B")), rt.sphere_table(records("A"))
    ref = M.accumulate(cur_of(f2), prev_of(f1), cam, prev_cam, par, now, was)
    c = census(ref[3])
    on_moved = np.isin(f2["sphere_id"], MOVED_IDS)
    kept_moved = int((on_moved & (ref[3] == M.KEPT)).sum())
    print("pixels on a moved sphere:", int(on_moved.sum()), "of those kept:", kept_moved)
    assert kept_moved >= 20
    assert c["edge"] >= 1 and c["all taps rejected"] >= 1
    assert_all_same(rt.temporal(cur_of(f2), prev_of(f1), cam, prev_cam, par, motion=(now, was)), ref[:3], "host")
    assert_all_same(device_call(cur_of(f2), prev_of(f1), cam, prev_cam, par, (now, was)), ref[:3], "device")
    # the static stage on the same inputs gives something else
    static = T.accumulate(cur_of(f2), prev_of(f1), cam, prev_cam, par)
    differ = int((u32(static[0]) != u32(ref[0])).any(axis=2).sum())
    print("pixels where the static stage differs:", differ)
    assert differ > 20


def test_a_resized_sphere_restarts():
    w, h, m = 64, 36, rt.CORRECTED
    f1, f2 = frame("A", w, h, m, 1), frame("R", w, h, m, 2)
    cam, par = camera(w, h, m), params(w, h)
    now, was = rt.sphere_table(records("R")), rt.sphere_table(records("A"))
    ref = M.accumulate(cur_of(f2), prev_of(f1), cam, cam, par, now, was)
    c = census(ref[3])
    assert c["resized or unknown sphere"] >= 1
    assert ((ref[3] == M.RESIZED) <= (f2["sphere_id"] == 2)).all()
    assert_all_same(rt.temporal(cur_of(f2), prev_of(f1), cam, cam, par, motion=(now, was)), ref[:3], "host")
    assert_all_same(device_call(cur_of(f2), prev_of(f1), cam, cam, par, (now, was)), ref[:3], "device")


# ---- 3: ids outside the tables, bad values in rows no pixel names --------------------------------------
def test_out_of_range_ids_and_bad_table_values():
    w, h, m = 48, 27, rt.CORRECTED
    f1, f2 = frame("A", w, h, m, 1), frame("A", w, h, m, 2)
    cam, par = camera(w, h, m), params(w, h)
    n = 8
    g = np.random.default_rng(9)
    sid = g.integers(0, 12, size=(h, w)).astype(np.uint32)   # ids 0..11: 8..11 are outside the tables
    sid[sid == 5] = 6                                        # no pixel names row 5
    sid[0, :4] = (0xffffffff, 0x80000000, n, n - 1)
    sid[f2["alpha"] == 0] = 0xffffffff
    cur = dict(cur_of(f2), sphere_id=sid)
    prev = dict(prev_of(f1), sphere_id=sid.copy())
    now = g.normal(size=(n, 4)).astype(F) * F(0.05)
    was = now.copy()
    was[:, :3] += g.normal(size=(n, 3)).astype(F) * F(0.02)
    # the row no pixel names is full of NaN. (A NaN in a row a pixel names gives unspecified values.)
    now[5] = was[5] = np.nan
    assert sorted(np.unique(sid[sid < n])) == [0, 1, 2, 3, 4, 6, 7]
    ref = M.accumulate(cur, prev, cam, cam, par, now, was)
    c = census(ref[3])
    assert c["resized or unknown sphere"] >= 50 and c["kept"] >= 50
    got = device_call(cur, prev, cam, cam, par, (now, was))
    assert_all_same(got, ref[:3], "device")
    assert not any((a == SENTINEL).any() for a in got)
    assert_all_same(rt.temporal(cur, prev, cam, cam, par, motion=(now, was)), ref[:3], "host")
    # no sphere at all: every surface pixel restarts, the sky keeps its history
    empty = np.zeros((0, 4), dtype=F)
    ref0 = M.accumulate(cur, prev, cam, cam, par, empty, empty)
    assert (ref0[3][f2["alpha"] == 1] == M.RESIZED).all()
    assert_all_same(device_call(cur, prev, cam, cam, par, (empty, empty)), ref0[:3], "device, no sphere")
    assert_all_same(rt.temporal(cur, prev, cam, cam, par, motion=(empty, empty)), ref0[:3], "host, no sphere")


# ---- 4: aliased tables ------------------------------------------------------------------------------------
def test_aliased_tables_are_refused_and_nothing_is_written():
    import torch
    w, h = 16, 8
    n = w * h * 3 // 4          # a table as large as out_color
    planes = {name: torch.full((h, w, 3) if name in ("beauty", "normal", "prev_color", "prev_normal", "out_color") else (h, w),
                               SENTINEL, dtype=torch.float32, device="cuda:0")
              for name in ("beauty", "variance", "normal", "depth", "alpha", "prev_color", "prev_variance", "prev_history",
                           "prev_normal", "prev_depth", "out_color", "out_variance", "out_history")}
    for name in ("sphere_id", "prev_sphere_id"):
        planes[name] = torch.zeros((h, w), dtype=torch.int32, device="cuda:0")
    table = torch.full((n, 4), SENTINEL, dtype=torch.float32, device="cuda:0")
    cam, par = rt.Camera.default(w, h), rt.temporal_params(w, h)
    ptr = {k: a.data_ptr() for k, a in planes.items()}
    for motion in ((ptr["out_color"], table.data_ptr(), n), (table.data_ptr(), ptr["out_color"], n),
                   (table.data_ptr(), ptr["out_history"], 4)):
        with pytest.raises(rt.RtError) as e:
            rt.temporal_device(ptr, par, cam, cam, motion=motion)
        assert e.value.status == -1 and "motion." in str(e.value) and "output plane" in str(e.value)
    torch.cuda.synchronize()
    assert all((a == SENTINEL).all() for k, a in planes.items() if k.startswith("out_")) and (table == SENTINEL).all()
