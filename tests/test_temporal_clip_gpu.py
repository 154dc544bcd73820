"""The temporal stage's history clamp on the GPU (rt_temporal_clip, rt_temporal_clip_device, DESIGN.md
§4.17) against its numpy restatement (tests/tools/temporal_clip_ref.py).

Every comparison is on uint32 views with zero mismatches allowed. The planes are synthetic
(tests/tools/clip_cases.py, which says why the sizes 5 x 3, 70 x 37 and 129 x 9 were chosen and how the
ids lie across the workgroup borders); the restatement runs once per case and is shared. The condition
that makes a case meaningful (more than a tenth of the pixels with history have a channel changed by
the clamp, more than a tenth have none changed) is asserted on the restatement's result.
"""
import functools
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import clip_cases  # noqa: E402
import temporal_clip_ref as R  # noqa: E402
from device_io import SENTINEL  # noqa: E402
from support import assert_all_bits as assert_all_same, assert_bits, words as u32  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
CUR = ("beauty", "variance", "normal", "depth", "alpha", "sphere_id")
PREV = ("color", "variance", "history", "normal", "depth", "sphere_id")
OUT = ("out_color", "out_variance", "out_history")
CASES = [(w, h, r, m) for (w, h) in clip_cases.SIZES for r in clip_cases.RADII for m in (False, True)]
IDS = [f"{w}x{h}-r{r}-{'motion' if m else 'static'}" for w, h, r, m in CASES]


@functools.lru_cache(maxsize=None)
def reference(w, h, radius, motion):
    cur, prev, cam, prev_cam = clip_cases.planes(w, h)
    tabs = clip_cases.tables() if motion else (None, None)
    return R.accumulate(cur, prev, cam, prev_cam, clip_cases.params(w, h), clip_cases.clip(radius), *tabs)


def device_call(cur, prev, cam, prev_cam, par, clip, tables=None, sink=None):
    """rt_temporal_clip_device (clip None: rt_temporal_device / rt_temporal_motion_device) on a torch
    stream of its own into sentinel-filled outputs. Returns the outputs and whether every input plane
    and table still holds the bits that were uploaded. sink: a dict that takes the output tensors before
    the call is made (for a call that raises)."""
    import torch
    h, w = cur["variance"].shape

    def up(a):
        a = np.array(a)  # a writable copy (the shared planes are read-only)
        return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")

    t = {n: up(cur[n]) for n in CUR}
    if prev is not None:
        t.update({"prev_" + n: up(prev[n]) for n in PREV})
    motion = None
    if tables is not None:
        t["centres"], t["prev_centres"] = up(tables[0]), up(tables[1])
        motion = (t["centres"].data_ptr(), t["prev_centres"].data_ptr(), len(tables[0]))
    keep = {n: a.clone() for n, a in t.items()}
    out = {n: torch.full((h, w, 3) if n == "out_color" else (h, w), SENTINEL, dtype=torch.float32, device="cuda:0")
           for n in OUT}
    if sink is not None:
        sink.update(out)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ptrs = {n: a.data_ptr() for n, a in {**t, **out}.items() if n not in ("centres", "prev_centres")}
        rt.temporal_device(ptrs, par, cam, prev_cam, st.cuda_stream, motion=motion, clip=clip)
    st.synchronize()
    intact = all(torch.equal(t[n], keep[n]) for n in t)
    return tuple(out[n].cpu().numpy() for n in OUT), intact


# ---- 1: the device and the host call against the restatement ---------------------------------------------
@pytest.mark.parametrize("w,h,radius,motion", CASES, ids=IDS)
def test_clip_is_the_restatement_bit_for_bit(w, h, radius, motion):
    cur, prev, cam, prev_cam = clip_cases.planes(w, h)
    par, clip = clip_cases.params(w, h), clip_cases.clip(radius)
    tabs = clip_cases.tables() if motion else None
    ref = reference(w, h, radius, motion)
    kept, changed = int((ref[3] == R.KEPT).sum()), int(ref[4]["changed"].sum())
    print(f"pixels with history: {kept} of {w * h}; a channel changed by the clamp on {changed}")
    assert kept >= 5
    assert changed > kept / 10 and kept - changed > kept / 10
    got, intact = device_call(cur, prev, cam, prev_cam, par, clip, tabs)
    assert not any((a == SENTINEL).any() for a in got)
    assert_all_same(got, ref[:3], "device")
    assert intact, "an input plane was written"
    host = rt.temporal(cur, prev, cam, prev_cam, par, motion=tabs, clip=clip)
    assert_all_same(host, ref[:3], "host")
    assert_all_same(host, got, "host against device")
    # (the host call took read-only arrays: they are what they were)
    again = clip_cases.planes.__wrapped__(w, h)
    for a, b in zip(list(cur.values()) + list(prev.values()), list(again[0].values()) + list(again[1].values())):
        assert_bits(a, b)


# ---- 2: the clamp does something, and gamma reaches the kernel ------------------------------------------
@pytest.mark.parametrize("motion", [False, True], ids=["static", "motion"])
def test_clip_differs_from_the_plain_stage_and_follows_gamma(motion):
    w, h, radius = 70, 37, 2
    cur, prev, cam, prev_cam = clip_cases.planes(w, h)
    par = clip_cases.params(w, h)
    tabs = clip_cases.tables() if motion else None
    plain, _ = device_call(cur, prev, cam, prev_cam, par, None, tabs)
    ref = reference(w, h, radius, motion)
    differ = (u32(plain[0]) != u32(ref[0])).any(axis=2)
    print("pixels where the plain stage differs from the clamped one:", int(differ.sum()))
    assert differ.sum() > (ref[3] == R.KEPT).sum() / 10 and (differ <= ref[4]["changed"]).all()
    assert_all_same(plain[1:], ref[1:3], "the plain stage's", names=("variance", "history"))
    for gamma in (0.0, 0.5, 2.5):
        clip = clip_cases.clip(radius, gamma=gamma)
        want = R.accumulate(cur, prev, cam, prev_cam, par, clip, *(tabs or (None, None)))
        got, intact = device_call(cur, prev, cam, prev_cam, par, clip, tabs)
        assert_all_same(got, want[:3], f"gamma {gamma}")
        assert intact


# ---- 3: without history the call is the plain stage's copy ------------------------------------------------
@pytest.mark.parametrize("w,h", clip_cases.SIZES)
def test_clip_without_prev_is_the_copy(w, h):
    cur, _, cam, _ = clip_cases.planes(w, h)
    par, clip = clip_cases.params(w, h), clip_cases.clip(3)
    plain, _ = device_call(cur, None, cam, None, par, None)
    for tabs in (None, clip_cases.tables()):
        got, intact = device_call(cur, None, cam, None, par, clip, tabs)
        assert_all_same(got, plain, "device")
        assert_all_same(got, (cur["beauty"], cur["variance"], np.ones((h, w), dtype=F)), "the current frame")
        assert intact
        assert_all_same(rt.temporal(cur, None, cam, None, par, motion=tabs, clip=clip), plain, "host")


# ---- 4: a refused record writes nothing --------------------------------------------------------------------
def test_a_refused_record_leaves_the_outputs_untouched():
    w, h = 70, 37
    cur, prev, cam, prev_cam = clip_cases.planes(w, h)
    bad = clip_cases.clip(1)
    bad.radius = 4
    out = {}
    with pytest.raises(rt.RtError) as e:
        device_call(cur, prev, cam, prev_cam, clip_cases.params(w, h), bad, sink=out)
    assert e.value.status == -1 and "clip.radius" in str(e.value)
    import torch
    torch.cuda.synchronize()
    assert len(out) == 3 and all(bool((a == SENTINEL).all()) for a in out.values())
