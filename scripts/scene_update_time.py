#!/usr/bin/env python3
"""Times rt_scene_update against the only way to move a sphere without it: on the
huge scene (seed 1234) at 1280x720, three spheres (2, 3, 4) moved by 0.05 per step,

    update      rt_scene_update, then the first render
    recreate    rt_scene_destroy + rt_scene_create_ex, then the first render (whose workspaces grow)

Wall time on the host clock around work that ends in a device synchronise, `--reps` steps each,
alternating. The update's own parts (host derivation, device wait, upload and swap) are what the
library prints under RT_DIAG_VERBOSE; the script runs a second scene with that bit and shows the lines.
Needs a GPU; prints the table (kept as profiles/motion/update_time.txt).
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    args = ap.parse_args()
    import numpy as np
    import torch

    import raytracinginoneweekend_amd as rt

    assert torch.cuda.is_available(), "scene_update_time.py needs a GPU"
    W, H, spp = 1280, 720, 4
    base, mats = rt.huge_scene_arrays(1234)

    def records(step):
        s = base.copy()
        s["center"][2:5, 2] += np.float32(0.05) * np.float32(step)
        return s, mats

    cam, p = rt.Camera.default(W, H, rt.CORRECTED), rt.make_params(W, H, spp, 8, 1)
    rgb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")

    def render(ds):
        ds.render(cam, p, rgb.data_ptr())
        torch.cuda.synchronize()

    live = rt.DeviceScene(records(0))
    other = rt.DeviceScene(records(0))
    render(live), render(other)
    rows = {"update": [], "update + first render": [], "recreate": [], "recreate + first render": []}
    for step in range(1, args.reps + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        live.update(records(step))
        t1 = time.perf_counter()
        render(live)
        t2 = time.perf_counter()
        other.close()
        other = rt.DeviceScene(records(step))
        t3 = time.perf_counter()
        render(other)
        t4 = time.perf_counter()
        if step > 2:
            for k, v in zip(rows, (t1 - t0, t2 - t0, t3 - t2, t4 - t2)):
                rows[k].append(v * 1e3)
    render(live)
    t5 = time.perf_counter()
    render(live)
    repeated = (time.perf_counter() - t5) * 1e3
    props = torch.cuda.get_device_properties(0)
    print(f"huge scene (seed 1234, {len(base)} spheres), spheres 2, 3, 4 moved by 0.05 per step, {W}x{H}, {spp} spp, "
          f"max_depth 8; host wall time in ms ending in a device synchronise, {args.reps} steps after 2 warm-up steps, "
          f"the two ways alternating; device {props.name}")
    print(f"{'':<26}{'median':>9}{'min':>9}{'max':>9}")
    for k, v in rows.items():
        print(f"{k:<26}{statistics.median(v):9.3f}{min(v):9.3f}{max(v):9.3f}")
    print(f"a repeated render of the same scene and camera: {repeated:.3f} ms")
    sys.stdout.flush()
    print("the update's parts (RT_DIAG_VERBOSE, on an idle device):")
    sys.stdout.flush()
    v = rt.DeviceScene(records(0), options=rt.options(verbose=True))
    for step in (1, 2, 3):
        v.update(records(step))
    sys.stderr.flush()


if __name__ == "__main__":
    main()
