#!/usr/bin/env python3
"""Times the first-hit feature buffers (rt_render_aov_device) on config 3's scene
and camera (huge scene seed 1234, 1280x720, spp 128, reference camera) beside a lone beauty frame,
all in one process: after a warm-up, the median of `--reps` stream-event timings of

    rt_render_aov_device, samples = 8, all planes
    rt_render_aov_device, samples = 128 (= spp), all planes
    DeviceScene.render (a lone beauty frame: each one ends before the next is enqueued)

the three interleaved rep by rep. Needs a GPU; prints the table (kept as profiles/aov/time_c3.txt).

    python scripts/aov_time.py [--reps 15] [--warmup 3] > profiles/aov/time_c3.txt
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert args.reps >= 10, "the median of at least 10 timings"
    import numpy as np
    import torch

    import bench
    import raytracinginoneweekend_amd as rt
    from raytracinginoneweekend_amd import _abi as abi

    assert torch.cuda.is_available(), "aov_time.py needs a GPU"
    torch.cuda.set_device(0)
    scene_name, W, H, spp, depth = bench.CONFIGS["c3"]
    assert scene_name == "huge"
    scene = rt.huge_scene_arrays(1234)
    cam = rt.Camera.default(W, H)
    p = rt.make_params(W, H, spp, depth, 1234)
    ds = rt.DeviceScene(scene, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    planes = {n: torch.empty((H, W, ch) if ch > 1 else (H, W), dtype=torch.float32 if dt is np.float32 else torch.int32,
                             device="cuda:0") for n, (ch, dt, _) in abi.AOV_PLANES.items()}
    ptrs = {n: t.data_ptr() for n, t in planes.items()}
    rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")
    runs = {
        "aov samples=8": lambda: ds.render_aov(cam, p, ptrs, 8, stream),
        f"aov samples={spp}": lambda: ds.render_aov(cam, p, ptrs, spp, stream),
        "lone beauty frame": lambda: ds.render(cam, p, rgb.data_ptr(), stream),
    }
    times = {k: [] for k in runs}
    for rep in range(args.warmup + args.reps):
        for name, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()  # nothing else in flight: every timing is of one call alone
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    u = ds.usage()
    ds.close()
    print(f"config 3: huge scene seed 1234, {W}x{H}, spp {spp}, depth {depth}, reference camera; "
          f"{args.reps} stream-event timings each after {args.warmup} warm-up rounds, interleaved, ms")
    print(f"timed render kernels sha256 {bench.kernel_sha256()}")
    print(f"beauty: {u['sky_tiles']} sky tiles of {W * H // 64}")
    print(f"{'call':<22}{'median':>9}{'min':>9}{'max':>9}")
    for name, t in times.items():
        print(f"{name:<22}{statistics.median(t):9.3f}{min(t):9.3f}{max(t):9.3f}")
    a, b = statistics.median(times[f"aov samples={spp}"]), statistics.median(times["lone beauty frame"])
    print(f"aov at samples = spp / lone beauty frame: {a / b:.3f}")


if __name__ == "__main__":
    main()
