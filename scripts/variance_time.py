#!/usr/bin/env python3
"""Times the variance render (rt_render_var_device) beside the plain render
(rt_render_device) on config 3's scene and camera (huge scene seed 1234, 1280x720, reference
camera, depth 64) at 8 spp and at 128 spp, in one process. The figure is the frame period of a
stream of frames: `--frames` frames enqueued back to back on one stream (frames in flight), timed
by a stream-event pair around the block and divided by their number. Blocks of the two calls
alternate, `--reps` blocks each after `--warmup` warm-up rounds; the median, minimum and maximum
are printed. The gap is the price of tracing the proven-sky tiles in the main launch (no sky kernel)
plus the moments in the accumulation. Needs a GPU; prints the table (kept as
profiles/variance/render_time_c3.txt).

    python scripts/variance_time.py [--reps 10] [--warmup 2] [--frames 20] > profiles/variance/render_time_c3.txt
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=20)
    args = ap.parse_args()
    assert args.reps >= 10, "the median of at least 10 timings"
    import torch

    import bench
    import raytracinginoneweekend_amd as rt

    assert torch.cuda.is_available(), "variance_time.py needs a GPU"
    torch.cuda.set_device(0)
    scene_name, W, H, _, depth = bench.CONFIGS["c3"]
    assert scene_name == "huge"
    scene = rt.huge_scene_arrays(1234)
    cam = rt.Camera.default(W, H)
    stream = torch.cuda.current_stream().cuda_stream
    rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")
    var = torch.empty((H, W), dtype=torch.float32, device="cuda:0")
    print(f"config 3's scene and camera: huge scene seed 1234, {W}x{H}, depth {depth}, reference camera; frame period "
          f"of {args.frames} frames enqueued back to back, ms per frame; {args.reps} blocks each after {args.warmup} "
          f"warm-up rounds, the two calls' blocks alternating")
    print(f"timed render kernels sha256 {bench.kernel_sha256()}")
    print(f"{'call':<30}{'median':>9}{'min':>9}{'max':>9}")
    for spp in (8, 128):
        p = rt.make_params(W, H, spp, depth, 1234)
        # a scene per sample count: each keeps the workspaces its frames were cut into
        ds = rt.DeviceScene(scene, device=0)
        runs = {
            f"rt_render_device {spp} spp": lambda: ds.render(cam, p, rgb.data_ptr(), stream),
            f"rt_render_var_device {spp} spp": lambda: ds.render_var(cam, p, rgb.data_ptr(), var.data_ptr(), stream),
        }
        times, usage = {k: [] for k in runs}, {}
        for rep in range(args.warmup + args.reps):
            for name, fn in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()  # nothing else in flight when a block starts
                e0.record()
                for _ in range(args.frames):
                    fn()
                e1.record()
                e1.synchronize()
                usage[name] = ds.usage()
                if rep >= args.warmup:
                    times[name].append(e0.elapsed_time(e1) / args.frames)
        ds.close()
        med = {}
        for name, t in times.items():
            med[name] = statistics.median(t)
            print(f"{name:<30}{med[name]:9.4f}{min(t):9.4f}{max(t):9.4f}")
        a, b = med[f"rt_render_var_device {spp} spp"], med[f"rt_render_device {spp} spp"]
        u = usage[f"rt_render_device {spp} spp"]
        print(f"{spp} spp: variance render / plain render = {a / b:.3f} (+{a - b:.4f} ms per frame); the plain "
              f"render's sky kernel takes {u['sky_tiles']} of {W * H // 64} tiles, passes of {u['pass_samples']} samples")


if __name__ == "__main__":
    main()
