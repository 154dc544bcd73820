#!/usr/bin/env python3
"""Times the temporal stage with the history clamp (rt_temporal_clip_device) against the
plain history launch on the same planes, by scripts/temporal_time.py's method: config 3's scene at
1280x720, two frames of its orbit one degree apart at 4 spp. In one process after a warm-up, the median
of `--reps` stream-event timings, each around `--calls` back-to-back launches over one set of planes, of

    plain            rt_temporal_device (temporal_accumulate<true, false, false>)
    clip, radius r   rt_temporal_clip_device at gamma 1, r = 1, 2, 3 (temporal_accumulate<true, false, true>)

interleaved rep by rep. The clip kernel's workgroup shape is a compile-time choice (RT_CLIP_BW: 64 x 4,
or 32 x 8 with -DRT_CLIP_BW=32, scripts/build_variant.sh); RT_LIB_PATH times another build, and the
plain row, whose kernel does not depend on the shape, ties the two runs together. Needs a GPU; prints the
table (kept, with both shapes, as profiles/clip/kernel_time.txt).

    python scripts/clip_time.py [--reps 15] [--warmup 3] [--calls 50]
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    assert args.reps >= 10, "the median of at least 10 timings"
    import numpy as np
    import torch

    import bench
    import raytracinginoneweekend_amd as rt
    from raytracinginoneweekend_amd import _abi as abi
    from temporal_time import orbit

    assert torch.cuda.is_available(), "clip_time.py needs a GPU"
    torch.cuda.set_device(0)
    _, W, H, _, depth = bench.CONFIGS["c3"]
    spp = 4
    scene = rt.huge_scene_arrays(1234)
    ds = rt.DeviceScene(scene, device=0)
    stream = torch.cuda.current_stream().cuda_stream

    def plane(n):
        ch, dt = abi.TEMPORAL_PLANES[n]
        return torch.zeros((H, W, ch) if ch > 1 else (H, W), dtype=torch.int32 if dt is np.uint32 else torch.float32,
                           device="cuda:0")

    t = {n: plane(n) for n in abi.TEMPORAL_PLANES}
    cams = [orbit(rt, W, H, a, rt.CORRECTED) for a in (0.0, 1.0)]
    for i, (cam, pre) in enumerate(zip(cams, ("prev_", ""))):
        p = rt.make_params(W, H, spp, depth, 1 + i)
        beauty, var = (t["prev_color"], t["prev_variance"]) if pre else (t["beauty"], t["variance"])
        ds.render_var(cam, p, beauty.data_ptr(), var.data_ptr(), stream)
        guides = {n: t[pre + n].data_ptr() for n in ("normal", "depth", "sphere_id")}
        if not pre:
            guides["alpha"] = t["alpha"].data_ptr()
        ds.render_aov(cam, p, guides, spp, stream)
    t["prev_history"].fill_(1.0)
    torch.cuda.synchronize()
    ds.close()
    par = rt.temporal_params(W, H)
    ptrs = {n: a.data_ptr() for n, a in t.items()}

    def run(clip):
        def go():
            for _ in range(args.calls):
                rt.temporal_device(ptrs, par, cams[1], cams[0], stream, clip=clip)
        return go

    runs = {"plain": run(None)}
    runs.update({f"clip, radius {r}": run(rt.temporal_clip(radius=r, gamma=1.0)) for r in (1, 2, 3)})
    changed = {}
    for name, fn in runs.items():
        fn()
        torch.cuda.synchronize()
        out = t["out_color"].clone().view(torch.int32)
        if name == "plain":
            plain, kept = out, int((t["out_history"] > 1).sum())
        else:
            changed[name] = int((out != plain).any(dim=2).sum())
    times = {k: [] for k in runs}
    for rep in range(args.warmup + args.reps):
        for name, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3 / args.calls)
    props = torch.cuda.get_device_properties(0)
    print(f"config 3's scene, {W}x{H}, corrected camera, two frames of an orbit one degree apart at {spp} spp, default "
          f"parameters, gamma 1; {args.reps} stream-event timings each after {args.warmup} warm-up rounds, interleaved, each "
          f"around {args.calls} back-to-back launches over one set of planes; microseconds per launch (launch gaps included)")
    print(f"device {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs); library "
          + (os.path.relpath(os.environ["RT_LIB_PATH"], REPO) if os.environ.get("RT_LIB_PATH") else "the tree build"))
    print(f"pixels with history: {kept} of {W * H}; pixels whose colour the clamp changes: "
          + ", ".join(f"{n.split(', ')[1]}: {c}" for n, c in changed.items()))
    print(f"{'launch':<18}{'median':>9}{'min':>9}{'max':>9}{'/ plain':>9}")
    base = statistics.median(times["plain"])
    for name, ts in times.items():
        print(f"{name:<18}{statistics.median(ts):9.2f}{min(ts):9.2f}{max(ts):9.2f}{statistics.median(ts) / base:9.3f}")


if __name__ == "__main__":
    main()
