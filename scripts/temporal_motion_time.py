#!/usr/bin/env python3
"""Times the temporal stage with object motion (rt_temporal_motion_device) against the
static stage on the same planes: config 3's scene at 1280x720, two frames of scripts/temporal_time.py's
orbit, the scene's sphere table and a copy of it with spheres 2, 3 and 4 moved by 0.05. In one process
after a warm-up, the median of `--reps` stream-event timings, each around `--calls` back-to-back
launches over one set of planes, of

    static          rt_temporal_device
    motion          rt_temporal_motion_device, two 16-byte table loads per surface lane
    motion, LDS     only with a library built from profiles/motion/lds_form.diff (RT_LIB_PATH), under
                    RT_TEMPORAL_MOTION_LDS=1: the workgroup stages the table in LDS

interleaved rep by rep. The LDS form would have been kept only if its slowest timing were below the
base form's fastest; it was not (profiles/motion/kernel_time.txt), and the library no longer holds it:
without that build the third row repeats the second. Needs a GPU; prints the table.

    python scripts/temporal_motion_time.py [--reps 15] [--warmup 3] [--calls 50] > profiles/motion/kernel_time.txt
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

    assert torch.cuda.is_available(), "temporal_motion_time.py needs a GPU"
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
    now = rt.sphere_table(scene)
    was = now.copy()
    was[2:5, 2] -= np.float32(0.05)
    d_now, d_was = torch.from_numpy(now).to("cuda:0"), torch.from_numpy(was).to("cuda:0")
    motion = (d_now.data_ptr(), d_was.data_ptr(), len(now))
    par = rt.temporal_params(W, H)
    ptrs = {n: a.data_ptr() for n, a in t.items()}

    def run(m, lds):
        def go():
            os.environ["RT_TEMPORAL_MOTION_LDS"] = "1" if lds else "0"
            for _ in range(args.calls):
                rt.temporal_device(ptrs, par, cams[1], cams[0], stream, motion=m)
        return go

    runs = {"static": run(None, False), "motion": run(motion, False), "motion, LDS": run(motion, True)}
    outs = {}
    for name, fn in runs.items():
        fn()
        torch.cuda.synchronize()
        outs[name] = [t[n].clone() for n in ("out_color", "out_variance", "out_history")]
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs["motion"], outs["motion, LDS"]))
    moved = int((outs["motion"][0].view(torch.int32) != outs["static"][0].view(torch.int32)).any(dim=2).sum())
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
    os.environ.pop("RT_TEMPORAL_MOTION_LDS", None)
    props = torch.cuda.get_device_properties(0)
    print(f"config 3's scene, {W}x{H}, {len(now)} spheres, corrected camera, two frames of an orbit one degree apart at "
          f"{spp} spp, default parameters; {args.reps} stream-event timings each after {args.warmup} warm-up rounds, "
          f"interleaved, each around {args.calls} back-to-back launches over one set of planes; microseconds per launch "
          "(launch gaps included)")
    print(f"device {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs)")
    print(f"the two motion forms' outputs are the same bits: {same}; pixels where the motion changes the colour: {moved}")
    print(f"{'launch':<16}{'median':>9}{'min':>9}{'max':>9}")
    for name, ts in times.items():
        print(f"{name:<16}{statistics.median(ts):9.2f}{min(ts):9.2f}{max(ts):9.2f}")
    keep = max(times["motion, LDS"]) < min(times["motion"])
    print("the LDS form's slowest timing is " + ("below" if keep else "not below") + " the base form's fastest: "
          + ("keep it" if keep else "it stays off"))


if __name__ == "__main__":
    main()
