#!/usr/bin/env python3
"""Times the temporal accumulation kernel (rt_temporal_device) on config 3's scene
at 1280x720: two consecutive frames of an orbit of the default camera around its look-at point
(one degree apart, corrected camera, 4 spp, guides of the same samples) from rt_render_var_device and
rt_render_aov_device, then, in one process after a warm-up, the median of `--reps` stream-event
timings, each around `--calls` back-to-back launches (one launch is tens of microseconds: an event
pair around a single one would time the events), of

    rt_temporal_device with history       over one set of planes (92 MB: it stays in the 256 MB
                                          Infinity Cache between launches)
    rt_temporal_device with history       rotating over `--sets` copies of the planes (more than the
                                          cache holds: every launch reads HBM)
    rt_temporal_device without history    the copy, over one set

interleaved rep by rep. Beside each time: the bytes the contract moves (the current planes read
once, the outputs written once, the previous planes counted once) over that time, and that rate as a
share of the 6.29 TB/s a float4 copy reaches on this GPU. Needs a GPU; prints the table (kept as
profiles/temporal/time_c3.txt).

    python scripts/temporal_time.py [--reps 15] [--warmup 3] [--calls 50] [--sets 4] > profiles/temporal/time_c3.txt
"""
import argparse
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_COPY_TBS = 6.29  # measured float4 copy rate of an MI355X (8.0 TB/s is the specification's peak)
CUR_BYTES, PREV_BYTES, OUT_BYTES = 40, 40, 20  # per pixel: see rt_temporal_buffers


def orbit(rt, w, h, degrees, mode):
    """The default camera turned by `degrees` around the vertical axis through its look-at point."""
    import numpy as np
    pos, look = np.array([-4.0, 3.2, 5.0]), np.array([0.0, 1.0, 0.0])
    a = math.radians(degrees)
    d = pos - look
    p = look + np.array([d[0] * math.cos(a) + d[2] * math.sin(a), d[1], -d[0] * math.sin(a) + d[2] * math.cos(a)])
    focus = float(np.float32(np.linalg.norm((p - look).astype(np.float32))))
    return rt.Camera(tuple(p), tuple(look), (0, 1, 0), w / h, 42.0, 0.0625, focus, mode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--sets", type=int, default=4)
    args = ap.parse_args()
    assert args.reps >= 10, "the median of at least 10 timings"
    import numpy as np
    import torch

    import bench
    import raytracinginoneweekend_amd as rt
    from raytracinginoneweekend_amd import _abi as abi

    assert torch.cuda.is_available(), "temporal_time.py needs a GPU"
    torch.cuda.set_device(0)
    scene_name, W, H, _, depth = bench.CONFIGS["c3"]
    assert scene_name == "huge"
    spp = 4
    ds = rt.DeviceScene(rt.huge_scene_arrays(1234), device=0)
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
    sets = [t] + [{n: a.clone() for n, a in t.items()} for _ in range(args.sets - 1)]
    with_prev = [{n: a.data_ptr() for n, a in s.items()} for s in sets]
    without = {n: a for n, a in with_prev[0].items() if not n.startswith("prev_")}
    rt.temporal_device(with_prev[0], par, cams[1], cams[0], stream)
    torch.cuda.synchronize()
    kept = float((t["out_history"] > 1.0).float().mean())

    def run(ptrs):
        def go():
            for c in range(args.calls):
                rt.temporal_device(ptrs[c % len(ptrs)], par, cams[1], cams[0], stream)
        return go

    px = W * H
    runs = {
        "history, one set": (run(with_prev[:1]), px * (CUR_BYTES + PREV_BYTES + OUT_BYTES)),
        f"history, {args.sets} sets": (run(with_prev), px * (CUR_BYTES + PREV_BYTES + OUT_BYTES)),
        "no history (copy)": (run([without]), px * (16 + OUT_BYTES)),
    }
    times = {k: [] for k in runs}
    for rep in range(args.warmup + args.reps):
        for name, (fn, _) in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()  # nothing else in flight
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3 / args.calls)
    print(f"config 3's scene, {W}x{H}, corrected camera, two frames of an orbit one degree apart at {spp} spp, default "
          f"parameters: {100 * kept:.1f}% of the pixels keep a history. {args.reps} stream-event timings each after "
          f"{args.warmup} warm-up rounds, interleaved, each around {args.calls} back-to-back launches; microseconds per "
          f"launch (launch gaps included)")
    props = torch.cuda.get_device_properties(0)
    print(f"device {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs); "
          f"timed render kernels sha256 {bench.kernel_sha256()}")
    print("bytes: the contract's (current planes read once, outputs written once, previous planes counted once; the copy "
          f"reads beauty and variance only); share: of the {HBM_COPY_TBS} TB/s a float4 copy reaches (HBM; one set of "
          "planes stays in the Infinity Cache, so its share says how far the kernel is from being bound by HBM, not that "
          "HBM delivered it)")
    print(f"{'launch':<22}{'median':>9}{'min':>9}{'max':>9}{'MB':>9}{'TB/s':>8}{'share':>8}")
    for name, ts in times.items():
        med, nbytes = statistics.median(ts), runs[name][1]
        rate = nbytes / (med * 1e-6) / 1e12
        print(f"{name:<22}{med:9.2f}{min(ts):9.2f}{max(ts):9.2f}{nbytes / 1e6:9.2f}{rate:8.2f}{100 * rate / HBM_COPY_TBS:7.1f}%")


if __name__ == "__main__":
    main()
