#!/usr/bin/env python3
"""Times the guided upsample kernel (rt_upsample_device) and the upscaled preview session
(rt_preview_create_upscaled) on config 3's scene.

The kernel: 640x360 -> 1280x720 over planes rendered from the scene (rt_render_var_device and
rt_render_aov_device at both sizes, one corrected camera), the median of `--reps` stream-event
timings, each around `--calls` back-to-back launches, without the variance pair (what the session
launches) and with it, interleaved rep by rep; beside each time the bytes the contract moves (the
output-size guides read once, the outputs written once, the low-resolution planes counted once) over
that time, as a share of the 6.29 TB/s a float4 copy reaches on this GPU (scripts/temporal_time.py).

The sessions, each on a scene of its own (so that rt_scene_order_counts shows what each one asked of
its scene), default flags, max_depth of config 3, interleaved in one run as scripts/preview_time.py
does it (blocks of `--frames` frames enqueued back to back on one stream and one synchronise, each
block run once untimed just before it is timed, `--reps` times after `--warmup` rounds; the frame
period is the host clock around a block over its frames, the enqueue share the host's time until the
last call returned):

    a   1280x720 at 8 spp, not upscaled (the path before this stage existed)
    b   1280x720 at 2 spp, not upscaled
    c0  640x360 at 8 spp shown at 1280x720, guide_samples 0 (every sample)
    c1  the same with guide_samples 1

each with the camera at rest (the first camera every frame) and on the orbit (`--step` degrees per
frame: every frame's dealing orders are computed on the host). Needs a GPU; prints
the table (kept as profiles/upscale/time_c3.txt).

    python scripts/upscale_time.py [--reps 11] [--warmup 2] [--frames 20] [--calls 50] > profiles/upscale/time_c3.txt
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_COPY_TBS = 6.29  # measured float4 copy rate of an MI355X (scripts/temporal_time.py)
HI_BYTES, LO_BYTES, OUT_BYTES = 24, 32, 12  # per pixel: see rt_upsample_buffers (the variance pair: + 4 and + 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--step", type=float, default=1.5)
    args = ap.parse_args()
    assert args.reps >= 10, "the median of at least 10 timings"
    import numpy as np
    import torch

    import bench
    import raytracinginoneweekend_amd as rt
    from raytracinginoneweekend_amd import _abi as abi
    from temporal_time import orbit

    assert torch.cuda.is_available(), "upscale_time.py needs a GPU"
    torch.cuda.set_device(0)
    scene_name, W, H, _, depth = bench.CONFIGS["c3"]
    assert scene_name == "huge"
    LW, LH = W // 2, H // 2
    scene = rt.huge_scene_arrays(1234)
    st = torch.cuda.Stream()
    stream = st.cuda_stream
    props = torch.cuda.get_device_properties(0)
    print(f"device {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs); "
          f"timed render kernels sha256 {bench.kernel_sha256()}; upsample kernels sha256 "
          f"{bench.kernel_sha256(('_ZN2rt15upsample_guidedILb0EEEvNS_9KUpsampleE', '_ZN2rt15upsample_guidedILb1EEEvNS_9KUpsampleE'))}")

    # ---- the kernel alone -------------------------------------------------------------------------------
    def plane(w, h, n):
        ch, dt = abi.UPSAMPLE_PLANES[n]
        return torch.zeros((h, w, ch) if ch > 1 else (h, w), dtype=torch.int32 if dt is np.uint32 else torch.float32,
                           device="cuda:0")

    t = {n: plane(LW, LH, n) if n.startswith("lo_") else plane(W, H, n) for n in abi.UPSAMPLE_PLANES}
    ds = rt.DeviceScene(scene, device=0)
    cam = orbit(rt, W, H, 0.0, rt.CORRECTED)
    p_lo, p_hi = rt.make_params(LW, LH, 8, depth, 1), rt.make_params(W, H, 8, depth, 1)
    ds.render_var(cam, p_lo, t["lo_color"].data_ptr(), t["lo_variance"].data_ptr(), stream)
    ds.render_aov(cam, p_lo, dict(normal=t["lo_normal"].data_ptr(), depth=t["lo_depth"].data_ptr(),
                                  sphere_id=t["lo_sphere_id"].data_ptr()), 0, stream)
    ds.render_aov(cam, p_hi, {n: t[n].data_ptr() for n in ("normal", "depth", "alpha", "sphere_id")}, 0, stream)
    st.synchronize()
    ds.close()
    par = rt.upsample_params(W, H, LW, LH)
    every = {n: a.data_ptr() for n, a in t.items()}
    colour_only = {n: a for n, a in every.items() if n not in ("lo_variance", "out_variance")}
    runs = {"colour only (the session's launch)": (colour_only, W * H * (HI_BYTES + OUT_BYTES) + LW * LH * LO_BYTES),
            "colour and variance": (every, W * H * (HI_BYTES + OUT_BYTES + 4) + LW * LH * (LO_BYTES + 4))}
    times = {k: [] for k in runs}
    with torch.cuda.stream(st):
        for rep in range(args.warmup + args.reps):
            for name, (ptrs, _) in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(st)
                for _ in range(args.calls):
                    rt.upsample_device(ptrs, par, stream)
                e1.record(st)
                e1.synchronize()
                if rep >= args.warmup:
                    times[name].append(e0.elapsed_time(e1) * 1e3 / args.calls)
    print(f"the kernel alone: config 3's scene, {LW}x{LH} -> {W}x{H}, corrected camera, 8 spp, default tolerances; {args.reps} "
          f"stream-event timings each after {args.warmup} warm-up rounds, interleaved, each around {args.calls} back-to-back "
          "launches; microseconds per launch (launch gaps included)")
    print("bytes: the contract's (the output-size guides read once, the outputs written once, the low-resolution planes "
          f"counted once); share: of the {HBM_COPY_TBS} TB/s a float4 copy reaches (the planes stay in the Infinity Cache "
          "between launches: the share says how far the kernel is from being bound by HBM)")
    print(f"{'launch':<38}{'median':>9}{'min':>9}{'max':>9}{'MB':>9}{'TB/s':>8}{'share':>8}")
    for name, ts in times.items():
        med, nbytes = statistics.median(ts), runs[name][1]
        rate = nbytes / (med * 1e-6) / 1e12
        print(f"{name:<38}{med:9.2f}{min(ts):9.2f}{max(ts):9.2f}{nbytes / 1e6:9.2f}{rate:8.2f}{100 * rate / HBM_COPY_TBS:7.1f}%")

    # ---- the sessions ---------------------------------------------------------------------------------------
    n = args.frames
    cams = [orbit(rt, W, H, args.step * i, rt.CORRECTED) for i in range(n)]
    still = [cams[0]] * n
    rgb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
    specs = {"a  1280x720 8 spp": (W, H, 8, None), "b  1280x720 2 spp": (W, H, 2, None),
             "c0 640x360 8 spp upscaled, guides 8": (LW, LH, 8, 0), "c1 640x360 8 spp upscaled, guides 1": (LW, LH, 8, 1)}
    scenes, sessions = {}, {}
    for name, (w, h, spp, guide) in specs.items():
        scenes[name] = rt.DeviceScene(scene, device=0)
        p = rt.preview_params(w, h, spp, max_depth=depth)
        sessions[name] = scenes[name].preview(p, None if guide is None else rt.preview_upscale(p, W, H, guide_samples=guide))

    def block(pv, cams):
        def go():
            pv.reset()
            for i in range(n):
                pv.frame(cams[i], 1 + i, rgb.data_ptr(), rgb8.data_ptr(), stream)
        return go

    blocks = {}
    for where, cs in (("rest ", still), ("orbit", cams)):
        for name, pv in sessions.items():
            blocks[f"{where} {name}"] = (block(pv, cs), name)
    periods, enqueue, orders = {k: [] for k in blocks}, {k: [] for k in blocks}, {}
    for rep in range(args.warmup + args.reps):
        for key, (fn, name) in blocks.items():
            fn()  # not timed: every block starts from the cache of dealing orders its own cameras leave
            torch.cuda.synchronize()
            before = scenes[name].order_counts()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            st.synchronize()
            t2 = time.perf_counter()
            after = scenes[name].order_counts()
            orders[key] = {k: after[k] - before[k] for k in after}
            if rep >= args.warmup:
                periods[key].append((t2 - t0) * 1e3 / n)
                enqueue[key].append((t1 - t0) * 1e3 / n)
    print(f"the sessions: config 3's scene, output {W}x{H}, default flags (DEMODULATE), max_depth {depth}, corrected camera at "
          f"rest and on an orbit {args.step} degrees per frame; blocks of {n} frames enqueued back to back and one synchronise, "
          f"{args.reps} blocks each after {args.warmup} warm-up rounds, alternating; milliseconds per frame by the host clock "
          "(period: enqueue to the end of the last frame; enqueue: the host's share until the last call returned); orders: "
          "rt_scene_order_counts over one timed block (dealing orders computed on the host / on the device / found cached)")
    print("session planes: " + ", ".join(f"{name.split()[0]} {pv.usage()} bytes" for name, pv in sessions.items()))
    print(f"{'block':<44}{'period':>9}{'min':>9}{'max':>9}{'enqueue':>10}{'min':>9}{'max':>9}   orders host/device/cached")
    for key in blocks:
        ps, es, o = periods[key], enqueue[key], orders[key]
        print(f"{key:<44}{statistics.median(ps):9.3f}{min(ps):9.3f}{max(ps):9.3f}{statistics.median(es):10.3f}{min(es):9.3f}"
              f"{max(es):9.3f}   {o['host_orders']}/{o['device_orders']}/{o['hits']}")
    for where in ("rest ", "orbit"):
        med = {name.split()[0]: statistics.median(periods[f"{where} {name}"]) for name in sessions}
        print(f"{where.strip()}: c0 / a = {med['c0'] / med['a']:.3f}, c0 / b = {med['c0'] / med['b']:.3f}, "
              f"c1 / a = {med['c1'] / med['a']:.3f}, c1 / b = {med['c1'] / med['b']:.3f} (medians of the periods)")
    for pv in sessions.values():
        pv.close()
    for s in scenes.values():
        s.close()


if __name__ == "__main__":
    main()
