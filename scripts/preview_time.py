#!/usr/bin/env python3
"""Times a preview session's frame (rt_preview_frame_device) against the same chain
issued as the five public device calls from Python, on config 3's scene at 1280x720, 8 spp, on an
orbit of the default camera (corrected, `--step` degrees per frame). A scene keeps the dealing orders
of its 8 most recent cameras, so on the orbit both render calls of every frame compute the frame's
dealing order on the host: what a moving camera costs today, and the same on both
sides of the comparison. The blocks with the camera at rest leave that out.

A block is `--frames` frames enqueued back to back on one stream and one synchronise; its frame
period is the host clock around it over the frames (the enqueue's host time is part of what is
compared). Blocks alternate: session (flags 0: the chain's bits), chain, session with DEMODULATE |
FEEDBACK, then session and chain with the camera at rest (the first camera every frame, seeds as
before), `--reps` times after `--warmup` rounds, each block run once untimed just before it is
timed; median and min-max of the blocks' periods. Then the
session's two kernels alone by stream events around `--calls` back-to-back launches, as
scripts/temporal_time.py times its kernel. Needs a GPU; prints the table (kept as
profiles/preview/time_c3.txt).

    python scripts/preview_time.py [--reps 11] [--warmup 2] [--frames 20] [--calls 50] > profiles/preview/time_c3.txt
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--step", type=float, default=1.5)
    ap.add_argument("--spp", type=int, default=8)
    args = ap.parse_args()
    import torch

    import bench
    import raytracinginoneweekend_amd as rt
    from raytracinginoneweekend_amd import _abi as abi
    from raytracinginoneweekend_amd import render
    from temporal_time import orbit

    assert torch.cuda.is_available(), "preview_time.py needs a GPU"
    torch.cuda.set_device(0)
    scene_name, W, H, _, depth = bench.CONFIGS["c3"]
    assert scene_name == "huge"
    spp, n = args.spp, args.frames
    ds = rt.DeviceScene(rt.huge_scene_arrays(1234), device=0)
    st = torch.cuda.Stream()
    stream = st.cuda_stream
    cams = [orbit(rt, W, H, args.step * i, rt.CORRECTED) for i in range(n)]
    still = [cams[0]] * n

    def plane(ch, dtype=torch.float32):
        return torch.zeros((H, W, ch) if ch > 1 else (H, W), dtype=dtype, device="cuda:0")

    rgb, rgb8 = plane(3), plane(3, torch.uint8)
    par = {name: rt.preview_params(W, H, spp, flags=flags, max_depth=depth)
           for name, flags in (("session, flags 0", 0), ("session, DEMODULATE | FEEDBACK", abi.RT_PREVIEW_DEMODULATE | abi.RT_PREVIEW_FEEDBACK))}
    sessions = {name: ds.preview(p) for name, p in par.items()}

    def session_block(pv, cams=cams):
        def go():
            pv.reset()
            for i in range(n):
                pv.frame(cams[i], 1 + i, rgb.data_ptr(), rgb8.data_ptr(), stream)
        return go

    # the chain by hand: the planes a caller keeps, ping-ponged
    p0 = par["session, flags 0"]
    beauty, variance, albedo, alpha = plane(3), plane(1), plane(3), plane(1)
    g = [dict(normal=plane(3), depth=plane(1), sphere_id=plane(1, torch.int32)) for _ in range(2)]
    hist = [dict(color=plane(3), variance=plane(1), history=plane(1)) for _ in range(2)]
    out, scratch, var_scratch = plane(3), plane(3), plane(2)

    def chain_block(cams=cams):
        for i in range(n):
            c, o = i % 2, 1 - i % 2
            rp = rt.make_params(W, H, spp, depth, 1 + i)
            ds.render_var(cams[i], rp, beauty.data_ptr(), variance.data_ptr(), stream)
            ds.render_aov(cams[i], rp, dict(albedo=albedo.data_ptr(), alpha=alpha.data_ptr(),
                                            **{k: a.data_ptr() for k, a in g[c].items()}), 0, stream)
            ptrs = dict(beauty=beauty, variance=variance, alpha=alpha, **g[c], out_color=hist[c]["color"],
                        out_variance=hist[c]["variance"], out_history=hist[c]["history"])
            if i:
                ptrs.update({"prev_" + k: a for k, a in {**hist[o], **g[o]}.items()})
            rt.temporal_device({k: a.data_ptr() for k, a in ptrs.items()}, p0.temporal, cams[i], cams[i - 1] if i else None, stream)
            rt.denoise_var_device(dict(beauty=hist[c]["color"].data_ptr(), albedo=albedo.data_ptr(),
                                       normal=g[c]["normal"].data_ptr(), depth=g[c]["depth"].data_ptr(), out=out.data_ptr(),
                                       scratch=scratch.data_ptr()), p0.denoise,
                                  render.denoise_var_buffers(dict(variance=hist[c]["variance"].data_ptr(),
                                                                  var_scratch=var_scratch.data_ptr()), p0.var_floor), stream)
            rt.epilogue_rgb8_device(out.data_ptr(), rgb8.data_ptr(), W * H, stream)

    blocks = {"session, flags 0": session_block(sessions["session, flags 0"]), "five device calls from Python": chain_block,
              "session, DEMODULATE | FEEDBACK": session_block(sessions["session, DEMODULATE | FEEDBACK"]),
              # the camera at rest: the render calls find the dealing order in the scene's cache
              "static: session, flags 0": session_block(sessions["session, flags 0"], still),
              "static: five device calls": lambda: chain_block(still)}
    periods = {k: [] for k in blocks}
    enqueue = {k: [] for k in blocks}
    for rep in range(args.warmup + args.reps):
        for name, fn in blocks.items():
            fn()  # not timed: every block starts from the cache of dealing orders its own cameras leave
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            st.synchronize()
            t2 = time.perf_counter()
            if rep >= args.warmup:
                periods[name].append((t2 - t0) * 1e3 / n)
                enqueue[name].append((t1 - t0) * 1e3 / n)
    props = torch.cuda.get_device_properties(0)
    print(f"config 3's scene, {W}x{H}, corrected camera on an orbit {args.step} degrees per frame, {spp} spp, max_depth {depth}; "
          f"blocks of {n} frames enqueued back to back and one synchronise, {args.reps} blocks each after {args.warmup} warm-up "
          "rounds, alternating; milliseconds per frame by the host clock (period: enqueue to the end of the last frame; "
          "enqueue: the host's share until the last call returned)")
    print(f"device {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs); "
          f"timed render kernels sha256 {bench.kernel_sha256()}")
    print(f"session planes: {sessions['session, flags 0'].usage()} bytes (flags 0), "
          f"{sessions['session, DEMODULATE | FEEDBACK'].usage()} bytes (DEMODULATE | FEEDBACK)")
    print(f"{'block':<34}{'period':>9}{'min':>9}{'max':>9}{'enqueue':>10}{'min':>9}{'max':>9}")
    for name in blocks:
        ps, es = periods[name], enqueue[name]
        print(f"{name:<34}{statistics.median(ps):9.3f}{min(ps):9.3f}{max(ps):9.3f}{statistics.median(es):10.3f}{min(es):9.3f}{max(es):9.3f}")
    a, b = statistics.median(periods["session, flags 0"]), statistics.median(periods["five device calls from Python"])
    print(f"session / chain: {a / b:.4f} of the chain's period (medians)")
    a, b = statistics.median(periods["static: session, flags 0"]), statistics.median(periods["static: five device calls"])
    print(f"static camera, session / chain: {a / b:.4f} of the chain's period (medians)")

    # the two kernels alone
    illum, ivar = plane(3), plane(1)
    kernels = {
        "preview_split": lambda: rt.preview_split_device(W, H, beauty.data_ptr(), variance.data_ptr(), albedo.data_ptr(),
                                                         illum.data_ptr(), ivar.data_ptr(), stream),
        "preview_merge x albedo, f32 + rgb8": lambda: rt.preview_merge_device(W, H, out.data_ptr(), albedo.data_ptr(),
                                                                               rgb.data_ptr(), rgb8.data_ptr(), stream),
        "preview_merge x albedo, rgb8 only": lambda: rt.preview_merge_device(W, H, out.data_ptr(), albedo.data_ptr(), None,
                                                                              rgb8.data_ptr(), stream),
        "preview_merge copy, f32 + rgb8": lambda: rt.preview_merge_device(W, H, out.data_ptr(), None, rgb.data_ptr(),
                                                                           rgb8.data_ptr(), stream),
        "rt_epilogue_rgb8_device": lambda: rt.epilogue_rgb8_device(out.data_ptr(), rgb8.data_ptr(), W * H, stream),
    }
    px = W * H
    moved = {"preview_split": px * (12 + 4 + 12 + 12 + 4), "preview_merge x albedo, f32 + rgb8": px * (12 + 12 + 12 + 3),
             "preview_merge x albedo, rgb8 only": px * (12 + 12 + 3), "preview_merge copy, f32 + rgb8": px * (12 + 12 + 3),
             "rt_epilogue_rgb8_device": px * (12 + 3)}
    times = {k: [] for k in kernels}
    with torch.cuda.stream(st):
        for rep in range(args.warmup + args.reps):
            for name, fn in kernels.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(st)
                for _ in range(args.calls):
                    fn()
                e1.record(st)
                e1.synchronize()
                if rep >= args.warmup:
                    times[name].append(e0.elapsed_time(e1) * 1e3 / args.calls)
    print(f"the kernels alone: {args.reps} stream-event timings each around {args.calls} back-to-back launches, interleaved; "
          "microseconds per launch (launch gaps included); MB: the planes read and written once (they stay in the Infinity "
          "Cache between launches)")
    print(f"{'launch':<38}{'median':>9}{'min':>9}{'max':>9}{'MB':>9}{'TB/s':>8}")
    for name, ts in times.items():
        med = statistics.median(ts)
        print(f"{name:<38}{med:9.2f}{min(ts):9.2f}{max(ts):9.2f}{moved[name] / 1e6:9.2f}{moved[name] / (med * 1e-6) / 1e12:8.2f}")
    for pv in sessions.values():
        pv.close()
    ds.close()


if __name__ == "__main__":
    main()
