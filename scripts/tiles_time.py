#!/usr/bin/env python3
"""Times the dealing order computed on the device (rt_options.tile_classes = 1)
against the host's (tile_classes = 0, the default) with scripts/preview_time.py's protocol: config
3's scene at 1280x720, 8 spp, the corrected default camera on an orbit (`--step` degrees per frame)
or at rest; a block is `--frames` frames enqueued back to back on one stream and one synchronise,
its frame period the host clock around it over the frames, its enqueue time the host's share until
the last call returned. Blocks alternate host mode / device mode, `--reps` times after `--warmup`
rounds, each block run once untimed just before it is timed (so every block starts from the cache of
dealing orders its own cameras leave: on the orbit every frame then has a camera the scene no longer
holds); median and min-max. Both through a preview session (flags 0) and through the five device
calls a caller would make (scripts/preview_time.py's chain).

Then the cost of one new camera in each mode: the host duration of one rt_render_var_device call
with a camera the scene has not seen, on an idle device and with `--inflight` frames of a resting
camera enqueued just before it (does the event wait stall behind the frames in flight?). And the
device's work for one order by stream events around single rt_tile_order_device calls (the two
kernels and the counts' copy; each call ends in a synchronise, so a batch cannot be bracketed).
`--kernels-only` runs just those calls, for a kernel trace. Needs a GPU; prints the table (kept as
profiles/tiles/time_c3.txt).

    python scripts/tiles_time.py [--reps 11] [--warmup 2] [--frames 20] > profiles/tiles/time_c3.txt
"""
import argparse
import ctypes as C
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
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--step", type=float, default=1.5)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    import torch

    import bench
    import raytracinginoneweekend_amd as rt
    from raytracinginoneweekend_amd import render
    from temporal_time import orbit

    assert torch.cuda.is_available(), "tiles_time.py needs a GPU"
    torch.cuda.set_device(0)
    scene_name, W, H, _, depth = bench.CONFIGS["c3"]
    assert scene_name == "huge"
    spp, n = args.spp, args.frames
    arrays = rt.huge_scene_arrays(1234)
    scenes = {"host": rt.DeviceScene(arrays, device=0, options=rt.options(tile_classes=0)),
              "device": rt.DeviceScene(arrays, device=0, options=rt.options(tile_classes=1))}
    st = torch.cuda.Stream()
    stream = st.cuda_stream
    cams = [orbit(rt, W, H, args.step * i, rt.CORRECTED) for i in range(n)]
    still = [cams[0]] * n

    def plane(ch, dtype=torch.float32):
        return torch.zeros((H, W, ch) if ch > 1 else (H, W), dtype=dtype, device="cuda:0")

    def one_order_us(ds, cam, p, perm):
        nb, nl, ns = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        t0 = time.perf_counter()
        render.check(rt.lib().rt_tile_order_device(ds.handle, C.byref(cam.c), C.byref(p), C.c_void_p(perm.data_ptr()),
                                                   perm.numel(), C.byref(nb), C.byref(nl), C.byref(ns), C.c_void_p(stream)))
        t1 = time.perf_counter()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, (t1 - t0) * 1e6, (nb.value, nl.value, ns.value)

    rp0 = rt.make_params(W, H, spp, depth, 1)
    perm = torch.zeros(W * H // 64, dtype=torch.int32, device="cuda:0")
    if args.kernels_only:
        for i in range(args.calls):
            one_order_us(scenes["host"], orbit(rt, W, H, 90.0 + 0.5 * i, rt.CORRECTED), rp0, perm)
        return

    rgb, rgb8 = plane(3), plane(3, torch.uint8)
    par = rt.preview_params(W, H, spp, flags=0, max_depth=depth)
    sessions = {m: ds.preview(par) for m, ds in scenes.items()}

    def session_block(pv, cams):
        def go():
            pv.reset()
            for i in range(n):
                pv.frame(cams[i], 1 + i, rgb.data_ptr(), rgb8.data_ptr(), stream)
        return go

    # the chain by hand (scripts/preview_time.py): the planes a caller keeps, ping-ponged
    beauty, variance, albedo, alpha = plane(3), plane(1), plane(3), plane(1)
    g = [dict(normal=plane(3), depth=plane(1), sphere_id=plane(1, torch.int32)) for _ in range(2)]
    hist = [dict(color=plane(3), variance=plane(1), history=plane(1)) for _ in range(2)]
    out, scratch, var_scratch = plane(3), plane(3), plane(2)

    def chain_block(ds, cams):
        def go():
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
                rt.temporal_device({k: a.data_ptr() for k, a in ptrs.items()}, par.temporal, cams[i], cams[i - 1] if i else None,
                                   stream)
                rt.denoise_var_device(dict(beauty=hist[c]["color"].data_ptr(), albedo=albedo.data_ptr(),
                                           normal=g[c]["normal"].data_ptr(), depth=g[c]["depth"].data_ptr(), out=out.data_ptr(),
                                           scratch=scratch.data_ptr()), par.denoise,
                                      render.denoise_var_buffers(dict(variance=hist[c]["variance"].data_ptr(),
                                                                      var_scratch=var_scratch.data_ptr()), par.var_floor), stream)
                rt.epilogue_rgb8_device(out.data_ptr(), rgb8.data_ptr(), W * H, stream)
        return go

    blocks = {}
    for what, cs in (("orbit", cams), ("at rest", still)):
        for m in scenes:
            blocks[f"{what}: session, {m} mode"] = session_block(sessions[m], cs)
        for m in scenes:
            blocks[f"{what}: five calls, {m} mode"] = chain_block(scenes[m], cs)
    periods = {k: [] for k in blocks}
    enqueue = {k: [] for k in blocks}
    for rep in range(args.warmup + args.reps):
        for name, fn in blocks.items():
            fn()
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
    print(f"config 3's scene, {W}x{H}, corrected camera on an orbit {args.step} degrees per frame or at rest, {spp} spp, "
          f"max_depth {depth}; blocks of {n} frames enqueued back to back and one synchronise, {args.reps} blocks each after "
          f"{args.warmup} warm-up rounds, alternating; milliseconds per frame by the host clock (period: enqueue to the end of "
          "the last frame; enqueue: the host's share until the last call returned)")
    print(f"device {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs); "
          f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')}; timed render kernels sha256 {bench.kernel_sha256()}")
    print(f"{'block':<34}{'period':>9}{'min':>9}{'max':>9}{'enqueue':>10}{'min':>9}{'max':>9}")
    for name in blocks:
        ps, es = periods[name], enqueue[name]
        print(f"{name:<34}{statistics.median(ps):9.3f}{min(ps):9.3f}{max(ps):9.3f}{statistics.median(es):10.3f}{min(es):9.3f}{max(es):9.3f}")
    for what in ("orbit", "at rest"):
        for how in ("session", "five calls"):
            a = statistics.median(periods[f"{what}: {how}, device mode"])
            b = statistics.median(periods[f"{what}: {how}, host mode"])
            print(f"{what}, {how}: device / host = {a / b:.4f} of the period (medians)")
    print("order counts:", {m: ds.order_counts() for m, ds in scenes.items()})

    # one new camera: the host duration of its first render call
    fresh = iter(range(10 ** 6))
    new_cost = {}
    for busy in (0, args.inflight):
        for m, ds in scenes.items():
            ts = []
            for rep in range(args.warmup + args.calls):
                cam = orbit(rt, W, H, 120.0 + 0.37 * next(fresh), rt.CORRECTED)
                torch.cuda.synchronize()
                for _ in range(busy):
                    ds.render_var(cams[0], rp0, beauty.data_ptr(), variance.data_ptr(), stream)
                t0 = time.perf_counter()
                ds.render_var(cam, rp0, beauty.data_ptr(), variance.data_ptr(), stream)
                t1 = time.perf_counter()
                if rep >= args.warmup:
                    ts.append((t1 - t0) * 1e3)
            torch.cuda.synchronize()
            new_cost[(busy, m)] = ts
    cached = []
    for rep in range(args.warmup + args.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scenes["host"].render_var(cams[0], rp0, beauty.data_ptr(), variance.data_ptr(), stream)
        cached.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    print(f"one rt_render_var_device call with a camera the scene has not seen, host milliseconds of the call, {args.calls} cameras "
          "each (the scene holds 8 orders already)")
    print(f"{'call':<52}{'median':>9}{'min':>9}{'max':>9}")
    for (busy, m), ts in new_cost.items():
        name = f"{m} mode, " + ("idle device" if not busy else f"{busy} frames of a resting camera in flight")
        print(f"{name:<52}{statistics.median(ts):9.3f}{min(ts):9.3f}{max(ts):9.3f}")
    ts = cached[args.warmup:]
    print(f"{'a cached camera, idle device':<52}{statistics.median(ts):9.3f}{min(ts):9.3f}{max(ts):9.3f}")

    # the device's work for one order
    ev, host = [], []
    for rep in range(args.warmup + args.calls):
        torch.cuda.synchronize()
        e, h, counts = one_order_us(scenes["host"], orbit(rt, W, H, 200.0 + 0.41 * rep, rt.CORRECTED), rp0, perm)
        if rep >= args.warmup:
            ev.append(e)
            host.append(h)
    print(f"one rt_tile_order_device call ({counts[0]} blocks; classify_tiles_kernel, order_blocks_kernel and the counts' copy), "
          f"{args.calls} cameras, microseconds")
    print(f"{'':<34}{'median':>9}{'min':>9}{'max':>9}")
    print(f"{'stream events around the call':<34}{statistics.median(ev):9.1f}{min(ev):9.1f}{max(ev):9.1f}")
    print(f"{'host clock around the call':<34}{statistics.median(host):9.1f}{min(host):9.1f}{max(host):9.1f}")
    for pv in sessions.values():
        pv.close()
    for ds in scenes.values():
        ds.close()


if __name__ == "__main__":
    main()
