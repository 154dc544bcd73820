#!/usr/bin/env python3
"""Times a progressive session (rt_progressive_*) against the one-shot variance
render on config 3 (1280x720, 128 spp, the huge scene): the whole frame by rt_render_var_device, and
by a session in windows of 128, 32 and 8 samples, each window resolved into rgb + variance + rgb8 +
the noise count. A session is timed twice: with its steps enqueued back to back and one synchronise
(`queued`), and with a host wait after every step (`waited`, the interactive case, where nothing
overlaps the end of a window). Blocks alternate in one process, `--reps` times after `--warmup`
rounds; milliseconds per frame by the host clock, median and min-max.

`--parent-lib PATH`: the one-shot is also timed from another build of the library (the parent
commit's), in a child process per repetition, alternating with this build's.
`--c5`: config 5 (1024 spp) instead: the time to the first resolved image with windows of 8, against
the whole frame.
`--resolve-calls N`: also N resolve-only steps (step(0) with outputs) between two stream events: the
resolve kernel with its launch gap; for its time alone profile that run with
`rocprofv3 --kernel-trace --stats -- python scripts/progressive_time.py --reps 0 --resolve-calls 200`.
Needs a GPU; prints the table (kept as profiles/progressive/time_c3.txt).
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def one_shot_ms(reps, spp):
    """This process's library: `reps` one-shot variance frames, each synchronised; [ms]."""
    import torch

    import bench
    import raytracinginoneweekend_amd as rt
    _, W, H, _, depth = bench.CONFIGS["c3"]
    ds = rt.DeviceScene(rt.huge_scene_arrays(1234), device=0)
    st = torch.cuda.Stream()
    rgb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    var = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
    p, cam = rt.make_params(W, H, spp, depth, 1234), rt.Camera.default(W, H)
    out = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ds.render_var(cam, p, rgb.data_ptr(), var.data_ptr(), st.cuda_stream)
        st.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    ds.close()
    return out[1:]  # (the first frame allocates)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--c5", action="store_true")
    ap.add_argument("--resolve-calls", type=int, default=0)
    ap.add_argument("--child-one-shot", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child_one_shot:
        print(" ".join(f"{t:.4f}" for t in one_shot_ms(args.child_one_shot, 128)))
        return
    import torch

    import bench
    import raytracinginoneweekend_amd as rt

    assert torch.cuda.is_available(), "progressive_time.py needs a GPU"
    torch.cuda.set_device(0)
    _, W, H, spp, depth = bench.CONFIGS["c5" if args.c5 else "c3"]
    ds = rt.DeviceScene(rt.huge_scene_arrays(1234), device=0)
    st = torch.cuda.Stream()
    stream = st.cuda_stream
    rgb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    var = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
    rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
    noisy = torch.zeros((1,), dtype=torch.int32, device="cuda:0")
    p, cam = rt.make_params(W, H, spp, depth, 1234), rt.Camera.default(W, H)
    outs = rt.progressive_outputs(rgb.data_ptr(), var.data_ptr(), rgb8.data_ptr(), noisy.data_ptr(), 0.1)
    pg = ds.progressive(cam, p)
    first_image = {}

    def one_shot():
        ds.render_var(cam, p, rgb.data_ptr(), var.data_ptr(), stream)

    def session(window, waited, first=None):
        def go():
            pg.reset()
            t0 = time.perf_counter()
            for i in range(0, spp, window):
                pg.step(window, outputs=outs, stream=stream)
                if waited or (first is not None and i == 0):
                    st.synchronize()
                    if i == 0 and first is not None:
                        first.append((time.perf_counter() - t0) * 1e3)
        return go

    blocks = {"one-shot rt_render_var_device": one_shot}
    if args.c5:
        first_image["session, windows of 8"] = []
        blocks["session, windows of 8, first image waited for"] = session(8, False, first_image["session, windows of 8"])
    else:
        for w in (128, 32, 8):
            blocks[f"session, windows of {w}, queued"] = session(w, False)
            blocks[f"session, windows of {w}, waited"] = session(w, True)
    times = {k: [] for k in blocks}
    parent, own_child = [], []
    for rep in range(args.warmup + args.reps):
        for name, fn in blocks.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            st.synchronize()
            if rep >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
        if args.parent_lib and rep >= args.warmup and not args.c5:
            for lib, into in ((args.parent_lib, parent), (None, own_child)):
                env = dict(os.environ)
                if lib:
                    env["RT_LIB_PATH"] = os.path.abspath(lib)
                else:
                    env.pop("RT_LIB_PATH", None)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-one-shot", "3"], env=env, check=True,
                                   capture_output=True, text=True, timeout=300)
                into.extend(float(x) for x in r.stdout.split())
    props = torch.cuda.get_device_properties(0)
    print(f"config {'5' if args.c5 else '3'}: the huge scene, {W}x{H}, {spp} spp, max_depth {depth}, reference camera; every block "
          f"{args.reps} times after {args.warmup} warm-up rounds, alternating; milliseconds per frame by the host clock "
          "(enqueue to the end of the frame's last work)")
    print(f"device {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs); "
          f"timed render kernels sha256 {bench.kernel_sha256()}")
    print(f"session planes: {pg.info()['device_bytes']} bytes; scene after the blocks: {ds.usage()}")
    print(f"{'block':<50}{'median':>9}{'min':>9}{'max':>9}")

    def row(name, ts):
        if ts:
            print(f"{name:<50}{statistics.median(ts):9.3f}{min(ts):9.3f}{max(ts):9.3f}")

    for name, ts in times.items():
        row(name, ts)
    for name, ts in first_image.items():
        row(name + ": enqueue to the first image", ts[args.warmup:])
    row("child process, this build: one-shot", own_child)
    row("child process, --parent-lib: one-shot", parent)

    if args.resolve_calls:
        pg.reset()
        pg.step(spp, stream=stream)
        ts = []
        with torch.cuda.stream(st):
            for _ in range(max(args.reps, 1) + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(st)
                for _ in range(args.resolve_calls):
                    pg.step(0, outputs=outs, stream=stream)
                e1.record(st)
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3 / args.resolve_calls)
        px = W * H
        moved = px * (24 + 12 + 4 + 3)
        print(f"resolve-only steps (the count's 4-byte memset and progressive_resolve, launch gaps included), {args.resolve_calls} "
              f"back to back between stream events; microseconds per step; {moved / 1e6:.2f} MB read and written once per launch "
              "(24 B read, 19 B written per pixel; the planes stay in the Infinity Cache between launches)")
        med = statistics.median(ts[1:])
        print(f"{'rgb + variance + rgb8 + count':<50}{med:9.2f}{min(ts[1:]):9.2f}{max(ts[1:]):9.2f}   {moved / (med * 1e-6) / 1e12:.2f} TB/s")
    pg.close()
    ds.close()


if __name__ == "__main__":
    main()
