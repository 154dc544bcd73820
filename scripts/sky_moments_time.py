#!/usr/bin/env python3
"""Times rt_options.sky_moments (sky_moments_kernel) on config 3 (1280x720, the huge
scene, the reference camera): every workload that carries per-pixel moments on a scene with the
option at 0 and on one with it at 1, in one process, the blocks alternating `--reps` times after
`--warmup` rounds; milliseconds by the host clock, median and min-max. A difference counts only if it
exceeds the min-max spread of the option-0 block beside it.

  lone frame      rt_render_device / rt_render_var_device, one call and a wait, at 8 and 128 spp
  frame stream    `--frames` such calls back to back and one wait; per frame
  progressive     a 128-sample session in windows of 128, 32 and 8, queued, each window resolved
  adaptive        noise_tau 0.1 and 0.25 (min_samples 8) in windows of 32, and with a first window of 8
                  followed by windows of 32; queued
  preview         a session at 8 spp, `--frames` frames at rest and on the 1.5 degree orbit

`--parent-lib PATH`: the lone variance frame (option 0) is also timed from another build of the
library (the parent commit's), in a child process per repetition, alternating with this build's.
`--noground-lib PATH`: nothing else is timed; the plain frame (rt_render_device, lone and in a stream of
`--frames`, at 128 and 8 spp) from this build and from a build with -DRT_NO_GROUND
(scripts/build_variant.sh), in child processes alternating `--reps` times: whether the ground kernel's
stages are why the plain frame is slower than the variance frame with the option.
`--kernels N`: nothing is timed; N variance frames with the option and N plain frames at 128 spp, for
`rocprofv3 --kernel-trace --stats -- python scripts/sky_moments_time.py --kernels 20` (sky_moments_kernel
against sky_kernel on the same frame).
Needs a GPU; prints the table (kept as profiles/sky_moments/time_c3.txt).
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def setup():
    import torch

    import bench
    import raytracinginoneweekend_amd as rt
    assert torch.cuda.is_available(), "sky_moments_time.py needs a GPU"
    torch.cuda.set_device(0)
    _, W, H, spp, depth = bench.CONFIGS["c3"]
    return torch, bench, rt, W, H, spp, depth


def child_lone(reps):
    """This process's library, option 0: `reps` lone variance frames at 128 and at 8 spp; two lines of ms."""
    torch, _, rt, W, H, spp, depth = setup()
    ds = rt.DeviceScene(rt.huge_scene_arrays(1234), device=0)
    st = torch.cuda.Stream()
    rgb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    var = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
    cam = rt.Camera.default(W, H)
    for n in (spp, 8):
        p, out = rt.make_params(W, H, n, depth, 1234), []
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ds.render_var(cam, p, rgb.data_ptr(), var.data_ptr(), st.cuda_stream)
            st.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        print(" ".join(f"{t:.4f}" for t in out[1:]))  # (the first frame allocates)
    ds.close()


def child_plain(reps, n_stream):
    """This process's library: `reps` plain frames, lone at 128 and 8 spp, then per frame in a stream of
    `n_stream`, likewise; four lines of ms."""
    torch, _, rt, W, H, spp, depth = setup()
    ds = rt.DeviceScene(rt.huge_scene_arrays(1234), device=0)
    st = torch.cuda.Stream()
    rgb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    cam = rt.Camera.default(W, H)
    for count in (1, n_stream):
        for n in (spp, 8):
            p, out = rt.make_params(W, H, n, depth, 1234), []
            for _ in range(reps + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(count):
                    ds.render(cam, p, rgb.data_ptr(), st.cuda_stream)
                st.synchronize()
                out.append((time.perf_counter() - t0) * 1e3 / count)
            print(" ".join(f"{t:.4f}" for t in out[2:]))  # (the first frames allocate)
    ds.close()


def noground(args):
    rows = ("lone frame, 128 spp", "lone frame, 8 spp", f"stream of {args.frames}, 128 spp", f"stream of {args.frames}, 8 spp")
    times = {w: [[] for _ in rows] for w in ("this build", "RT_NO_GROUND build")}
    for _ in range(args.reps):
        for which, lib in (("RT_NO_GROUND build", args.noground_lib), ("this build", None)):
            env = dict(os.environ)
            env.pop("RT_LIB_PATH", None)
            if lib:
                env["RT_LIB_PATH"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-plain", "5", "--frames", str(args.frames)],
                               env=env, check=True, capture_output=True, text=True, timeout=300)
            for into, line in zip(times[which], r.stdout.strip().splitlines()[-4:]):
                into.extend(float(x) for x in line.split())
    print(f"rt_render_device on config 3 (the plain frame), child processes alternating {args.reps} times, 5 timings each; "
          "ms per frame by the host clock")
    print(f"{'block':<64}{'median':>9}{'min':>9}{'max':>9}")
    for i, row in enumerate(rows):
        for which in times:
            ts = times[which][i]
            print(f"{row + ', ' + which:<64}{statistics.median(ts):9.3f}{min(ts):9.3f}{max(ts):9.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--noground-lib", default=None)
    ap.add_argument("--child-lone", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--child-plain", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child_lone:
        child_lone(args.child_lone)
        return
    if args.child_plain:
        child_plain(args.child_plain, args.frames)
        return
    if args.noground_lib:
        noground(args)
        return
    torch, bench, rt, W, H, spp, depth = setup()
    from temporal_time import orbit
    records = rt.huge_scene_arrays(1234)
    scenes = {o: rt.DeviceScene(records, device=0, options=rt.options(sky_moments=o)) for o in (0, 1)}
    st = torch.cuda.Stream()
    stream = st.cuda_stream
    rgb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    var = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
    rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
    samples = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    noisy = torch.zeros((1,), dtype=torch.int32, device="cuda:0")
    cam = rt.Camera.default(W, H)
    params = {n: rt.make_params(W, H, n, depth, 1234) for n in (8, spp)}

    if args.kernels:
        for _ in range(args.kernels):
            scenes[1].render_var(cam, params[spp], rgb.data_ptr(), var.data_ptr(), stream)
            st.synchronize()
            scenes[1].render(cam, params[spp], rgb.data_ptr(), stream)
            st.synchronize()
        print("usage after the last variance frame's scene:", scenes[1].usage())
        return

    def frames(ds, n, count, plain):
        def go():
            for _ in range(count):
                if plain:
                    ds.render(cam, params[n], rgb.data_ptr(), stream)
                else:
                    ds.render_var(cam, params[n], rgb.data_ptr(), var.data_ptr(), stream)
        return go, count

    pouts = rt.progressive_outputs(rgb.data_ptr(), var.data_ptr(), rgb8.data_ptr(), noisy.data_ptr(), 0.1)
    aouts = rt.adaptive_outputs(rgb.data_ptr(), var.data_ptr(), rgb8.data_ptr(), samples.data_ptr(), noisy.data_ptr())
    keep = []  # the sessions, closed at the end

    def progressive(ds, window):
        pg = ds.progressive(cam, params[spp])
        keep.append(pg)

        def go():
            pg.reset()
            for _ in range(0, spp, window):
                pg.step(window, outputs=pouts, stream=stream)
        return go, 1

    def adaptive(ds, tau, schedule):
        ad = ds.adaptive(cam, params[spp], rt.adaptive_params(tau, 0, 8))
        keep.append(ad)

        def go():
            ad.reset()
            for n in schedule:
                ad.step(n, outputs=aouts, stream=stream)
        return go, 1

    n = args.frames
    orbit_cams = [orbit(rt, W, H, 1.5 * i, rt.REFERENCE) for i in range(n)]
    pp = rt.preview_params(W, H, 8, flags=0, max_depth=depth)

    def preview(ds, cams):
        pv = ds.preview(pp)
        keep.append(pv)

        def go():
            pv.reset()
            for i in range(n):
                pv.frame(cams[i], 1 + i, rgb.data_ptr(), rgb8.data_ptr(), stream)
        return go, n

    W32, W8 = (32,) * (spp // 32), (8,) + (32,) * ((spp - 8) // 32) + ((spp - 8) % 32,)
    blocks = {}
    for s in (8, spp):
        blocks[f"lone frame, {s} spp: rt_render_device"] = frames(scenes[0], s, 1, True)
        for o in (0, 1):
            blocks[f"lone frame, {s} spp: rt_render_var_device, sky_moments {o}"] = frames(scenes[o], s, 1, False)
    for s in (8, spp):
        blocks[f"frame stream, {s} spp: rt_render_device"] = frames(scenes[0], s, n, True)
        for o in (0, 1):
            blocks[f"frame stream, {s} spp: rt_render_var_device, sky_moments {o}"] = frames(scenes[o], s, n, False)
    for w in (128, 32, 8):
        for o in (0, 1):
            blocks[f"progressive, windows of {w}, sky_moments {o}"] = progressive(scenes[o], w)
    for tau in (0.1, 0.25):
        for name, sched in (("windows of 32", W32), ("8 then windows of 32", W8)):
            for o in (0, 1):
                blocks[f"adaptive tau {tau}, {name}, sky_moments {o}"] = adaptive(scenes[o], tau, sched)
    for name, cams in (("at rest", [orbit_cams[0]] * n), ("on the orbit", orbit_cams)):
        for o in (0, 1):
            blocks[f"preview 8 spp {name}, sky_moments {o}"] = preview(scenes[o], cams)

    times = {k: [] for k in blocks}
    parent = {"this": ([], []), "parent": ([], [])}
    for rep in range(args.warmup + args.reps):
        for name, (fn, per) in blocks.items():
            if name.startswith("preview"):
                fn()  # not timed: the block starts from the cache of dealing orders its own cameras leave
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            st.synchronize()
            if rep >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3 / per)
        if args.parent_lib and rep >= args.warmup and rep % 2 == 0:
            for which, lib in (("parent", args.parent_lib), ("this", None)):
                env = dict(os.environ)
                env.pop("RT_LIB_PATH", None)
                if lib:
                    env["RT_LIB_PATH"] = os.path.abspath(lib)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-lone", "3"], env=env, check=True,
                                   capture_output=True, text=True, timeout=300)
                for into, line in zip(parent[which], r.stdout.strip().splitlines()[-2:]):
                    into.extend(float(x) for x in line.split())

    props = torch.cuda.get_device_properties(0)
    print(f"config 3: the huge scene, {W}x{H}, max_depth {depth}, reference camera; every block {args.reps} times after "
          f"{args.warmup} warm-up rounds, alternating in one process; milliseconds by the host clock (enqueue to the end of "
          f"the last work), per frame; frame streams and preview blocks hold {n} frames")
    print(f"device {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs); "
          f"timed render kernels sha256 {bench.kernel_sha256()}")
    for o in (0, 1):
        print(f"scene with sky_moments {o} after the blocks: {scenes[o].usage()}")
    print(f"{'block':<64}{'median':>9}{'min':>9}{'max':>9}")
    for name, ts in times.items():
        if ts:
            print(f"{name:<64}{statistics.median(ts):9.3f}{min(ts):9.3f}{max(ts):9.3f}")
    for which in ("this", "parent"):
        for ts, s in zip(parent[which], (spp, 8)):
            if ts:
                name = f"child process, {which} build: lone variance frame, {s} spp, sky_moments 0"
                print(f"{name:<64}{statistics.median(ts):9.3f}{min(ts):9.3f}{max(ts):9.3f}")
    print("adaptive schedules (deterministic): blocks active after each step, samples rendered / (n_pixels N)")
    for tau in (0.1, 0.25):
        for name, sched in (("windows of 32", W32), ("8 then windows of 32", W8)):
            ad = scenes[1].adaptive(cam, params[spp], rt.adaptive_params(tau, 0, 8))
            active = []
            for m in sched:
                ad.step(m, outputs=aouts, stream=stream)
                active.append(ad.info()["active_blocks"])
            info = ad.info()
            print(f"  tau {tau}, {name}: {active}  {info['samples_rendered'] / (W * H * spp):.4f}")
            ad.close()
    for s in keep:
        s.close()
    for ds in scenes.values():
        ds.close()


if __name__ == "__main__":
    main()
