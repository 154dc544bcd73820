#!/usr/bin/env python3
"""Times the à-trous denoiser (rt_denoise_device) on config 3's scene and camera
(huge scene seed 1234, 1280x720, reference camera): the beauty at 8 spp, the guides (albedo,
normal, depth) at 8 samples, the default sigmas, levels = 5. In one process, after a warm-up, the
median of `--reps` stream-event timings of

    each level alone (rt_denoise_level_device over that level's true input C_l), tiled and direct
    the whole call, with the library's choice of kernel per level and with RT_DENOISE_DIRECT
    a lone beauty frame at 8 spp, and rt_render_aov_device at 8 samples

interleaved rep by rep. A level's timing spans `--batch` back-to-back launches of it and is
divided by their number (one launch is too short for an event pair); the other calls are timed one
at a time. Each level's time is set against the bytes it must move: one read of each plane that is
on and one write of the output, 52 B per pixel with every guide, over 6.3 TB/s, the HBM rate a
streaming kernel achieves on an MI355X (8 TB/s peak). Needs a GPU; prints the table (kept as
profiles/denoise/time_c3.txt).

    python scripts/denoise_time.py [--reps 15] [--warmup 3] [--batch 20] > profiles/denoise/time_c3.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LEVELS = 5
TILED_MAX_STEP = 4  # rt_denoise_level_device runs the tiled kernel up to this step (its LDS image fits)
HBM_ACHIEVABLE = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=20)
    args = ap.parse_args()
    assert args.reps >= 10, "the median of at least 10 timings"
    import torch

    import bench
    import raytracinginoneweekend_amd as rt
    from raytracinginoneweekend_amd import _abi as abi

    assert torch.cuda.is_available(), "denoise_time.py needs a GPU"
    torch.cuda.set_device(0)
    scene_name, W, H, _, depth = bench.CONFIGS["c3"]
    assert scene_name == "huge"
    spp = 8
    scene = rt.huge_scene_arrays(1234)
    cam = rt.Camera.default(W, H)
    p = rt.make_params(W, H, spp, depth, 1234)
    ds = rt.DeviceScene(scene, device=0)
    stream = torch.cuda.current_stream().cuda_stream

    def plane(ch):
        return torch.zeros((H, W, ch) if ch > 1 else (H, W), dtype=torch.float32, device="cuda:0")

    t = {n: plane(ch) for n, ch in abi.DENOISE_PLANES.items()}
    guides = {n: t[n].data_ptr() for n in ("albedo", "normal", "depth")}
    ds.render(cam, p, t["beauty"].data_ptr(), stream)
    ds.render_aov(cam, p, guides, spp, stream)
    ptrs = {n: a.data_ptr() for n, a in t.items()}
    par = {d: rt.denoise_params(W, H, levels=LEVELS, direct=d) for d in (False, True)}
    # C_l, the input of level l: the result of the run's first l levels
    level_in = [t["beauty"]]
    for l in range(1, LEVELS):
        c = plane(3)
        rt.denoise_device(dict(ptrs, out=c.data_ptr()), rt.denoise_params(W, H, levels=l), stream)
        level_in.append(c)
    torch.cuda.synchronize()

    def level_run(l, direct):
        rec = rt.render.denoise_buffers(dict(guides, beauty=level_in[l].data_ptr(), out=t["out"].data_ptr()))

        def fn():
            for _ in range(args.batch):
                rt.render.check(rt.lib().rt_denoise_level_device(C.byref(par[direct]), C.byref(rec), l,
                                                                 C.c_void_p(stream)))
        return fn

    runs, per = {}, {}
    for l in range(LEVELS):
        for direct in (False, True):
            if not direct and (1 << l) > TILED_MAX_STEP:
                continue
            name = f"level {l} {'direct' if direct else 'tiled'}"
            runs[name], per[name] = level_run(l, direct), args.batch
    runs["whole call"] = lambda: rt.denoise_device(ptrs, par[False], stream)
    runs["whole call, direct"] = lambda: rt.denoise_device(ptrs, par[True], stream)
    runs[f"lone beauty frame {spp} spp"] = lambda: ds.render(cam, p, t["beauty"].data_ptr(), stream)
    runs[f"aov samples={spp}"] = lambda: ds.render_aov(cam, p, guides, spp, stream)
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
                times[name].append(e0.elapsed_time(e1) / per.get(name, 1))
    ds.close()
    level_bytes = W * H * 52
    print(f"config 3's scene and camera: huge scene seed 1234, {W}x{H}, reference camera; beauty {spp} spp, guides "
          f"{spp} samples, default sigmas, levels {LEVELS}; {args.reps} stream-event timings each after {args.warmup} "
          f"warm-up rounds, interleaved, ms; a level's timing is of {args.batch} launches, divided by {args.batch}")
    print(f"timed render kernels sha256 {bench.kernel_sha256()}")
    print(f"bytes a level must move: {level_bytes / 1e6:.1f} MB (52 B per pixel); TB/s and the share of "
          f"{HBM_ACHIEVABLE / 1e12:.1f} TB/s are of the median")
    print(f"{'call':<26}{'median':>9}{'min':>9}{'max':>9}{'TB/s':>8}{'share':>8}")
    med = {}
    for name, ts in times.items():
        med[name] = m = statistics.median(ts)
        line = f"{name:<26}{m:9.4f}{min(ts):9.4f}{max(ts):9.4f}"
        if name.startswith("level"):
            rate = level_bytes / (m * 1e-3)
            line += f"{rate / 1e12:8.2f}{rate / HBM_ACHIEVABLE:8.2f}"
        print(line)
    for l in range(LEVELS):
        a, b = med.get(f"level {l} tiled"), med[f"level {l} direct"]
        if a is not None:
            print(f"level {l}: tiled / direct = {a / b:.3f}")
    frame = med[f"lone beauty frame {spp} spp"]
    print(f"whole call / lone beauty frame at {spp} spp: {med['whole call'] / frame:.3f} "
          f"(direct: {med['whole call, direct'] / frame:.3f})")


if __name__ == "__main__":
    main()
