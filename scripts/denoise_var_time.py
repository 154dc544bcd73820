#!/usr/bin/env python3
"""Times the variance-guided à-trous filter (rt_denoise_var_device) beside the
plain one (rt_denoise_device, §4.9) on config 3's scene and camera (huge scene seed 1234, 1280x720,
reference camera): the beauty and its variance at 8 spp from rt_render_var_device, the guides
(albedo, normal, depth) at 8 samples, each call's default sigmas, levels = 5. In one process, after
a warm-up, the median of `--reps` stream-event timings of

    rt_denoise_var_device, with and without variance_out
    rt_denoise_device, with the library's choice of kernel per level and with RT_DENOISE_DIRECT

interleaved rep by rep, one call per timing. The variance-guided call is five direct-load launches
(no LDS-tiled form), so RT_DENOISE_DIRECT is the like-for-like row. Needs a GPU; prints the table
(kept as profiles/variance/denoise_time_c3.txt).

    python scripts/denoise_var_time.py [--reps 15] [--warmup 3] > profiles/variance/denoise_time_c3.txt
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LEVELS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert args.reps >= 10, "the median of at least 10 timings"
    import torch

    import bench
    import raytracinginoneweekend_amd as rt
    from raytracinginoneweekend_amd import _abi as abi

    assert torch.cuda.is_available(), "denoise_var_time.py needs a GPU"
    torch.cuda.set_device(0)
    scene_name, W, H, _, depth = bench.CONFIGS["c3"]
    assert scene_name == "huge"
    spp = 8
    cam = rt.Camera.default(W, H)
    p = rt.make_params(W, H, spp, depth, 1234)
    ds = rt.DeviceScene(rt.huge_scene_arrays(1234), device=0)
    stream = torch.cuda.current_stream().cuda_stream

    def plane(ch):
        return torch.zeros((H, W, ch) if ch > 1 else (H, W), dtype=torch.float32, device="cuda:0")

    t = {n: plane(ch) for n, ch in {**abi.DENOISE_PLANES, **abi.DENOISE_VAR_PLANES}.items()}
    ds.render_var(cam, p, t["beauty"].data_ptr(), t["variance"].data_ptr(), stream)
    ds.render_aov(cam, p, {n: t[n].data_ptr() for n in ("albedo", "normal", "depth")}, spp, stream)
    torch.cuda.synchronize()
    ds.close()
    ptrs = {n: t[n].data_ptr() for n in abi.DENOISE_PLANES}
    vp, vv = rt.denoise_var_params(W, H, levels=LEVELS)
    vrec = {out: rt.render.denoise_var_buffers({"variance": t["variance"].data_ptr(),
                                                "variance_out": t["variance_out"].data_ptr() if out else 0,
                                                "var_scratch": t["var_scratch"].data_ptr()}, vv.var_floor)
            for out in (False, True)}
    par = {d: rt.denoise_params(W, H, levels=LEVELS, direct=d) for d in (False, True)}
    runs = {
        "rt_denoise_var_device": lambda: rt.denoise_var_device(ptrs, vp, vrec[False], stream),
        "  with variance_out": lambda: rt.denoise_var_device(ptrs, vp, vrec[True], stream),
        "rt_denoise_device": lambda: rt.denoise_device(ptrs, par[False], stream),
        "  RT_DENOISE_DIRECT": lambda: rt.denoise_device(ptrs, par[True], stream),
    }
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
                times[name].append(e0.elapsed_time(e1))
    print(f"config 3's scene and camera: huge scene seed 1234, {W}x{H}, reference camera; beauty and variance {spp} spp, "
          f"guides {spp} samples, each call's default sigmas, levels {LEVELS}; {args.reps} stream-event timings each "
          f"after {args.warmup} warm-up rounds, interleaved, ms per call")
    print(f"timed render kernels sha256 {bench.kernel_sha256()}")
    print(f"{'call':<26}{'median':>9}{'min':>9}{'max':>9}")
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        print(f"{name:<26}{med[name]:9.4f}{min(ts):9.4f}{max(ts):9.4f}")
    print(f"variance-guided / plain: {med['rt_denoise_var_device'] / med['rt_denoise_device']:.3f} "
          f"(against RT_DENOISE_DIRECT: {med['rt_denoise_var_device'] / med['  RT_DENOISE_DIRECT']:.3f})")


if __name__ == "__main__":
    main()
