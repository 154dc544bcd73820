#!/usr/bin/env python3
"""Times an adaptive session (rt_adaptive_*) against the plain progressive session on
config 3 (1280x720, 128 spp, the huge scene) in windows of 32 samples, every window resolved into
rgb + variance + rgb8 (+ the sample counts) + the noise count. The blocks alternate in one process,
`--reps` times after `--warmup` rounds; milliseconds per frame by the host clock, median and min-max:

  plain session              rt_progressive_*, steps enqueued back to back and one synchronise (queued),
                             or a host wait after every step (waited: what an adaptive step's wait
                             for the previous step's block counts amounts to)
  adaptive, nothing retires  min_samples = 128: every block active at every step, so a step is the
                             plain step + adaptive_resolve for progressive_resolve + compact_blocks +
                             the copy of four words + one event wait
  adaptive, tau t            noise_tau t in 0.1, 0.25, 0.5, max_noisy 0, min_samples 8

Per adaptive run also the share of the frame's samples it rendered and the blocks active after every
step. Then the error each result buys: the mean squared error of the linear rgb against the full
128-sample frame, for the adaptive result and for a plain session stopped after the same total number
of samples spread uniformly (rounded down to a multiple of 4).

For the two kernels' times alone profile a short run:
`rocprofv3 --kernel-trace --stats -- python scripts/adaptive_time.py --reps 2 --warmup 1 --no-mse`.
Needs a GPU; prints the table (kept as profiles/adaptive/time_c3.txt).
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WINDOW = 32
TAUS = (0.1, 0.25, 0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-mse", action="store_true")
    args = ap.parse_args()
    import torch

    import bench
    import raytracinginoneweekend_amd as rt

    assert torch.cuda.is_available(), "adaptive_time.py needs a GPU"
    torch.cuda.set_device(0)
    _, W, H, spp, depth = bench.CONFIGS["c3"]
    ds = rt.DeviceScene(rt.huge_scene_arrays(1234), device=0)
    st = torch.cuda.Stream()
    stream = st.cuda_stream
    rgb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    var = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
    rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
    samples = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    noisy = torch.zeros((1,), dtype=torch.int32, device="cuda:0")
    p, cam = rt.make_params(W, H, spp, depth, 1234), rt.Camera.default(W, H)
    pg = ds.progressive(cam, p)
    pouts = {t: rt.progressive_outputs(rgb.data_ptr(), var.data_ptr(), rgb8.data_ptr(), noisy.data_ptr(), t) for t in TAUS}
    aouts = rt.adaptive_outputs(rgb.data_ptr(), var.data_ptr(), rgb8.data_ptr(), samples.data_ptr(), noisy.data_ptr())
    sessions = {"adaptive, nothing retires (min_samples 128)": ds.adaptive(cam, p, rt.adaptive_params(0.1, 0, 128))}
    for t in TAUS:
        sessions[f"adaptive, tau {t}, max_noisy 0, min_samples 8"] = ds.adaptive(cam, p, rt.adaptive_params(t, 0, 8))

    def plain(upto=spp):
        pg.reset()
        for s in range(0, upto, WINDOW):
            pg.step(min(WINDOW, upto - s), outputs=pouts[0.1], stream=stream)

    def adaptive(name):
        ad = sessions[name]

        def go():
            ad.reset()
            for _ in range(0, spp, WINDOW):
                ad.step(WINDOW, outputs=aouts, stream=stream)
        return go

    def plain_waited():
        pg.reset()
        for _ in range(0, spp, WINDOW):
            pg.step(WINDOW, outputs=pouts[0.1], stream=stream)
            st.synchronize()

    blocks = {"plain session, windows of 32, queued": plain, "plain session, windows of 32, waited": plain_waited}
    for name in sessions:
        blocks[name] = adaptive(name)
    times = {k: [] for k in blocks}
    for rep in range(args.warmup + args.reps):
        for name, fn in blocks.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            st.synchronize()
            if rep >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)

    props = torch.cuda.get_device_properties(0)
    print(f"config 3: the huge scene, {W}x{H}, {spp} spp, max_depth {depth}, reference camera, windows of {WINDOW}; every block "
          f"{args.reps} times after {args.warmup} warm-up rounds, alternating; milliseconds per frame by the host clock "
          "(enqueue to the end of the frame's last work)")
    print(f"device {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs); "
          f"timed render kernels sha256 {bench.kernel_sha256()}")
    print(f"{'block':<52}{'median':>9}{'min':>9}{'max':>9}")
    for name, ts in times.items():
        if ts:
            print(f"{name:<52}{statistics.median(ts):9.3f}{min(ts):9.3f}{max(ts):9.3f}")
    ts_plain, ts_all = times["plain session, windows of 32, queued"], times["adaptive, nothing retires (min_samples 128)"]
    if ts_plain and ts_all:
        ts_w = times["plain session, windows of 32, waited"]
        print(f"adaptive with every block active - plain session: {statistics.median(ts_all) - statistics.median(ts_plain):+.3f} ms "
              f"against queued, {statistics.median(ts_all) - statistics.median(ts_w):+.3f} ms against waited, per frame of "
              f"{spp // WINDOW} steps (medians); the plain session's run-to-run spread in this file (max - min): "
              f"{max(ts_plain) - min(ts_plain):.3f} ms queued, {max(ts_w) - min(ts_w):.3f} ms waited")

    # the schedule of every adaptive run (deterministic), step by step, with a wait per step
    print("blocks active after each step, of", W * H // 64, "; samples rendered / (n_pixels N)")
    totals = {}
    for name, ad in sessions.items():
        ad.reset()
        active = []
        for _ in range(0, spp, WINDOW):
            ad.step(WINDOW, outputs=aouts, stream=stream)
            active.append(ad.info()["active_blocks"])
        info = ad.info()
        totals[name] = info["samples_rendered"]
        print(f"{name:<52}{active}  {info['samples_rendered'] / (W * H * spp):.4f}  (done {info['done']})")

    if not args.no_mse:
        plain()
        st.synchronize()
        full = rgb.clone()
        print("mean squared error of the linear rgb against the full 128-sample frame (a result, not a condition)")
        print(f"{'run':<52}{'adaptive':>12}{'uniform':>12}{'uniform spp':>13}")
        for name, ad in sessions.items():
            if "nothing retires" in name:
                continue
            ad.reset()
            for _ in range(0, spp, WINDOW):
                ad.step(WINDOW, outputs=aouts, stream=stream)
            st.synchronize()
            mse_a = float(((rgb.double() - full.double()) ** 2).mean())
            k = (totals[name] // (W * H)) & ~3
            plain(k)
            st.synchronize()
            mse_u = float(((rgb.double() - full.double()) ** 2).mean())
            print(f"{name:<52}{mse_a:12.4e}{mse_u:12.4e}{k:13d}")
    for ad in sessions.values():
        ad.close()
    pg.close()
    ds.close()


if __name__ == "__main__":
    main()
