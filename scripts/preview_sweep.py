#!/usr/bin/env python3
"""The sweep behind rt_preview_params_default's flags: §4.11's 16-frame orbit of the
default camera around its look-at point (`--step` degrees per frame, the huge scene at `--width` x
`--height`), every frame at 4 spp with a seed of its own against the same frame at 1024 spp, with the
corrected and with the reference camera. Rows:

    (a) raw           the 4-spp frame (rt_render_var)
    (b) filter alone  rt_denoise_var of that frame alone, its default parameters
    the session in each of {plain, DEMODULATE, FEEDBACK, DEMODULATE | FEEDBACK}, and NO_TEMPORAL with
    and without DEMODULATE (the filter alone through the session: the first repeats (b))

Per row: the mean over the frames of the mean squared error against the target, that figure over
(a)'s and over (b)'s, and a flicker figure: the mean over t = 1..15 of mean((e_t - e_{t-1})^2) with
e_t = output_t - target_t, the frame-to-frame change of the error image (the target's own motion
cancels). Needs a GPU; prints the table (kept as profiles/preview/sweep.txt).

    python scripts/preview_sweep.py [--width 320] [--height 180] [--step 1.5] > profiles/preview/sweep.txt
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raytracinginoneweekend_amd as rt  # noqa: E402
from raytracinginoneweekend_amd import _abi as abi  # noqa: E402
from temporal_sweep import FRAMES, SPP, TARGET_SPP, mse, orbit  # noqa: E402

D, FB, NT = abi.RT_PREVIEW_DEMODULATE, abi.RT_PREVIEW_FEEDBACK, abi.RT_PREVIEW_NO_TEMPORAL
MODES = (("session, plain", 0), ("session, DEMODULATE", D), ("session, FEEDBACK", FB), ("session, DEMODULATE | FEEDBACK", D | FB),
         ("session, NO_TEMPORAL", NT), ("session, NO_TEMPORAL | DEMODULATE", NT | D))


def flicker(outs, targets):
    e = [o.astype(np.float64) - t.astype(np.float64) for o, t in zip(outs, targets)]
    return float(np.mean([np.mean((e[i] - e[i - 1]) ** 2) for i in range(1, len(e))]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=180)
    ap.add_argument("--step", type=float, default=1.5)
    args = ap.parse_args()
    import torch
    w, h = args.width, args.height
    scene = rt.huge_scene_arrays(1234)
    ds = rt.DeviceScene(scene, device=0)
    d_rgb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    best = {}
    for mode_name, mode in (("corrected", rt.CORRECTED), ("reference", rt.REFERENCE)):
        cams = [orbit(w, h, args.step * i, mode) for i in range(FRAMES)]
        frames, targets = [], []
        for i, cam in enumerate(cams):
            p = rt.make_params(w, h, SPP, 64, 1 + i)
            beauty, variance, _ = rt.render_var(scene, p, cam)
            frames.append(dict(beauty=beauty, variance=variance, **rt.render_aov(scene, p, cam, SPP)))
            targets.append(rt.render_f32(scene, rt.make_params(w, h, TARGET_SPP, 64, 1000 + i), cam)[0])
        rows = [("(a) raw", [f["beauty"] for f in frames]),
                ("(b) filter alone", [rt.denoise_var(f["beauty"], f["variance"], f["albedo"], f["normal"], f["depth"]) for f in frames])]
        for name, flags in MODES:
            pv = ds.preview(rt.preview_params(w, h, SPP, flags=flags, max_depth=64))
            outs = []
            for i, cam in enumerate(cams):
                pv.frame(cam, 1 + i, d_rgb.data_ptr(), None, stream)
                torch.cuda.synchronize()
                outs.append(d_rgb.cpu().numpy())
            pv.close()
            rows.append((name, outs))
        err = {name: float(np.mean([mse(o, t) for o, t in zip(outs, targets)])) for name, outs in rows}
        raw, alone = err["(a) raw"], err["(b) filter alone"]
        print(f"{mode_name} camera, huge scene {w}x{h}, {FRAMES} frames {args.step} degrees apart, {SPP} spp against "
              f"{TARGET_SPP} spp; mean over the frames")
        print(f"{'row':<36}{'mse':>14}{'/ (a)':>9}{'/ (b)':>9}{'flicker':>14}{'/ (a)':>9}{'/ (b)':>9}")
        fl = {name: flicker(outs, targets) for name, outs in rows}
        for name, _ in rows:
            print(f"{name:<36}{err[name]:14.6e}{err[name] / raw:9.4f}{err[name] / alone:9.4f}{fl[name]:14.6e}"
                  f"{fl[name] / fl['(a) raw']:9.4f}{fl[name] / fl['(b) filter alone']:9.4f}")
        with_history = [n for n, f in MODES if not f & NT]
        best[mode_name] = min(with_history, key=lambda n: err[n])
        print(f"best of the four modes with history by mse: {best[mode_name]} "
              f"({err[best[mode_name]] / alone:.4f} of (b); flicker {fl[best[mode_name]] / fl['(b) filter alone']:.4f} of (b)'s)")
        print()
    ds.close()
    print(f"rt_preview_params_default's flags: the corrected camera's best row, {best['corrected']}")


if __name__ == "__main__":
    main()
