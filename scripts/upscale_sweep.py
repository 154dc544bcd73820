#!/usr/bin/env python3
"""The sweep behind rt_upsample_params_default's tolerances, and what a render scale of one half costs in
quality: §4.11's 16-frame orbit of the default camera around its look-at point
(`--step` degrees per frame, the huge scene), output `--width` x `--height`, every frame with a seed
of its own against the same frame at 1024 spp at the output size, with the corrected and with the
reference camera. Rows, each a preview session (max_depth 64; the library's defaults but for what the
row names):

    full size, 8 spp                   an ordinary session at the output size
    full size, 2 spp                   the same at 2 spp: as many paths per frame as the rows below trace
    half size, 8 spp, upscaled         rendered at half the width and height, DEMODULATE (the default)
    ... without DEMODULATE             flags 0: the albedo is upsampled with the illumination
    ... bilinear                       normal_tol = depth_tol = 0: every surface pixel whose taps do
                                       not repeat its depth bit for bit falls back to the plain bilinear
                                       value (sky and edge pixels take the id test alone); what the guides buy

then the grid normal_tol {0.01, 0.1, 0.5} x depth_tol {0.02, 0.1, 0.3} over the upscaled DEMODULATE
row, which starts from the temporal stage's defaults (0.5, 0.1). Per row: the mean over the frames of
the mean squared error against the target, that figure over the first row's, and the flicker figure
of scripts/preview_sweep.py. Needs a GPU; prints the tables (kept as profiles/upscale/sweep.txt).

    python scripts/upscale_sweep.py [--width 320] [--height 180] [--step 1.5] > profiles/upscale/sweep.txt
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raytracinginoneweekend_amd as rt  # noqa: E402
from preview_sweep import flicker  # noqa: E402
from temporal_sweep import FRAMES, TARGET_SPP, mse, orbit  # noqa: E402

GRID_NORMAL, GRID_DEPTH = (0.01, 0.1, 0.5), (0.02, 0.1, 0.3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=180)
    ap.add_argument("--step", type=float, default=1.5)
    args = ap.parse_args()
    import torch
    w, h = args.width, args.height
    lw, lh = w // 2, h // 2
    scene = rt.huge_scene_arrays(1234)
    ds = rt.DeviceScene(scene, device=0)
    d_rgb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    default = rt.upsample_params(w, h, lw, lh)

    def run(cams, pw, ph, spp, flags=None, **upscale):
        p = rt.preview_params(pw, ph, spp, max_depth=64) if flags is None else rt.preview_params(pw, ph, spp, max_depth=64, flags=flags)
        pv = ds.preview(p, rt.preview_upscale(p, w, h, **upscale) if (pw, ph) != (w, h) else None)
        outs = []
        for i, cam in enumerate(cams):
            pv.frame(cam, 1 + i, d_rgb.data_ptr(), None, stream)
            torch.cuda.synchronize()
            outs.append(d_rgb.cpu().numpy())
        pv.close()
        return outs

    chosen = {}
    for mode_name, mode in (("corrected", rt.CORRECTED), ("reference", rt.REFERENCE)):
        cams = [orbit(w, h, args.step * i, mode) for i in range(FRAMES)]
        targets = [rt.render_f32(scene, rt.make_params(w, h, TARGET_SPP, 64, 1000 + i), cam)[0] for i, cam in enumerate(cams)]
        rows = [("full size, 8 spp", run(cams, w, h, 8)), ("full size, 2 spp", run(cams, w, h, 2)),
                ("half size, 8 spp, upscaled", run(cams, lw, lh, 8)),
                ("half size, 8 spp, upscaled, flags 0", run(cams, lw, lh, 8, flags=0)),
                ("half size, 8 spp, bilinear", run(cams, lw, lh, 8, normal_tol=0.0, depth_tol=0.0))]
        err = {name: float(np.mean([mse(o, t) for o, t in zip(outs, targets)])) for name, outs in rows}
        fl = {name: flicker(outs, targets) for name, outs in rows}
        full = rows[0][0]
        print(f"{mode_name} camera, huge scene, output {w}x{h}, half size {lw}x{lh}, {FRAMES} frames {args.step} degrees apart "
              f"against {TARGET_SPP} spp; default tolerances normal_tol {default.normal_tol:g}, depth_tol {default.depth_tol:g}; "
              "mean over the frames")
        print(f"{'row':<40}{'mse':>14}{'/ full 8':>10}{'flicker':>14}{'/ full 8':>10}")
        for name, _ in rows:
            print(f"{name:<40}{err[name]:14.6e}{err[name] / err[full]:10.4f}{fl[name]:14.6e}{fl[name] / fl[full]:10.4f}")
        print(f"{'normal_tol':>12}{'depth_tol':>11}{'mse':>14}{'/ full 8':>10}{'flicker':>14}{'/ full 8':>10}")
        grid = {}
        for nt in GRID_NORMAL:
            for dt in GRID_DEPTH:
                outs = run(cams, lw, lh, 8, normal_tol=nt, depth_tol=dt)
                e = float(np.mean([mse(o, t) for o, t in zip(outs, targets)]))
                f = flicker(outs, targets)
                grid[(nt, dt)] = e
                print(f"{nt:12g}{dt:11g}{e:14.6e}{e / err[full]:10.4f}{f:14.6e}{f / fl[full]:10.4f}")
        chosen[mode_name] = min(grid, key=grid.get)
        print(f"least mse of the grid: normal_tol {chosen[mode_name][0]:g}, depth_tol {chosen[mode_name][1]:g}")
        print()
    ds.close()
    print(f"rt_upsample_params_default's tolerances: the corrected camera's, normal_tol {chosen['corrected'][0]:g}, "
          f"depth_tol {chosen['corrected'][1]:g}")


if __name__ == "__main__":
    main()
