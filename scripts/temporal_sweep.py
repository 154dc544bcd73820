#!/usr/bin/env python3
"""The sweep behind rt_temporal_params_default: a 16-frame orbit of the default
camera around its look-at point (`--step` degrees per frame, corrected camera, the huge scene at
`--width` x `--height`), every frame rendered at 4 spp with a seed of its own (rt_render_var, guides
from rt_render_aov over the same samples) and at 1024 spp as its target. Per frame the mean squared
error against the target of

    (a) the 4-spp frame
    (b) rt_denoise_var of that frame alone, its default parameters
    (c) rt_temporal (the accumulated colour and variance fed back as prev) followed by rt_denoise_var
        with the same parameters

averaged over the 16 frames, (c) over a grid of alpha_min, max_history, normal_tol and depth_tol. The
first row of the table is the choice (among rows that tie, the starting value). The reference
camera's orbit is reported for the library defaults and the starting point. Needs a GPU (every stage
runs through the library's host calls); prints the table (kept as profiles/temporal/sweep.txt, and
at 640x360 as profiles/temporal/sweep_640x360.txt).

    python scripts/temporal_sweep.py [--width 320] [--height 180] [--step 1.5] > profiles/temporal/sweep.txt
"""
import argparse
import itertools
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import raytracinginoneweekend_amd as rt  # noqa: E402

FRAMES, SPP, TARGET_SPP = 16, 4, 1024
GRID = dict(alpha_min=(0.05, 0.1, 0.2, 0.4), max_history=(8.0, 32.0, 128.0), normal_tol=(0.01, 0.1, 0.5),
            depth_tol=(0.02, 0.1, 0.3))
START = dict(alpha_min=0.2, max_history=32.0, normal_tol=0.1, depth_tol=0.1)  # SVGF's alpha and round figures


def orbit(w, h, degrees, mode):
    """The default camera turned by `degrees` around the vertical axis through its look-at point."""
    pos, look = np.array([-4.0, 3.2, 5.0]), np.array([0.0, 1.0, 0.0])
    a = math.radians(degrees)
    d = pos - look
    p = look + np.array([d[0] * math.cos(a) + d[2] * math.sin(a), d[1], -d[0] * math.sin(a) + d[2] * math.cos(a)])
    focus = float(np.float32(np.linalg.norm((p - look).astype(np.float32))))
    return rt.Camera(tuple(p), tuple(look), (0, 1, 0), w / h, 42.0, 0.0625, focus, mode)


def mse(a, b):
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def sequence(frames, cams, targets, **par):
    """Mean over the frames of (c)'s error, and the mean share of pixels that kept a history."""
    prev, errs, kept = None, [], []
    for i, f in enumerate(frames):
        cur = {n: f[n] for n in ("beauty", "variance", "normal", "depth", "alpha", "sphere_id")}
        color, variance, history = rt.temporal(cur, prev, cams[i], cams[i - 1] if i else None, **par)
        out = rt.denoise_var(color, variance, f["albedo"], f["normal"], f["depth"])
        errs.append(mse(out, targets[i]))
        kept.append(float((history > 1).mean()))
        prev = dict(color=color, variance=variance, history=history, normal=f["normal"], depth=f["depth"],
                    sphere_id=f["sphere_id"])
    return float(np.mean(errs)), float(np.mean(kept[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=180)
    ap.add_argument("--step", type=float, default=1.5)
    args = ap.parse_args()
    w, h = args.width, args.height
    scene = rt.huge_scene_arrays(1234)
    for mode_name, mode in (("corrected", rt.CORRECTED), ("reference", rt.REFERENCE)):
        cams = [orbit(w, h, args.step * i, mode) for i in range(FRAMES)]
        frames, targets = [], []
        for i, cam in enumerate(cams):
            p = rt.make_params(w, h, SPP, 64, 1 + i)
            beauty, variance, _ = rt.render_var(scene, p, cam)
            frames.append(dict(beauty=beauty, variance=variance, **rt.render_aov(scene, p, cam, SPP)))
            targets.append(rt.render_f32(scene, rt.make_params(w, h, TARGET_SPP, 64, 1000 + i), cam)[0])
        raw = float(np.mean([mse(f["beauty"], t) for f, t in zip(frames, targets)]))
        alone = float(np.mean([mse(rt.denoise_var(f["beauty"], f["variance"], f["albedo"], f["normal"], f["depth"]), t)
                               for f, t in zip(frames, targets)]))
        print(f"{mode_name} camera, huge scene {w}x{h}, {FRAMES} frames {args.step} degrees apart, {SPP} spp against "
              f"{TARGET_SPP} spp; mean squared error, mean over the frames")
        print(f"(a) raw {raw:.6e}   (b) denoise_var alone {alone:.6e} ({alone / raw:.4f} of raw)")
        if mode != rt.CORRECTED:
            # the grid is swept on the corrected camera (the pinhole picture); here the chosen row and the start
            for name, par in (("library defaults", {}), ("starting point", START)):
                err, kept = sequence(frames, cams, targets, **par)
                print(f"(c) temporal + denoise_var, {name}: {err:.6e} ({err / raw:.4f} of raw, {err / alone:.4f} of (b)), "
                      f"{100 * kept:.1f}% of the pixels keep a history")
            continue
        rows = []
        for values in itertools.product(*GRID.values()):
            par = dict(zip(GRID, values))
            err, kept = sequence(frames, cams, targets, **par)
            rows.append((err / raw, err / alone, kept) + values)
        rows.sort()
        head = "(c) / raw  (c) / (b)  kept   " + " ".join(GRID)
        print("(c) temporal + denoise_var over the grid; the first row is rt_temporal_params_default's\n" + head)
        for r in rows[:12]:
            print("%.4f     %.4f     %.3f  %g %g %g %g" % r)
        print("the starting point and the library defaults\n" + head)
        for par in (START, {}):
            err, kept = sequence(frames, cams, targets, **par)
            d = rt.temporal_params(w, h, **par)
            print("%.4f     %.4f     %.3f  %g %g %g %g" % (err / raw, err / alone, kept, d.alpha_min, d.max_history,
                                                           d.normal_tol, d.depth_tol))
        print("the worst rows\n" + head)
        for r in rows[-3:]:
            print("%.4f     %.4f     %.3f  %g %g %g %g" % r)


if __name__ == "__main__":
    main()
