#!/usr/bin/env python3
"""The sweep behind rt_temporal_clip_default: does a history clamped to the frame's
own colours pay under motion, and does it make a longer history (a lower alpha_min) affordable?

Two sequences, both the huge scene at `--width` x `--height` through RT_PREVIEW_DEMODULATE sessions:

  orbit   §4.12's protocol exactly (scripts/preview_sweep.py): 16 frames of the default camera 1.5 degrees
          apart around its look-at point, 4 spp with a seed per frame against 1024 spp, with the corrected
          and with the reference camera
  moving  §4.16's (scripts/preview_motion.py): a static corrected camera, 16 frames at 8 spp against 1024
          spp, sphere 2 moving 0.05 per frame along +z and spheres 3 and 4 along -z by one rt_scene_update
          per frame; figures over the whole frame and over the pixels on a moved sphere

Rows of each: the filter alone (orbit: rt_denoise_var of the frame, row (b) of §4.12; moving: the session
with rt_preview_reset before every frame, row (b) of §4.16); the session without clip at alpha_min 0.4
(the default, the rows those sections record), 0.2 and 0.1; the session with rt_preview_set_clip over
radius {1, 2, 3} x gamma {0.5, 1, 1.5, 2, 3} x alpha_min {0.4, 0.2, 0.1}. MSE: the mean over the frames of
the mean squared error against the target; flicker: the mean over t of mean((e_t - e_{t-1})^2) with
e = output - target.

The choice: the grid point with the lowest corrected-camera orbit MSE among those whose flicker does not
exceed the unclipped default session's. Needs a GPU; writes the tables to `--out`.

    python scripts/clip_sweep.py [--width 320] [--height 180] [--out profiles/clip/sweep.txt]
"""
import argparse
import functools
import itertools
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raytracinginoneweekend_amd as rt  # noqa: E402
from preview_motion import FRAMES as M_FRAMES, MOVED, SPP as M_SPP, TARGET_SPP as M_TARGET_SPP, figures, records  # noqa: E402
from preview_sweep import flicker  # noqa: E402
from temporal_sweep import FRAMES, SPP, TARGET_SPP, mse, orbit  # noqa: E402

RADII, GAMMAS, ALPHAS = (1, 2, 3), (0.5, 1.0, 1.5, 2.0, 3.0), (0.4, 0.2, 0.1)
GRID = list(itertools.product(ALPHAS, RADII, GAMMAS))
STEP_DEG = 1.5


def label(alpha_min, radius=None, gamma=None):
    return f"session, alpha_min {alpha_min}" + ("" if radius is None else f", clip r {radius} gamma {gamma}")


def session_rows():
    """(label, alpha_min, clip record or None) of every session row."""
    rows = [(label(a), a, None) for a in ALPHAS]
    return rows + [(label(a, r, g), a, rt.temporal_clip(radius=r, gamma=g)) for a, r, g in GRID]


def run_session(ds, w, h, spp, alpha_min, clip, cams, d_rgb, stream, before_frame=None):
    import torch
    pv = ds.preview(rt.preview_params(w, h, spp, max_depth=64, temporal=dict(alpha_min=alpha_min)))
    pv.set_clip(clip)
    outs = []
    for i, cam in enumerate(cams):
        if before_frame:
            before_frame(i, pv)
        pv.frame(cam, 1 + i, d_rgb.data_ptr(), None, stream)
        torch.cuda.synchronize()
        outs.append(d_rgb.cpu().numpy())
    pv.close()
    return outs


def orbit_part(w, h, mode_name, mode, d_rgb, stream, say):
    scene = rt.huge_scene_arrays(1234)
    ds = rt.DeviceScene(scene, device=0)
    cams = [orbit(w, h, STEP_DEG * i, mode) for i in range(FRAMES)]
    frames, targets = [], []
    for i, cam in enumerate(cams):
        p = rt.make_params(w, h, SPP, 64, 1 + i)
        beauty, variance, _ = rt.render_var(scene, p, cam)
        frames.append(dict(beauty=beauty, variance=variance, **rt.render_aov(scene, p, cam, SPP)))
        targets.append(rt.render_f32(scene, rt.make_params(w, h, TARGET_SPP, 64, 1000 + i), cam)[0])
    print(f"orbit, {mode_name}: frames and targets rendered", flush=True)
    rows = [("filter alone", [rt.denoise_var(f["beauty"], f["variance"], f["albedo"], f["normal"], f["depth"]) for f in frames])]
    for name, alpha_min, clip in session_rows():
        rows.append((name, run_session(ds, w, h, SPP, alpha_min, clip, cams, d_rgb, stream)))
        print(f"orbit, {mode_name}: {name}", flush=True)
    ds.close()
    fig = {name: (float(np.mean([mse(o, t) for o, t in zip(outs, targets)])), flicker(outs, targets)) for name, outs in rows}
    alone, base = fig["filter alone"], fig[label(0.4)]
    say(f"orbit, {mode_name} camera, huge scene {w}x{h}, {FRAMES} frames {STEP_DEG} degrees apart, {SPP} spp against "
        f"{TARGET_SPP} spp, RT_PREVIEW_DEMODULATE; means over the frames; 'alone': the filter alone, 'session': the "
        f"unclipped session at alpha_min 0.4")
    say(f"{'row':<48}{'mse':>14}{'/ alone':>9}{'/ session':>10}{'flicker':>14}{'/ alone':>9}{'/ session':>10}")
    for name, _ in rows:
        m, f = fig[name]
        say(f"{name:<48}{m:14.6e}{m / alone[0]:9.4f}{m / base[0]:10.4f}{f:14.6e}{f / alone[1]:9.4f}{f / base[1]:10.4f}")
    say("")
    return fig


def moving_part(w, h, d_rgb, stream, say):
    cam = rt.Camera.default(w, h, rt.CORRECTED)
    recs = functools.lru_cache(maxsize=None)(records)
    targets, masks = [], []
    for i in range(M_FRAMES):
        targets.append(rt.render_f32(recs(i), rt.make_params(w, h, M_TARGET_SPP, 64, 1000 + i), cam)[0])
        ids = rt.render_aov(recs(i), rt.make_params(w, h, M_SPP, 64, 1 + i), cam, M_SPP, ("sphere_id",))["sphere_id"]
        masks.append(np.isin(ids, MOVED))
    print("moving: targets rendered", flush=True)
    cams = [cam] * M_FRAMES
    rows = []
    for name, alpha_min, clip, reset in [("filter alone", 0.4, None, True)] + [r + (False,) for r in session_rows()]:
        ds = rt.DeviceScene(recs(0), device=0)

        def before(i, pv):
            if i:
                ds.update(recs(i))
            if reset:
                pv.reset()

        rows.append((name, run_session(ds, w, h, M_SPP, alpha_min, clip, cams, d_rgb, stream, before)))
        ds.close()
        print(f"moving: {name}", flush=True)
    fig = {name: figures(outs, targets, None) + figures(outs, targets, masks) for name, outs in rows}
    alone, base = fig["filter alone"], fig[label(0.4)]
    say(f"moving spheres, huge scene {w}x{h}, static corrected camera, {M_FRAMES} frames, {M_SPP} spp against {M_TARGET_SPP} "
        f"spp; sphere 2 moves 0.05 per frame along +z, spheres 3 and 4 along -z; moved pixels: "
        f"{int(np.mean([m.sum() for m in masks]))} of {w * h} per frame on average; the ratios are to the filter alone")
    say(f"{'row':<48}{'mse, frame':>14}{'/ alone':>9}{'flicker, frame':>16}{'/ alone':>9}{'mse, moved':>14}{'/ alone':>9}"
        f"{'flicker, moved':>16}{'/ alone':>9}")
    for name, _ in rows:
        v = fig[name]
        say(f"{name:<48}{v[0]:14.6e}{v[0] / alone[0]:9.4f}{v[1]:16.6e}{v[1] / alone[1]:9.4f}{v[2]:14.6e}{v[2] / alone[2]:9.4f}"
            f"{v[3]:16.6e}{v[3] / alone[3]:9.4f}")
    say(f"the unclipped default session against the filter alone: mse {base[0] / alone[0]:.4f} (frame) {base[2] / alone[2]:.4f} "
        f"(moved pixels); flicker {base[1] / alone[1]:.4f} (frame) {base[3] / alone[3]:.4f} (moved pixels)")
    say("")
    return fig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=180)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "clip", "sweep.txt"))
    args = ap.parse_args()
    import torch
    w, h = args.width, args.height
    d_rgb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    lines = []
    say = lines.append
    corrected = orbit_part(w, h, "corrected", rt.CORRECTED, d_rgb, stream, say)
    reference = orbit_part(w, h, "reference", rt.REFERENCE, d_rgb, stream, say)
    moving = moving_part(w, h, d_rgb, stream, say)

    # the choice, on the corrected camera's orbit
    alone, base = corrected["filter alone"], corrected[label(0.4)]
    ok = [(a, r, g) for a, r, g in GRID if corrected[label(a, r, g)][1] <= base[1]]
    say(f"grid points whose flicker does not exceed the unclipped session's ({base[1]:.6e}): {len(ok)} of {len(GRID)}")
    best = min(ok, key=lambda k: corrected[label(*k)][0]) if ok else None
    if best is not None:
        a, r, g = best
        m, f = corrected[label(a, r, g)]
        say(f"lowest mse among them: alpha_min {a}, radius {r}, gamma {g}: mse {m:.6e} = {m / base[0]:.4f} of the unclipped "
            f"session's, {m / alone[0]:.4f} of the filter alone's; flicker {f / base[1]:.4f} of the session's")
        mr, mm = reference[label(a, r, g)], moving[label(a, r, g)]
        say(f"the same point elsewhere: reference camera mse {mr[0] / reference[label(0.4)][0]:.4f} of the unclipped session's; "
            f"moving spheres mse {mm[0] / moving[label(0.4)][0]:.4f} (frame) {mm[2] / moving[label(0.4)][2]:.4f} (moved pixels) "
            f"of the unclipped session's, {mm[2] / moving['filter alone'][2]:.4f} of the filter alone's on the moved pixels")
    if best is None or corrected[label(*best)][0] >= base[0]:
        say("no grid point beats the unclipped session by mse on the corrected camera: rt_temporal_clip_default keeps "
            "radius 1, gamma 1")
    else:
        say(f"rt_temporal_clip_default: radius {best[1]}, gamma {best[2]}" +
            ("" if best[0] == 0.4 else f" (found at alpha_min {best[0]}; rt_temporal_params_default's alpha_min is not changed)"))
        beats_filter = corrected[label(*best)][0] < alone[0]
        say("with it the session " + ("beats" if beats_filter else "still does not beat") + " the filter alone by mse on the "
            "corrected camera")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
