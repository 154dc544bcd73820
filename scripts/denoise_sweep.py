"""The CPU sweep behind rt_denoise_params_default: the simple scene at 64x32 and
4 spp from the oracle, guides from the feature buffers' CPU reference at 4 samples, the target the
oracle's render at a high sample count; the mean squared error of tests/tools/denoise_ref.py's
result against the target, over a grid of levels and sigmas, with and without demodulation. No GPU.

    python scripts/denoise_sweep.py [target_spp]
"""
import itertools
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "tools")]
import aov_ref  # noqa: E402
import denoise_ref  # noqa: E402
import oracle_binding as O  # noqa: E402
import raytracinginoneweekend_amd as rt  # noqa: E402

W, H, SPP, SEED = 64, 32, 4, 1234


def inputs(target_spp):
    s, m = rt.simple_scene_arrays()
    cam = rt.Camera.default(W, H)
    p = rt.make_params(W, H, SPP, 64, SEED)
    noisy, _ = O.render_f32(s, m, cam.c, p)
    target, _ = O.render_f32(s, m, cam.c, rt.make_params(W, H, target_spp, 64, SEED + 1))
    g = aov_ref.render(s, m, cam, p, SPP)
    return noisy, target, g


def mse(a, b):
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def main():
    target_spp = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    noisy, target, g = inputs(target_spp)
    base = mse(noisy, target)
    print(f"simple scene {W}x{H}: mse of the {SPP}-spp image against {target_spp} spp = {base:.6e}")
    rows = []
    for levels, sc, sn, sz, sa in itertools.product((1, 2, 3, 4, 5), (0.0, 0.5, 1.0, 2.0, 4.0), (0.25, 0.5, 1.0, 2.0),
                                                    (0.25, 1.0, 4.0), (0.0, 0.25, 1.0)):
        r = []
        for demod in (False, True):
            out, _ = denoise_ref.denoise(noisy, g["albedo"], g["normal"], g["depth"], levels, sc, sn, sz, sa, demod)
            r.append(mse(out, target) / base)
        rows.append((max(r), r[0], r[1], levels, sc, sn, sz, sa))
    rows.sort()
    print("worse-of-two  plain  demodulated  levels sigma_color sigma_normal sigma_depth sigma_albedo  (mse / 4-spp mse)")
    for r in rows[:12] + rows[-3:]:
        print("%.4f  %.4f  %.4f   %d %g %g %g %g" % r)


if __name__ == "__main__":
    main()
