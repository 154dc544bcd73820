"""The CPU sweep behind rt_denoise_var_params_default: the quality case of
tests/test_denoise_cpu.py (the simple scene at 64x32, 4 spp from the oracle, guides from the feature
buffers' CPU reference at 4 samples, the target the oracle's render at 1024 spp), the variance plane
from tests/tools/moments_ref.py; the mean squared error of tests/tools/denoise_var_ref.py's result
against the target over a grid of levels, sigmas and var_floor, beside the plain denoiser's with its
own defaults. The first row of the table is the choice. No GPU.

    python scripts/denoise_var_sweep.py [target_spp]
"""
import itertools
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "tools")]
import aov_ref  # noqa: E402
import denoise_ref  # noqa: E402
import denoise_var_ref  # noqa: E402
import moments_ref  # noqa: E402
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
    rgb, var, _ = moments_ref.render(s, m, cam, p)
    assert np.array_equal(rgb.view(np.uint32), noisy.view(np.uint32))
    return noisy, target, g, var


def mse(a, b):
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def main():
    target_spp = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    noisy, target, g, var = inputs(target_spp)
    base = mse(noisy, target)
    print(f"simple scene {W}x{H}: mse of the {SPP}-spp image against {target_spp} spp = {base:.6e}")
    plain, _ = denoise_ref.denoise(noisy, g["albedo"], g["normal"], g["depth"],
                                   **denoise_ref.params_kwargs(rt.denoise_params(W, H)))
    print(f"plain denoiser, its defaults: {mse(plain, target) / base:.4f}")
    rows = []
    for levels, sc, sn, sz, sa, fl in itertools.product((1, 2, 3, 4, 5), (0.0, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0),
                                                        (0.5, 1.0, 2.0), (0.25, 1.0, 4.0), (0.0, 0.25, 1.0),
                                                        (1e-6, 1e-4, 1e-2, 1.0)):
        if sc == 0.0 and fl != 1e-4:
            continue  # the floor is not used without the colour term
        out, _, _ = denoise_var_ref.denoise(noisy, var, g["albedo"], g["normal"], g["depth"], levels, sc, sn, sz, sa, fl)
        rows.append((mse(out, target) / base, levels, sc, sn, sz, sa, fl))
    rows.sort()
    head = "mse / 4-spp mse   levels sigma_color sigma_normal sigma_depth sigma_albedo var_floor"
    # the defaults are the best row whose colour term is on: the entry point exists to use the variance
    print("colour term on (sigma_color > 0); the first row is rt_denoise_var_params_default's\n" + head)
    for r in [r for r in rows if r[2] != 0.0][:12]:
        print("%.4f   %d %g %g %g %g %g" % r)
    print("colour term off (sigma_color = 0: the guides alone, the variance only propagated)\n" + head)
    for r in [r for r in rows if r[2] == 0.0][:4]:
        print("%.4f   %d %g %g %g %g %g" % r)
    print("the worst rows\n" + head)
    for r in rows[-3:]:
        print("%.4f   %d %g %g %g %g %g" % r)


if __name__ == "__main__":
    main()
