"""The upscaled preview session on the GPU (rt_preview_create_upscaled, rt_preview_output; DESIGN.md
§4.15).

Every comparison is on uint32 (or uint8) views with zero mismatches allowed. The huge scene, the
corrected camera on the preview module's 1.5 degree orbit (with the output's aspect: one camera
serves both sizes), 4 spp, max_depth 8, three frames with seeds 1..3, rendered at 32 x 18 and shown at
64 x 36, and at 35 x 19 shown at 70 x 37.

The hand-made chain an upscaled frame must equal: an ordinary session of the same params, its
planes read through rt_preview_planes; its filter output, which is rt_denoise_var_device's run of
every level over the planes the session reports as out_color and out_variance with its guides (under
FEEDBACK too: the first level of that run is the run that made C_1, V_1; the module checks this
reconstruction against the ordinary session's own image); then rt_render_aov_device at the output
size, rt_upsample_device and rt_preview_merge_device.
"""
import functools
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi
from raytracinginoneweekend_amd import render

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
from device_io import SENTINEL, Outputs, plane, read_planes  # noqa: E402
from support import assert_bits as assert_same, frozen, orbit_camera as camera, words as u32  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SCENE_SEED, SPP, MAX_DEPTH, FRAMES = 1234, 4, 8, 3
SIZES = [(32, 18, 64, 36), (35, 19, 70, 37)]
DEMOD, FEEDBACK, NO_TEMPORAL = abi.RT_PREVIEW_DEMODULATE, abi.RT_PREVIEW_FEEDBACK, abi.RT_PREVIEW_NO_TEMPORAL
MODES = {"plain": 0, "demodulate": DEMOD, "demodulate-feedback": DEMOD | FEEDBACK, "no-temporal": NO_TEMPORAL}
GUIDES = ("normal", "depth", "alpha", "sphere_id")


@functools.lru_cache(maxsize=None)
def scene():
    return rt.huge_scene_arrays(SCENE_SEED)


@functools.lru_cache(maxsize=None)
def device_scene():
    return rt.DeviceScene(scene(), device=0)


@functools.lru_cache(maxsize=None)
def output_guides(w, h, i, samples=0):
    """The feature buffers of the output size from the public synchronous call, once."""
    return frozen(rt.render_aov(scene(), rt.make_params(w, h, SPP, MAX_DEPTH, 1 + i), camera(w, h, i), samples))


def params(w, h, flags, levels=2):
    return rt.preview_params(w, h, SPP, flags=flags, max_depth=MAX_DEPTH, denoise=dict(levels=levels))


def read_output(pv):
    o = pv.output()
    return read_planes(pv, o["width"], o["height"], abi.PREVIEW_OUTPUT_PLANES, o)


Images = functools.partial(Outputs, own_stream=False)  # the caller brings the stream


def expected_usage(lw, lh, w, h, flags, levels):
    """The planes the contract needs, floats per pixel, each rounded up to 256 bytes: the ordinary
    session's at the render size, then the guides (the albedo under DEMODULATE only) and the upsampled
    image at the output size."""
    temporal, feedback, demod = not flags & NO_TEMPORAL, bool(flags & FEEDBACK), bool(flags & DEMOD)
    planes = [3, 1, 3, 1] + [3, 1] * demod + [3, 1, 1] * (2 if temporal else 1) + [3, 1, 1] * (2 * temporal)
    planes += [3, 1] * feedback + [3] + [3, 2] * (levels > (2 if feedback else 1))
    out = [3] * demod + [3, 1, 1, 1, 3]
    return sum((4 * lw * lh * c + 255) // 256 * 256 for c in planes) + sum((4 * w * h * c + 255) // 256 * 256 for c in out)


@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("lw,lh,w,h", SIZES)
def test_upscaled_frames_equal_the_chain_made_by_hand(lw, lh, w, h, mode, levels):
    import torch
    flags = MODES[mode]
    demod = bool(flags & DEMOD)
    ds, p = device_scene(), params(lw, lh, flags, levels)
    u = rt.preview_upscale(p, w, h)
    ordinary, upscaled = ds.preview(p), ds.preview(p, u)
    assert (upscaled.width, upscaled.height, upscaled.out_width, upscaled.out_height) == (lw, lh, w, h)
    assert upscaled.usage() == expected_usage(lw, lh, w, h, flags, levels)
    assert all(v is None for n, v in upscaled.output().items() if n not in ("width", "height"))
    lo_img, own, hand, check = Images(lw, lh), Images(w, h), Images(w, h), Images(lw, lh)
    filtered, scratch, var_scratch = plane(lw, lh, 3), plane(lw, lh, 3), plane(lw, lh, 2)
    g = dict(albedo=plane(w, h, 3), normal=plane(w, h, 3), depth=plane(w, h, 1), alpha=plane(w, h, 1),
             sphere_id=plane(w, h, 1, torch.int32))
    upsampled = plane(w, h, 3)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    up_params = rt.upsample_params(w, h, lw, lh, normal_tol=u.normal_tol, depth_tol=u.depth_tol)
    for i in range(FRAMES):
        cam, seed = camera(w, h, i), 1 + i
        # the ordinary session's frame, then the rest of the chain by hand over its planes
        ordinary.frame(cam, seed, lo_img.rgb.data_ptr(), lo_img.rgb8.data_ptr(), st.cuda_stream)
        pl = ordinary.planes()
        rt.denoise_var_device(dict(beauty=pl["out_color"], albedo=pl["albedo"], normal=pl["normal"], depth=pl["depth"],
                                   out=filtered.data_ptr(), scratch=scratch.data_ptr()), p.denoise,
                              render.denoise_var_buffers(dict(variance=pl["out_variance"], var_scratch=var_scratch.data_ptr()),
                                                         p.var_floor), st.cuda_stream)
        rt.preview_merge_device(lw, lh, filtered.data_ptr(), pl["albedo"] if demod else None, check.rgb.data_ptr(), None,
                                st.cuda_stream)
        ds.render_aov(cam, rt.make_params(w, h, SPP, MAX_DEPTH, seed),
                      {n: t.data_ptr() for n, t in g.items() if demod or n != "albedo"}, 0, st.cuda_stream)
        rt.upsample_device(dict(lo_color=filtered.data_ptr(), lo_normal=pl["normal"], lo_depth=pl["depth"],
                                lo_sphere_id=pl["sphere_id"], out_color=upsampled.data_ptr(),
                                **{n: g[n].data_ptr() for n in GUIDES}), up_params, st.cuda_stream)
        rt.preview_merge_device(w, h, upsampled.data_ptr(), g["albedo"].data_ptr() if demod else None, hand.rgb.data_ptr(),
                                hand.rgb8.data_ptr(), st.cuda_stream)
        st.synchronize()
        want_planes = read_planes(ordinary, lw, lh)
        # (the filter output reconstructed above is the one the ordinary session merged)
        assert_same(check.rgb.cpu().numpy(), lo_img.rgb.cpu().numpy(), f"frame {i}: the reconstructed filter output, merged")
        # the upscaled session's frame
        upscaled.frame(cam, seed, own.rgb.data_ptr(), own.rgb8.data_ptr(), st.cuda_stream)
        st.synchronize()
        (rgb, rgb8), (want, want8) = own.host(), hand.host()
        assert (rgb != SENTINEL).all()
        assert_same(rgb, want, f"frame {i} d_rgb")
        assert np.array_equal(rgb8, want8), f"frame {i} d_rgb8"
        # upscaling changes nothing at the render size
        got_planes = read_planes(upscaled, lw, lh)
        assert upscaled.planes()["frames"] == i + 1
        for n, a in want_planes.items():
            if a is None:
                assert got_planes[n] is None, n
            else:
                assert_same(got_planes[n], a, f"frame {i} render-size plane {n}")
        # the output-size planes: the guides of the public call, the upsampled image of the chain
        out = read_output(upscaled)
        assert (out["albedo"] is not None) == demod
        for n in GUIDES + (("albedo",) if demod else ()):
            assert_same(out[n], output_guides(w, h, i)[n], f"frame {i} output-size {n} against rt_render_aov")
        assert_same(out["upsampled"], upsampled.cpu().numpy(), f"frame {i} upsampled")
    ordinary.close()
    upscaled.close()


def test_one_guide_sample():
    """guide_samples = 1: the output-size guides are rt_render_aov's with samples = 1, they differ from
    those of every sample, and the render-size planes do not depend on it."""
    lw, lh, w, h = SIZES[1]
    ds, p = device_scene(), params(lw, lh, DEMOD, 2)
    one, every = ds.preview(p, rt.preview_upscale(p, w, h, guide_samples=1)), ds.preview(p, rt.preview_upscale(p, w, h))
    img = Images(w, h)
    import torch
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    got = []
    for pv in (one, every):
        pv.frame(camera(w, h, 0), 1, img.rgb.data_ptr(), None, st.cuda_stream)
        st.synchronize()
        got.append((read_output(pv), read_planes(pv, lw, lh), img.rgb.cpu().numpy()))
    for n in GUIDES + ("albedo",):
        assert_same(got[0][0][n], output_guides(w, h, 0, 1)[n], f"{n} with one guide sample")
        assert_same(got[1][0][n], output_guides(w, h, 0)[n], f"{n} with every sample")
    assert (u32(got[0][0]["normal"]) != u32(got[1][0]["normal"])).any()
    for n in ("out_color", "normal", "sphere_id"):
        assert_same(got[0][1][n], got[1][1][n], f"render-size {n}")
    assert (u32(got[0][2]) != u32(got[1][2])).any()
    one.close()
    every.close()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_usage_counts_the_output_size_planes(mode):
    lw, lh, w, h = SIZES[1]
    for levels in (1, 2, 3):
        p = params(lw, lh, MODES[mode], levels)
        pv = device_scene().preview(p, rt.preview_upscale(p, w, h))
        assert pv.usage() == expected_usage(lw, lh, w, h, MODES[mode], levels), (mode, levels)
        pv.close()


def test_output_of_an_ordinary_session_is_refused():
    pv = device_scene().preview(params(35, 19, 0, 2))
    with pytest.raises(rt.RtError) as e:
        pv.output()
    assert e.value.status == abi.RT_ERR_INVALID and "rt_preview_output" in str(e.value)
    pv.close()


def test_reset_behaves_as_before():
    lw, lh, w, h = SIZES[1]
    flags = DEMOD | FEEDBACK
    p = params(lw, lh, flags, 2)
    u = rt.preview_upscale(p, w, h)
    import torch
    img = Images(w, h)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()

    def frame(pv, i):
        pv.frame(camera(w, h, i), 1 + i, img.rgb.data_ptr(), None, st.cuda_stream)
        st.synchronize()
        return img.rgb.cpu().numpy()

    pv = device_scene().preview(p, u)
    frame(pv, 0)
    ab = frame(pv, 1)                                   # A, B
    assert pv.planes()["frames"] == 2
    pv.reset()
    assert pv.planes()["frames"] == 0
    b = frame(pv, 1)                                    # B after a reset
    hist = read_planes(pv, lw, lh)["out_history"]
    fresh = device_scene().preview(p, u)
    first = frame(fresh, 1)                             # B as a first frame
    assert_same(b, first, "a frame after reset against a first frame")
    assert (hist == 1).all()
    assert (u32(ab) != u32(b)).any()                    # the history mattered
    pv.close()
    fresh.close()
