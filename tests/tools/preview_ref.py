"""TEST INFRASTRUCTURE: CPU restatement of one frame of a preview session (include/rt_api.h,
rt_preview_frame_device) in numpy float32, from the frame's rendered planes on:
written from the contract and not from the library.

    illum, illum_var = preview_ref.split(beauty, variance, albedo)
    out = preview_ref.merge(filtered, albedo)        # albedo None: the filter's bits
    s = preview_ref.Session(params)                  # an rt_preview_params record
    r = s.frame(cur, camera)                         # cur: beauty, variance, albedo, normal, depth, alpha, sphere_id
    r["out"], r["color"], r["variance"], r["history"], r["reason"]
    s.reset()

The middle of a frame is temporal_ref.accumulate and denoise_var_ref.denoise. The feedback rule: a
levels = 1 run of the filter gives C_1, V_1, which the next frame reprojects; the run with every level
gives the frame's output (its first level is that same run, so levels 1.. continue from C_1, V_1).
Under RT_PREVIEW_NO_TEMPORAL color and variance are the filter's inputs themselves, history and
reason are None. The session keeps what the next frame takes as prev (s.prev, s.prev_camera).
"""
import numpy as np

import denoise_var_ref
import temporal_ref

F = np.float32
DEMODULATE, FEEDBACK, NO_TEMPORAL = 1, 2, 4
FLOOR = F(0.0078125)
GUIDES = ("normal", "depth", "sphere_id")


def _f32(a):
    a = np.asarray(a)
    assert a.dtype == np.float32
    return a


def floored(albedo):
    """A' of the contract."""
    return np.maximum(_f32(albedo), FLOOR)


def split(beauty, variance, albedo):
    a = floored(albedo)
    illum = _f32(beauty) / a
    la = (F(0.2126) * a[..., 0] + F(0.7152) * a[..., 1]) + F(0.0722) * a[..., 2]
    illum_var = _f32(variance) / (la * la)
    assert illum.dtype == F and illum_var.dtype == F
    return illum, illum_var


def merge(filtered, albedo=None):
    if albedo is None:
        return _f32(filtered).copy()
    out = _f32(filtered) * floored(albedo)
    assert out.dtype == F
    return out


class Session:
    def __init__(self, params):
        self.p = params
        self.prev = None
        self.prev_camera = None

    def reset(self):
        self.prev = None

    def frame(self, cur, camera):
        p, fl = self.p, self.p.flags
        color, variance = _f32(cur["beauty"]), _f32(cur["variance"])
        if fl & DEMODULATE:
            color, variance = split(color, variance, cur["albedo"])
        history = reason = None
        if not fl & NO_TEMPORAL:
            tcur = dict(beauty=color, variance=variance, alpha=cur["alpha"], **{n: cur[n] for n in GUIDES})
            color, variance, history, reason = temporal_ref.accumulate(tcur, self.prev, camera, self.prev_camera, p.temporal)
        kw = dict(sigma_color=p.denoise.sigma_color, sigma_normal=p.denoise.sigma_normal,
                  sigma_depth=p.denoise.sigma_depth, sigma_albedo=p.denoise.sigma_albedo, var_floor=p.var_floor)
        guides = (cur["albedo"], cur["normal"], cur["depth"])
        filtered = denoise_var_ref.denoise(color, variance, *guides, levels=p.denoise.levels, **kw)[0]
        back_c, back_v = color, variance
        if fl & FEEDBACK:
            back_c, back_v, _ = denoise_var_ref.denoise(color, variance, *guides, levels=1, **kw)
        if not fl & NO_TEMPORAL:
            self.prev = dict(color=back_c, variance=back_v, history=history, **{n: cur[n] for n in GUIDES})
            self.prev_camera = camera
        out = merge(filtered, cur["albedo"] if fl & DEMODULATE else None)
        return dict(out=out, color=color, variance=variance, history=history, reason=reason)
