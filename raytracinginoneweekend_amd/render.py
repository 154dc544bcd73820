"""Render entry points over the C-ABI (the replacement for `cuda_impl`, src/main.cxx:18,114).

render_f32 / render_rgb8   synchronous, host numpy buffers (rt_render_f32 / rt_render_rgb8)
DeviceScene.render         async on a caller stream into a device buffer (rt_render_device),
                           the path bench.py times with inputs resident in HBM
render_aov / DeviceScene.render_aov   first-hit feature buffers for a denoiser or compositor
                           (rt_render_aov / rt_render_aov_device)
denoise / denoise_device   the edge-avoiding à-trous denoiser over those buffers (rt_denoise /
                           rt_denoise_device)
Preview / DeviceScene.preview   the whole denoised-preview loop on the device, one call per frame
                           (rt_preview_*)
MultiContext               row tiles over ranks (devices), gathered to rank 0 (rt_multi_*)
save_ppm                   app::save_to_file (src/main.cxx:87-101), rt_write_ppm
"""
import contextlib
import ctypes as C
import os

import numpy as np

from . import _abi as abi
from ._lib import check, lib
from .camera import Camera


def make_params(width, height, spp, max_depth=64, seed=1234, row_offset=0, row_stride=1, num_rows=0,
                full_frame=False, scalar_scene=False, fast_math=False, brute_force=False, cuda_compat=False,
                wavefront=False):
    flags = (abi.RT_FLAG_FULL_FRAME if full_frame else 0) | (abi.RT_FLAG_SCALAR_SCENE if scalar_scene else 0) \
        | (abi.RT_FLAG_FAST_MATH if fast_math else 0) | (abi.RT_FLAG_BRUTE_FORCE if brute_force else 0) \
        | (abi.RT_FLAG_CUDA_COMPAT if cuda_compat else 0) | (abi.RT_FLAG_WAVEFRONT if wavefront else 0)
    return abi.RtParams(width, height, spp, max_depth, seed, row_offset, row_stride, num_rows, flags)


def options(base=None, **fields):
    """An rt_options record: the library defaults (or `base`) with `fields` set; diag bits by name
    (ieee_roots=True, stats=True, ...; include/rt_api.h rt_diag) or as diag=<int>."""
    o = abi.RtOptions()
    if base is None:
        check(lib().rt_options_default(C.byref(o)))
    else:
        C.memmove(C.byref(o), C.byref(base), C.sizeof(o))
    for k, v in fields.items():
        if k in abi.RT_DIAG:
            o.diag = (o.diag | abi.RT_DIAG[k]) if v else (o.diag & ~abi.RT_DIAG[k])
        elif k in dict(abi.RtOptions._fields_) and k != "size":
            setattr(o, k, int(v))
        else:
            raise KeyError(f"rt_options has no field {k!r}")
    return o


def parse_options(text, base=None):
    """rt_options_parse: "key=value,..." over `base` (default: the library defaults)."""
    o = options(base)
    check(lib().rt_options_parse(text.encode(), C.byref(o)))
    return o


def default_options():
    """The process default (rt_get_default_options): library defaults with RT_OPTIONS applied."""
    o = abi.RtOptions()
    check(lib().rt_get_default_options(C.byref(o)))
    return o


def set_default_options(opt=None):
    """rt_set_default_options (None: the library defaults)."""
    check(lib().rt_set_default_options(C.byref(opt) if opt is not None else None))


@contextlib.contextmanager
def default_options_set(**fields):
    """Within the block, scenes created without explicit options (the synchronous renders,
    DeviceScene(), MultiContext()) use the current defaults with `fields` changed."""
    prev = default_options()
    set_default_options(options(prev, **fields))
    try:
        yield
    finally:
        set_default_options(prev)


def _scene_arrays(scene):
    if isinstance(scene, tuple):
        s, m = scene
    else:
        s, m = scene.arrays()
    return (np.ascontiguousarray(s, dtype=abi.SPHERE_DTYPE), np.ascontiguousarray(m, dtype=abi.MATERIAL_DTYPE))


def _cam(camera, params):
    if camera is None:
        return Camera.default(params.width, params.height).c
    return camera.c if isinstance(camera, Camera) else camera


def _out_rows(params):
    return params.height if params.flags & abi.RT_FLAG_FULL_FRAME else abi.rows_of(params)


def render_f32(scene, params, camera=None):
    """Averaged linear RGB (before gamma) as float32 (rows, width, 3); returns (image, stats)."""
    s, m = _scene_arrays(scene)
    out = np.zeros((_out_rows(params), params.width, 3), dtype=np.float32)
    st = abi.RtStats()
    check(lib().rt_render_f32(abi.ptr(s, C.POINTER(abi.RtSphere)), len(s), abi.ptr(m, C.POINTER(abi.RtMaterial)),
                              len(m), C.byref(_cam(camera, params)), C.byref(params),
                              abi.ptr(out, C.POINTER(C.c_float)), C.byref(st)))
    return out, st


def render_rgb8(scene, params, camera=None):
    """Gamma-corrected 8-bit RGB (rows, width, 3), as main.cxx:209-213 produces."""
    s, m = _scene_arrays(scene)
    out = np.zeros((_out_rows(params), params.width, 3), dtype=np.uint8)
    st = abi.RtStats()
    check(lib().rt_render_rgb8(abi.ptr(s, C.POINTER(abi.RtSphere)), len(s), abi.ptr(m, C.POINTER(abi.RtMaterial)),
                               len(m), C.byref(_cam(camera, params)), C.byref(params),
                               abi.ptr(out, C.POINTER(C.c_uint8)), C.byref(st)))
    return out, st


def aov_buffers(pointers, samples=0):
    """An rt_aov_buffers record from a dict plane name -> address (absent or 0: not wanted)."""
    unknown = set(pointers) - set(abi.AOV_PLANES)
    if unknown:
        raise KeyError(f"rt_aov_buffers has no plane {sorted(unknown)!r}")
    return abi.RtAovBuffers(C.sizeof(abi.RtAovBuffers), samples, *(pointers.get(n) or None for n in abi.AOV_PLANES))


def render_aov(scene, params, camera=None, samples=0, planes=tuple(abi.AOV_PLANES)):
    """First-hit feature buffers (rt_render_aov) of samples 0..samples-1 (0: every
    sample) of the pass `params` describes, as a dict plane name -> array: albedo and normal
    float32 (rows, width, 3), depth and alpha float32 (rows, width), sphere_id uint32 (rows,
    width). Full frame: rows the call does not render hold 0 (sphere_id: 0xffffffff)."""
    s, m = _scene_arrays(scene)
    rows, w = _out_rows(params), params.width
    out = {n: np.full((rows, w, ch) if ch > 1 else (rows, w), fill, dtype=dt)
           for n, (ch, dt, fill) in abi.AOV_PLANES.items() if n in planes}
    if len(out) != len(set(planes)):
        raise KeyError(f"unknown plane in {planes!r}")
    rec = aov_buffers({n: a.ctypes.data for n, a in out.items()}, samples)
    check(lib().rt_render_aov(abi.ptr(s, C.POINTER(abi.RtSphere)), len(s), abi.ptr(m, C.POINTER(abi.RtMaterial)),
                              len(m), C.byref(_cam(camera, params)), C.byref(params), C.byref(rec), None))
    return out


def denoise_params(width, height, base=None, demodulate=None, direct=None, **fields):
    """An rt_denoise_params record: the library defaults for the image (or a copy of `base`) with
    `fields` set (levels, sigma_color, sigma_normal, sigma_depth, sigma_albedo, flags);
    demodulate / direct set or clear RT_DENOISE_DEMODULATE / RT_DENOISE_DIRECT."""
    p = abi.RtDenoiseParams()
    if base is None:
        check(lib().rt_denoise_params_default(width, height, C.byref(p)))
    else:
        C.memmove(C.byref(p), C.byref(base), C.sizeof(p))
        p.width, p.height = width, height
    names = dict(abi.RtDenoiseParams._fields_)
    for k, v in fields.items():
        if k not in names or k in ("size", "width", "height"):
            raise KeyError(f"rt_denoise_params has no field {k!r}")
        setattr(p, k, v)
    for bit, on in ((abi.RT_DENOISE_DEMODULATE, demodulate), (abi.RT_DENOISE_DIRECT, direct)):
        if on is not None:
            p.flags = (p.flags | bit) if on else (p.flags & ~bit)
    return p


def denoise_buffers(pointers):
    """An rt_denoise_buffers record from a dict plane name (beauty, albedo, normal, depth, out,
    scratch) -> address (absent or 0: not given)."""
    unknown = set(pointers) - set(abi.DENOISE_PLANES)
    if unknown:
        raise KeyError(f"rt_denoise_buffers has no plane {sorted(unknown)!r}")
    return abi.RtDenoiseBuffers(C.sizeof(abi.RtDenoiseBuffers), *(pointers.get(n) or None for n in abi.DENOISE_PLANES))


def denoise(beauty, albedo=None, normal=None, depth=None, params=None, stats=None, **fields):
    """rt_denoise: the à-trous filter of a float32 (h, w, 3) beauty image guided by
    the planes of render_aov that are given (albedo and normal (h, w, 3), depth (h, w)); returns
    float32 (h, w, 3). params: an rt_denoise_params record (default: the library's for this size);
    `fields` as denoise_params takes them. stats: an optional RtStats to fill."""
    planes = {"beauty": beauty, "albedo": albedo, "normal": normal, "depth": depth}
    if beauty is None or np.ndim(beauty) != 3 or np.shape(beauty)[2] != 3:
        raise ValueError(f"beauty must be float32 (h, w, 3), not {np.shape(beauty)}")
    h, w = np.shape(beauty)[:2]
    host = {}
    for n, a in planes.items():
        if a is None:
            continue
        want = (h, w, 3) if abi.DENOISE_PLANES[n] == 3 else (h, w)
        a = np.asarray(a)
        if a.dtype != np.float32 or a.shape != want:
            raise ValueError(f"{n} must be float32 {want}, not {a.dtype} {a.shape}")
        host[n] = np.ascontiguousarray(a)
    p = denoise_params(w, h, base=params, **fields)
    out = np.zeros((h, w, 3), dtype=np.float32)
    rec = denoise_buffers({**{n: a.ctypes.data for n, a in host.items()}, "out": out.ctypes.data})
    check(lib().rt_denoise(C.byref(p), C.byref(rec), C.byref(stats) if stats is not None else None))
    return out


def denoise_device(pointers, params, stream=None):
    """Enqueue rt_denoise_device on `stream`: `pointers` is a dict plane name (beauty, albedo,
    normal, depth, out, scratch) -> device address on the current device, `params` an
    rt_denoise_params record (denoise_params). One launch per level, no host synchronisation."""
    rec = denoise_buffers(pointers)
    check(lib().rt_denoise_device(C.byref(params), C.byref(rec), C.c_void_p(stream or 0)))


def render_var(scene, params, camera=None):
    """rt_render_var: the beauty as render_f32 returns it, float32 (rows, width,
    3), and the variance of each pixel's mean luminance, float32 (rows, width); returns (rgb, var,
    stats). Full frame: rows the call does not render hold 0."""
    s, m = _scene_arrays(scene)
    rows, w = _out_rows(params), params.width
    rgb = np.zeros((rows, w, 3), dtype=np.float32)
    var = np.zeros((rows, w), dtype=np.float32)
    st = abi.RtStats()
    check(lib().rt_render_var(abi.ptr(s, C.POINTER(abi.RtSphere)), len(s), abi.ptr(m, C.POINTER(abi.RtMaterial)),
                              len(m), C.byref(_cam(camera, params)), C.byref(params),
                              abi.ptr(rgb, C.POINTER(C.c_float)), abi.ptr(var, C.POINTER(C.c_float)), C.byref(st)))
    return rgb, var, st


def denoise_var_params(width, height, base=None, var_floor=None, direct=None, **fields):
    """The records of a variance-guided denoise: (rt_denoise_params, rt_denoise_var_buffers) with
    the library defaults for the image (rt_denoise_var_params_default; the params a copy of `base`
    if given), then `fields` set as denoise_params sets them and var_floor, if given."""
    p, v = abi.RtDenoiseParams(), abi.RtDenoiseVarBuffers()
    check(lib().rt_denoise_var_params_default(width, height, C.byref(p), C.byref(v)))
    if base is not None:
        C.memmove(C.byref(p), C.byref(base), C.sizeof(p))
        p.width, p.height = width, height
    names = dict(abi.RtDenoiseParams._fields_)
    for k, val in fields.items():
        if k not in names or k in ("size", "width", "height"):
            raise KeyError(f"rt_denoise_params has no field {k!r}")
        setattr(p, k, val)
    if direct is not None:
        p.flags = (p.flags | abi.RT_DENOISE_DIRECT) if direct else (p.flags & ~abi.RT_DENOISE_DIRECT)
    if var_floor is not None:
        v.var_floor = var_floor
    return p, v


def denoise_var_buffers(pointers, var_floor):
    """An rt_denoise_var_buffers record from a dict plane name (variance, variance_out,
    var_scratch) -> address (absent or 0: not given)."""
    unknown = set(pointers) - set(abi.DENOISE_VAR_PLANES)
    if unknown:
        raise KeyError(f"rt_denoise_var_buffers has no plane {sorted(unknown)!r}")
    return abi.RtDenoiseVarBuffers(C.sizeof(abi.RtDenoiseVarBuffers), var_floor,
                                   *(pointers.get(n) or None for n in abi.DENOISE_VAR_PLANES))


def denoise_var(beauty, variance, albedo=None, normal=None, depth=None, variance_out=False, params=None,
                stats=None, **fields):
    """rt_denoise_var: the à-trous filter of `beauty` with its colour term steered
    per pixel by `variance` (float32 (h, w), as render_var returns it); the guides as denoise takes
    them. Returns float32 (h, w, 3), or (image, variance after the last level) with variance_out.
    `fields` as denoise_var_params takes them (var_floor among them)."""
    planes = {"beauty": beauty, "albedo": albedo, "normal": normal, "depth": depth, "variance": variance}
    if beauty is None or np.ndim(beauty) != 3 or np.shape(beauty)[2] != 3:
        raise ValueError(f"beauty must be float32 (h, w, 3), not {np.shape(beauty)}")
    if variance is None:
        raise ValueError("variance must be float32 (h, w)")
    h, w = np.shape(beauty)[:2]
    host = {}
    for n, a in planes.items():
        if a is None:
            continue
        want = (h, w, 3) if n != "variance" and abi.DENOISE_PLANES[n] == 3 else (h, w)
        a = np.asarray(a)
        if a.dtype != np.float32 or a.shape != want:
            raise ValueError(f"{n} must be float32 {want}, not {a.dtype} {a.shape}")
        host[n] = np.ascontiguousarray(a)
    p, v = denoise_var_params(w, h, base=params, **fields)
    out = np.zeros((h, w, 3), dtype=np.float32)
    vout = np.zeros((h, w), dtype=np.float32) if variance_out else None
    rec = denoise_buffers({**{n: a.ctypes.data for n, a in host.items() if n != "variance"}, "out": out.ctypes.data})
    vrec = denoise_var_buffers({"variance": host["variance"].ctypes.data,
                                "variance_out": vout.ctypes.data if variance_out else 0}, v.var_floor)
    check(lib().rt_denoise_var(C.byref(p), C.byref(rec), C.byref(vrec), C.byref(stats) if stats is not None else None))
    return (out, vout) if variance_out else out


def denoise_var_device(pointers, params, var_record, stream=None):
    """Enqueue rt_denoise_var_device on `stream`: `pointers` as denoise_device takes them, `params`
    an rt_denoise_params record, `var_record` an rt_denoise_var_buffers record of device addresses
    (denoise_var_buffers). One launch per level, no host synchronisation."""
    rec = denoise_buffers(pointers)
    check(lib().rt_denoise_var_device(C.byref(params), C.byref(rec), C.byref(var_record), C.c_void_p(stream or 0)))


def temporal_params(width, height, base=None, **fields):
    """An rt_temporal_params record: the library defaults for the image (or a copy of `base`) with
    `fields` set (alpha_min, max_history, normal_tol, depth_tol, flags)."""
    p = abi.RtTemporalParams()
    if base is None:
        check(lib().rt_temporal_params_default(width, height, C.byref(p)))
    else:
        C.memmove(C.byref(p), C.byref(base), C.sizeof(p))
        p.width, p.height = width, height
    names = dict(abi.RtTemporalParams._fields_)
    for k, v in fields.items():
        if k not in names or k in ("size", "width", "height"):
            raise KeyError(f"rt_temporal_params has no field {k!r}")
        setattr(p, k, v)
    return p


def temporal_buffers(pointers):
    """An rt_temporal_buffers record from a dict plane name (abi.TEMPORAL_PLANES: the current
    frame's beauty, variance, normal, depth, alpha, sphere_id; prev_color, prev_variance,
    prev_history, prev_normal, prev_depth, prev_sphere_id; out_color, out_variance, out_history)
    -> address (absent or 0: not given)."""
    unknown = set(pointers) - set(abi.TEMPORAL_PLANES)
    if unknown:
        raise KeyError(f"rt_temporal_buffers has no plane {sorted(unknown)!r}")
    return abi.RtTemporalBuffers(C.sizeof(abi.RtTemporalBuffers), *(pointers.get(n) or None for n in abi.TEMPORAL_PLANES))


def _cam_record(camera):
    return camera.c if isinstance(camera, Camera) else camera


def reproject_basis(camera):
    """rt_reproject_basis: the projection record {A, B, G, o'} of a previous camera (DESIGN.md
    §4.11) as float32 (12,). Host-only."""
    out = np.zeros(12, dtype=np.float32)
    check(lib().rt_reproject_basis(C.byref(_cam_record(camera)), abi.ptr(out, C.POINTER(C.c_float))))
    return out


def sphere_table(scene):
    """The [n][4] float32 array {cx, cy, cz, radius} of a scene's spheres, row i = sphere i: what
    rt_temporal_motion takes as `centres` / `prev_centres` and a DeviceScene keeps."""
    s, _ = _scene_arrays(scene)
    t = np.empty((len(s), 4), dtype=np.float32)
    t[:, :3] = s["center"]
    t[:, 3] = s["radius"]
    return t


def temporal_motion_record(centres, prev_centres, n_spheres):
    """An rt_temporal_motion_t record from two table addresses (0 or None: not given)."""
    return abi.RtTemporalMotion(C.sizeof(abi.RtTemporalMotion), n_spheres, centres or None, prev_centres or None)


def temporal_clip(radius=None, gamma=None, **fields):
    """An rt_temporal_clip_t record: the library defaults with radius, gamma and
    `fields` (flags) set."""
    c = abi.RtTemporalClip()
    check(lib().rt_temporal_clip_default(C.byref(c)))
    for k, v in dict(radius=radius, gamma=gamma).items():
        if v is not None:
            setattr(c, k, v)
    for k, v in fields.items():
        if k != "flags":
            raise KeyError(f"rt_temporal_clip_t has no field {k!r} to set")
        setattr(c, k, v)
    return c


def temporal_device(pointers, params, camera, prev_camera, stream=None, motion=None, clip=None):
    """Enqueue rt_temporal_device on `stream`: `pointers` is a dict plane name -> device address on
    the current device (temporal_buffers; the prev_ planes all absent: no history yet), `params` an
    rt_temporal_params record, `camera` and `prev_camera` the two frames' cameras (prev_camera may be
    None without history). One launch, no host synchronisation. motion: (centres address,
    prev_centres address, n_spheres) of two device tables: rt_temporal_motion_device, the stage with
    object motion. clip: an rt_temporal_clip_t record (temporal_clip):
    rt_temporal_clip_device, the stage with the history clamp, with or without motion."""
    rec = temporal_buffers(pointers)
    cams = (C.byref(_cam_record(camera)), C.byref(_cam_record(prev_camera)) if prev_camera is not None else None)
    if clip is not None:
        m = temporal_motion_record(*motion) if motion is not None else None
        check(lib().rt_temporal_clip_device(C.byref(params), *cams, C.byref(rec), C.byref(m) if m is not None else None,
                                            C.byref(clip), C.c_void_p(stream or 0)))
        return
    if motion is not None:
        m = temporal_motion_record(*motion)
        check(lib().rt_temporal_motion_device(C.byref(params), *cams, C.byref(rec), C.byref(m), C.c_void_p(stream or 0)))
        return
    check(lib().rt_temporal_device(C.byref(params), *cams, C.byref(rec), C.c_void_p(stream or 0)))


_TEMPORAL_CUR = ("beauty", "variance", "normal", "depth", "alpha", "sphere_id")
_TEMPORAL_PREV = ("color", "variance", "history", "normal", "depth", "sphere_id")


def temporal(cur, prev, camera, prev_camera, params=None, stats=None, motion=None, clip=None, **fields):
    """rt_temporal: the previous frame's history reprojected into the current
    frame and blended. cur: dict of the current frame's planes (beauty and variance as render_var
    returns them; normal, depth, alpha, sphere_id as render_aov does); prev: dict of the previous
    frame's (color, variance, history as this call returned them, or color after a filter level;
    normal, depth, sphere_id of that frame), or None: no history yet. Returns (color float32 (h, w,
    3), variance float32 (h, w), history float32 (h, w)). params: an rt_temporal_params record
    (default: the library's for this size); `fields` as temporal_params takes them. motion:
    (centres, prev_centres), two float32 (n, 4) tables as sphere_table makes them: rt_temporal_motion,
    the stage with object motion. clip: an rt_temporal_clip_t record (temporal_clip):
    rt_temporal_clip, the stage with the history clamp, with or without motion."""
    if set(cur) != set(_TEMPORAL_CUR):
        raise KeyError(f"cur must hold exactly the planes {_TEMPORAL_CUR}, not {sorted(cur)}")
    if prev is not None and set(prev) != set(_TEMPORAL_PREV):
        raise KeyError(f"prev must hold exactly the planes {_TEMPORAL_PREV}, not {sorted(prev)}")
    if np.ndim(cur["beauty"]) != 3 or np.shape(cur["beauty"])[2] != 3:
        raise ValueError(f"beauty must be float32 (h, w, 3), not {np.shape(cur['beauty'])}")
    h, w = np.shape(cur["beauty"])[:2]
    host = {}
    for n, a in [(n, cur[n]) for n in _TEMPORAL_CUR] + [("prev_" + n, prev[n]) for n in _TEMPORAL_PREV if prev is not None]:
        ch, dt = abi.TEMPORAL_PLANES[n]
        want = (h, w, 3) if ch == 3 else (h, w)
        a = np.asarray(a)
        if a.dtype != dt or a.shape != want:
            raise ValueError(f"{n} must be {np.dtype(dt).name} {want}, not {a.dtype} {a.shape}")
        host[n] = np.ascontiguousarray(a)
    p = temporal_params(w, h, base=params, **fields)
    out = {n: np.zeros((h, w, 3) if abi.TEMPORAL_PLANES[n][0] == 3 else (h, w), dtype=np.float32)
           for n in ("out_color", "out_variance", "out_history")}
    rec = temporal_buffers({n: a.ctypes.data for n, a in {**host, **out}.items()})
    cams = (C.byref(_cam_record(camera)), C.byref(_cam_record(prev_camera)) if prev_camera is not None else None)
    st = C.byref(stats) if stats is not None else None
    m = None
    if motion is not None:
        tabs = [np.ascontiguousarray(t) for t in motion]
        if len(tabs) != 2 or any(t.dtype != np.float32 or t.ndim != 2 or t.shape != (len(tabs[0]), 4) for t in tabs):
            raise ValueError("motion must be two float32 (n, 4) tables of one length")
        m = temporal_motion_record(tabs[0].ctypes.data if len(tabs[0]) else None,
                                   tabs[1].ctypes.data if len(tabs[1]) else None, len(tabs[0]))
    if clip is not None:
        check(lib().rt_temporal_clip(C.byref(p), *cams, C.byref(rec), C.byref(m) if m is not None else None,
                                     C.byref(clip), st))
    elif m is not None:
        check(lib().rt_temporal_motion(C.byref(p), *cams, C.byref(rec), C.byref(m), st))
    else:
        check(lib().rt_temporal(C.byref(p), *cams, C.byref(rec), st))
    return out["out_color"], out["out_variance"], out["out_history"]


def upsample_params(width, height, lo_width, lo_height, base=None, **fields):
    """An rt_upsample_params record: the library defaults for the two image sizes
    (or a copy of `base`) with `fields` set (normal_tol, depth_tol, flags)."""
    p = abi.RtUpsampleParams()
    if base is None:
        check(lib().rt_upsample_params_default(width, height, lo_width, lo_height, C.byref(p)))
    else:
        C.memmove(C.byref(p), C.byref(base), C.sizeof(p))
        p.width, p.height, p.lo_width, p.lo_height = width, height, lo_width, lo_height
    for k, v in fields.items():
        if k not in ("normal_tol", "depth_tol", "flags"):
            raise KeyError(f"rt_upsample_params has no field {k!r} to set")
        setattr(p, k, v)
    return p


def upsample_buffers(pointers):
    """An rt_upsample_buffers record from a dict plane name (abi.UPSAMPLE_PLANES: lo_color,
    lo_variance, lo_normal, lo_depth, lo_sphere_id; normal, depth, alpha, sphere_id; out_color,
    out_variance) -> address (absent or 0: not given)."""
    unknown = set(pointers) - set(abi.UPSAMPLE_PLANES)
    if unknown:
        raise KeyError(f"rt_upsample_buffers has no plane {sorted(unknown)!r}")
    return abi.RtUpsampleBuffers(C.sizeof(abi.RtUpsampleBuffers), *(pointers.get(n) or None for n in abi.UPSAMPLE_PLANES))


def upsample_device(pointers, params, stream=None):
    """Enqueue rt_upsample_device on `stream`: `pointers` is a dict plane name -> device address on
    the current device (upsample_buffers), `params` an rt_upsample_params record. One launch, no host
    synchronisation."""
    rec = upsample_buffers(pointers)
    check(lib().rt_upsample_device(C.byref(params), C.byref(rec), C.c_void_p(stream or 0)))


_UPSAMPLE_LO = ("color", "normal", "depth", "sphere_id")
_UPSAMPLE_HI = ("normal", "depth", "alpha", "sphere_id")


def upsample(lo, guides, params=None, stats=None, **fields):
    """rt_upsample: a low-resolution image brought up to the size of `guides` by a
    joint-bilateral upsample. lo: dict of the low-resolution planes (color float32 (lh, lw, 3);
    normal, depth, sphere_id as render_aov returns them at that size; optionally variance (lh, lw));
    guides: dict of the output-size planes normal, depth, alpha, sphere_id (render_aov at the output
    size, same camera). Returns color float32 (h, w, 3), or (color, variance) when lo holds a
    variance. params: an rt_upsample_params record (default: the library's); `fields` as
    upsample_params takes them."""
    with_var = "variance" in lo
    if set(lo) - {"variance"} != set(_UPSAMPLE_LO):
        raise KeyError(f"lo must hold the planes {_UPSAMPLE_LO} (and optionally variance), not {sorted(lo)}")
    if set(guides) != set(_UPSAMPLE_HI):
        raise KeyError(f"guides must hold exactly the planes {_UPSAMPLE_HI}, not {sorted(guides)}")
    if np.ndim(lo["color"]) != 3 or np.shape(lo["color"])[2] != 3:
        raise ValueError(f"lo color must be float32 (lh, lw, 3), not {np.shape(lo['color'])}")
    if np.ndim(guides["normal"]) != 3 or np.shape(guides["normal"])[2] != 3:
        raise ValueError(f"normal must be float32 (h, w, 3), not {np.shape(guides['normal'])}")
    lh, lw = np.shape(lo["color"])[:2]
    h, w = np.shape(guides["normal"])[:2]
    host = {}
    for n, a, (hh, ww) in ([("lo_" + n, lo[n], (lh, lw)) for n in lo] + [(n, guides[n], (h, w)) for n in _UPSAMPLE_HI]):
        ch, dt = abi.UPSAMPLE_PLANES[n]
        want = (hh, ww, 3) if ch == 3 else (hh, ww)
        a = np.asarray(a)
        if a.dtype != dt or a.shape != want:
            raise ValueError(f"{n} must be {np.dtype(dt).name} {want}, not {a.dtype} {a.shape}")
        host[n] = np.ascontiguousarray(a)
    p = upsample_params(w, h, lw, lh, base=params, **fields)
    out = {"out_color": np.zeros((h, w, 3), dtype=np.float32)}
    if with_var:
        out["out_variance"] = np.zeros((h, w), dtype=np.float32)
    rec = upsample_buffers({n: a.ctypes.data for n, a in {**host, **out}.items()})
    check(lib().rt_upsample(C.byref(p), C.byref(rec), C.byref(stats) if stats is not None else None))
    return (out["out_color"], out["out_variance"]) if with_var else out["out_color"]


def preview_upscale(params, out_width, out_height, **fields):
    """An rt_preview_upscale record for a session of `params` (an rt_preview_params
    record) shown at out_width x out_height: the library defaults with `fields` set (guide_samples,
    normal_tol, depth_tol)."""
    u = abi.RtPreviewUpscale()
    check(lib().rt_preview_upscale_default(C.byref(params), out_width, out_height, C.byref(u)))
    for k, v in fields.items():
        if k not in ("guide_samples", "normal_tol", "depth_tol"):
            raise KeyError(f"rt_preview_upscale has no field {k!r} to set")
        setattr(u, k, v)
    return u


def preview_params(width, height, spp, base=None, demodulate=None, feedback=None, temporal=None, denoise=None,
                   **fields):
    """An rt_preview_params record: the library defaults for the frame (or a copy
    of `base`) with `fields` set (max_depth, flags, var_floor); demodulate / feedback / temporal set
    or clear RT_PREVIEW_DEMODULATE / RT_PREVIEW_FEEDBACK / the temporal stage (temporal=False:
    RT_PREVIEW_NO_TEMPORAL), or temporal is a dict of rt_temporal_params fields (temporal_params);
    denoise: a dict of rt_denoise_params fields (denoise_var_params; direct among them)."""
    p = abi.RtPreviewParams()
    if base is None:
        check(lib().rt_preview_params_default(width, height, spp, C.byref(p)))
    else:
        C.memmove(C.byref(p), C.byref(base), C.sizeof(p))
        p.width = p.temporal.width = p.denoise.width = width
        p.height = p.temporal.height = p.denoise.height = height
        p.spp = spp
    for k, v in fields.items():
        if k not in ("max_depth", "flags", "var_floor"):
            raise KeyError(f"rt_preview_params has no field {k!r} to set")
        setattr(p, k, v)
    if isinstance(temporal, dict):
        p.temporal = temporal_params(width, height, base=p.temporal, **temporal)
        temporal = True
    if denoise is not None:
        p.denoise = denoise_var_params(width, height, base=p.denoise, **denoise)[0]
    for bit, on in ((abi.RT_PREVIEW_DEMODULATE, demodulate), (abi.RT_PREVIEW_FEEDBACK, feedback),
                    (abi.RT_PREVIEW_NO_TEMPORAL, None if temporal is None else not temporal)):
        if on is not None:
            p.flags = (p.flags | bit) if on else (p.flags & ~bit)
    return p


class Preview:
    """A preview session on a DeviceScene (rt_preview_create): the loop render ->
    feature buffers -> temporal accumulation -> variance-guided filter -> epilogue with every plane
    and the history kept on the device, one call per frame. Close it before its scene. upscale: an
    rt_preview_upscale record (preview_upscale) makes it an upscaled session
    (rt_preview_create_upscaled): the loop runs at `params`' size, and frame()
    writes images of the record's output size."""

    def __init__(self, device_scene, params, upscale=None):
        h = C.c_void_p()
        sc = device_scene.handle if device_scene is not None else None
        if upscale is None:
            check(lib().rt_preview_create(sc, C.byref(params), C.byref(h)))
        else:
            check(lib().rt_preview_create_upscaled(sc, C.byref(params), C.byref(upscale), C.byref(h)))
        self.handle = h
        self.scene = device_scene  # (kept alive as long as the session)
        self.width, self.height = params.width, params.height
        self.out_width, self.out_height = ((params.width, params.height) if upscale is None
                                           else (upscale.out_width, upscale.out_height))

    def frame(self, camera, seed, rgb_ptr=None, rgb8_ptr=None, stream=None):
        """Enqueue one frame on `stream`: the denoised linear image into device address rgb_ptr
        (float32 (h, w, 3)) and / or its gamma-corrected texels into rgb8_ptr (uint8 (h, w, 3))."""
        check(lib().rt_preview_frame_device(self.handle, C.byref(_cam_record(camera)) if camera is not None else None,
                                            seed, C.c_void_p(rgb_ptr or 0), C.c_void_p(rgb8_ptr or 0),
                                            C.c_void_p(stream or 0)))

    def refine(self, camera, seed, total_spp, n_samples, rgb_ptr=None, rgb8_ptr=None, stream=None):
        """rt_preview_refine_device: the view at rest. Enqueue the next n_samples samples of the
        total_spp-sample frame of (camera, seed) and store the estimate, filtered with its own
        variance until the frame is complete and exact from then on."""
        check(lib().rt_preview_refine_device(self.handle, C.byref(_cam_record(camera)) if camera is not None else None,
                                             seed, total_spp, n_samples, C.c_void_p(rgb_ptr or 0), C.c_void_p(rgb8_ptr or 0),
                                             C.c_void_p(stream or 0)))

    def refine_info(self):
        """rt_preview_refine_info: (samples done, total) of the refinement in progress, (0, 0): none."""
        done, total = C.c_uint32(0), C.c_uint32(0)
        check(lib().rt_preview_refine_info(self.handle, C.byref(done), C.byref(total)))
        return done.value, total.value

    def reset(self):
        """The next frame has no history."""
        check(lib().rt_preview_reset(self.handle))

    def set_clip(self, clip):
        """rt_preview_set_clip: from the next frame on the temporal stage clamps the history with
        `clip` (an rt_temporal_clip_t record, temporal_clip); None turns it off."""
        check(lib().rt_preview_set_clip(self.handle, C.byref(clip) if clip is not None else None))

    def planes(self):
        """rt_preview_planes: what the last enqueued frame wrote, as a dict plane name
        (abi.PREVIEW_PLANES) -> device address (None: not there), and 'frames'."""
        r = abi.RtPreviewPlanes()
        check(lib().rt_preview_planes(self.handle, C.byref(r)))
        return {"frames": r.frames, **{n: getattr(r, n) for n in abi.PREVIEW_PLANES}}

    def output(self):
        """rt_preview_output: what an upscaled session's last frame wrote at the output size, as a
        dict plane name (abi.PREVIEW_OUTPUT_PLANES) -> device address (None: not there), and
        'width', 'height'. An ordinary session raises RtError."""
        r = abi.RtPreviewOutput()
        check(lib().rt_preview_output(self.handle, C.byref(r)))
        return {"width": r.width, "height": r.height, **{n: getattr(r, n) for n in abi.PREVIEW_OUTPUT_PLANES}}

    def usage(self):
        """rt_preview_usage: the bytes of the session's device allocation."""
        n = C.c_uint64(0)
        check(lib().rt_preview_usage(self.handle, C.byref(n)))
        return n.value

    def close(self):
        if self.handle:
            lib().rt_preview_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def progressive_outputs(rgb_ptr=None, variance_ptr=None, rgb8_ptr=None, noisy_ptr=None, noise_tau=0.0):
    """An rt_progressive_outputs record from device addresses (None: that plane is not wanted)."""
    return abi.RtProgressiveOutputs(C.sizeof(abi.RtProgressiveOutputs), noise_tau, rgb_ptr or None, variance_ptr or None,
                                    rgb8_ptr or None, noisy_ptr or None)


def progressive_window(spp, done, n_samples):
    """rt_progressive_window: the samples a step of n_samples takes after `done` of an spp-sample
    frame (the Step rule of include/rt_api.h); raises RtError where the step would be refused."""
    m = C.c_uint32(0)
    check(lib().rt_progressive_window(spp, done, n_samples, C.byref(m)))
    return m.value


def progressive_blob_check(blob, params, camera):
    """rt_progressive_blob_check: rt_progressive_load's check of a checkpoint against a params /
    camera pair, without a session; the blob's info as a dict."""
    info = abi.RtProgressiveInfo()
    buf = (C.c_char * len(blob)).from_buffer_copy(blob) if len(blob) else None
    check(lib().rt_progressive_blob_check(buf, len(blob), C.byref(params) if params is not None else None,
                                          C.byref(_cam_record(camera)) if camera is not None else None, C.byref(info)))
    return {n: getattr(info, n) for n in ("done", "spp", "n_pixels", "state_bytes", "device_bytes")}


class Progressive:
    """A progressive session on a DeviceScene (rt_progressive_create): the frame
    that `params` describes (params.spp is the whole frame's sample count), rendered in sample
    windows whose sums stay on the device; after the last window the outputs hold the bits of
    render_var / render for the same arguments. Close it before its scene."""

    def __init__(self, device_scene, camera, params):
        h = C.c_void_p()
        sc = device_scene.handle if device_scene is not None else None
        cam = C.byref(_cam_record(camera)) if camera is not None else None
        check(lib().rt_progressive_create(sc, cam, C.byref(params) if params is not None else None, C.byref(h)))
        self.handle = h
        self.scene = device_scene  # (kept alive as long as the session)

    def step(self, n_samples, rgb_ptr=None, variance_ptr=None, rgb8_ptr=None, noisy_ptr=None, noise_tau=0.0, stream=None,
             segments=None, outputs=None):
        """Enqueue the frame's next n_samples samples on `stream`, then (when an output is given)
        the estimate after them: linear float32 into rgb_ptr, the variance of the mean luminance
        into variance_ptr, texels into rgb8_ptr, the number of pixels noisier than noise_tau into
        the device word noisy_ptr (device addresses; `outputs`: a ready record instead)."""
        if outputs is None and (rgb_ptr or variance_ptr or rgb8_ptr or noisy_ptr):
            outputs = progressive_outputs(rgb_ptr, variance_ptr, rgb8_ptr, noisy_ptr, noise_tau)
        check(lib().rt_progressive_step_device(self.handle, n_samples, C.byref(outputs) if outputs is not None else None,
                                               C.c_void_p(stream or 0), C.c_void_p(segments) if segments else None))

    def info(self):
        """rt_progressive_info as a dict: done, spp, n_pixels, state_bytes, device_bytes."""
        r = abi.RtProgressiveInfo()
        check(lib().rt_progressive_info(self.handle, C.byref(r)))
        return {n: getattr(r, n) for n in ("done", "spp", "n_pixels", "state_bytes", "device_bytes")}

    def reset(self, camera=None, seed=None):
        """The frame starts again (done = 0), with another camera and / or seed when given."""
        check(lib().rt_progressive_reset(self.handle, C.byref(_cam_record(camera)) if camera is not None else None,
                                         C.byref(C.c_uint64(seed)) if seed is not None else None))

    def save(self):
        """rt_progressive_save: the session's state as bytes (waits for its enqueued work)."""
        buf = C.create_string_buffer(self.info()["state_bytes"])
        check(lib().rt_progressive_save(self.handle, buf, len(buf)))
        return buf.raw

    def load(self, blob):
        """rt_progressive_load: continue from a checkpoint of a session with the same arguments."""
        buf = (C.c_char * len(blob)).from_buffer_copy(blob) if len(blob) else None
        check(lib().rt_progressive_load(self.handle, buf, len(blob)))

    def close(self):
        if self.handle:
            lib().rt_progressive_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def adaptive_params(noise_tau, max_noisy=0, min_samples=4):
    """An rt_adaptive_params record: a block retires once it holds min_samples samples and at most
    max_noisy of its 64 pixels have var > noise_tau^2 L^2."""
    return abi.RtAdaptiveParams(C.sizeof(abi.RtAdaptiveParams), noise_tau, max_noisy, min_samples)


def adaptive_outputs(rgb_ptr=None, variance_ptr=None, rgb8_ptr=None, samples_ptr=None, noisy_ptr=None):
    """An rt_adaptive_outputs record from device addresses (None: that plane is not wanted)."""
    return abi.RtAdaptiveOutputs(C.sizeof(abi.RtAdaptiveOutputs), 0, rgb_ptr or None, variance_ptr or None, rgb8_ptr or None,
                                 samples_ptr or None, noisy_ptr or None)


def block_compact_device(src_perm_ptr, n_blocks, class_counts, active_ptr, out_perm_ptr, counts_ptr, stream=None):
    """rt_block_compact_device: the adaptive session's compaction kernel alone, on device addresses:
    the entries of the dealing order at src_perm_ptr whose block's word at active_ptr is nonzero, in
    order, to out_perm_ptr; {kept, kept lead, kept middle, kept sky} to counts_ptr."""
    cc = (C.c_uint32 * 3)(*class_counts) if class_counts is not None else None
    check(lib().rt_block_compact_device(C.c_void_p(src_perm_ptr or 0), n_blocks, cc, C.c_void_p(active_ptr or 0),
                                        C.c_void_p(out_perm_ptr or 0), C.c_void_p(counts_ptr or 0), C.c_void_p(stream or 0)))


class Adaptive:
    """An adaptive session on a DeviceScene (rt_adaptive_create): the frame that
    `params` describes in sample windows, like Progressive, but a 64-pixel block whose noise estimate
    has fallen under the rule of `adaptive` (adaptive_params) is rendered no further. params.spp is the
    cap of every pixel's sample count. Close it before its scene."""

    def __init__(self, device_scene, camera, params, adaptive):
        h = C.c_void_p()
        sc = device_scene.handle if device_scene is not None else None
        cam = C.byref(_cam_record(camera)) if camera is not None else None
        check(lib().rt_adaptive_create(sc, cam, C.byref(params) if params is not None else None,
                                       C.byref(adaptive) if adaptive is not None else None, C.byref(h)))
        self.handle = h
        self.scene = device_scene  # (kept alive as long as the session)

    def step(self, n_samples, rgb_ptr=None, variance_ptr=None, rgb8_ptr=None, samples_ptr=None, noisy_ptr=None, stream=None,
             segments=None, outputs=None):
        """Enqueue the next n_samples samples of the blocks still active on `stream`, then the
        estimate of the whole frame (every block after its own sample count) into the planes given,
        the retire rule and the next step's block list. Waits for the previous step's block counts."""
        if outputs is None and (rgb_ptr or variance_ptr or rgb8_ptr or samples_ptr or noisy_ptr):
            outputs = adaptive_outputs(rgb_ptr, variance_ptr, rgb8_ptr, samples_ptr, noisy_ptr)
        check(lib().rt_adaptive_step_device(self.handle, n_samples, C.byref(outputs) if outputs is not None else None,
                                            C.c_void_p(stream or 0), C.c_void_p(segments) if segments else None))

    def info(self):
        """rt_adaptive_info as a dict: done, spp, n_blocks, active_blocks, finished, n_pixels,
        samples_rendered, device_bytes (waits for the last step's block counts)."""
        r = abi.RtAdaptiveInfo()
        check(lib().rt_adaptive_info(self.handle, C.byref(r)))
        return {n: getattr(r, n) for n in ("done", "spp", "n_blocks", "active_blocks", "finished", "n_pixels",
                                           "samples_rendered", "device_bytes")}

    def blocks(self):
        """rt_adaptive_blocks: the samples folded into every 64-pixel block, in natural block order
        (uint32 array; synchronous)."""
        n = self.info()["n_blocks"]
        out = np.zeros(n, dtype=np.uint32)
        check(lib().rt_adaptive_blocks(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return out

    def reset(self, camera=None, seed=None):
        """The frame starts again (every block active, no sample), with another camera and / or seed when given."""
        check(lib().rt_adaptive_reset(self.handle, C.byref(_cam_record(camera)) if camera is not None else None,
                                      C.byref(C.c_uint64(seed)) if seed is not None else None))

    def close(self):
        if self.handle:
            lib().rt_adaptive_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def preview_split_device(width, height, beauty, variance, albedo, illumination, variance_out, stream=None):
    """Enqueue rt_preview_split_device (device addresses): illumination = beauty / albedo',
    variance_out = variance / luminance(albedo')^2."""
    check(lib().rt_preview_split_device(width, height, C.c_void_p(beauty), C.c_void_p(variance), C.c_void_p(albedo),
                                        C.c_void_p(illumination), C.c_void_p(variance_out), C.c_void_p(stream or 0)))


def preview_merge_device(width, height, filtered, albedo=None, rgb_ptr=None, rgb8_ptr=None, stream=None):
    """Enqueue rt_preview_merge_device (device addresses): filtered (x albedo' when albedo is given)
    as float32 into rgb_ptr and / or as gamma-corrected texels into rgb8_ptr."""
    check(lib().rt_preview_merge_device(width, height, C.c_void_p(filtered), C.c_void_p(albedo or 0),
                                        C.c_void_p(rgb_ptr or 0), C.c_void_p(rgb8_ptr or 0), C.c_void_p(stream or 0)))


def tile_order(scene, params, camera=None):
    """rt_tile_order: the pass's 64-pixel blocks in dealing order as
    (perm, n_lead, n_sky); perm is empty when the pass keeps the natural order."""
    s, m = _scene_arrays(scene)
    nb, nl, ns = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    args = (abi.ptr(s, C.POINTER(abi.RtSphere)), len(s), abi.ptr(m, C.POINTER(abi.RtMaterial)), len(m),
            C.byref(_cam(camera, params)), C.byref(params))
    check(lib().rt_tile_order(*args, None, 0, C.byref(nb), C.byref(nl), C.byref(ns)))
    perm = np.zeros(nb.value, dtype=np.uint32)
    if nb.value:
        check(lib().rt_tile_order(*args, abi.ptr(perm, C.POINTER(C.c_uint32)), nb.value, C.byref(nb), C.byref(nl),
                                  C.byref(ns)))
    return perm, nl.value, ns.value


def tile_ground(scene, params, camera=None):
    """rt_tile_ground: the pass's ground blocks, positions [n_lead, n_lead + n) of
    tile_order()'s perm; 0 when the scene or the pass keeps them in the main launch."""
    s, m = _scene_arrays(scene)
    n = C.c_uint32(0)
    check(lib().rt_tile_ground(abi.ptr(s, C.POINTER(abi.RtSphere)), len(s), abi.ptr(m, C.POINTER(abi.RtMaterial)), len(m),
                               C.byref(_cam(camera, params)), C.byref(params), C.byref(n)))
    return n.value


def trap_windows(scene):
    """rt_trap_windows: per sphere (cos_lo, cos_hi), the trap window of an isolated glass ball
    (DESIGN.md §4.1a); (1, 0) for a sphere without one."""
    s, m = _scene_arrays(scene)
    out = np.zeros((len(s), 2), dtype=np.float32)
    check(lib().rt_trap_windows(abi.ptr(s, C.POINTER(abi.RtSphere)), len(s), abi.ptr(m, C.POINTER(abi.RtMaterial)),
                                len(m), abi.ptr(out, C.POINTER(C.c_float))))
    return out


def release_cached():
    """rt_release_cached: free the device context the synchronous renders keep between calls."""
    check(lib().rt_release_cached())


def render_multi_f32(scene, params, ngpu=0, camera=None):
    """Row-interleaved render over `ngpu` devices of this process, gathered with RCCL."""
    s, m = _scene_arrays(scene)
    out = np.zeros((params.height, params.width, 3), dtype=np.float32)
    st = abi.RtStats()
    check(lib().rt_render_multi_f32(abi.ptr(s, C.POINTER(abi.RtSphere)), len(s),
                                    abi.ptr(m, C.POINTER(abi.RtMaterial)), len(m), C.byref(_cam(camera, params)),
                                    C.byref(params), ngpu, abi.ptr(out, C.POINTER(C.c_float)), C.byref(st)))
    return out, st


def render_multi_rgb8(scene, params, ngpu=0, camera=None):
    """As render_multi_f32 with the gamma/u8 epilogue on every rank before the gather."""
    s, m = _scene_arrays(scene)
    out = np.zeros((params.height, params.width, 3), dtype=np.uint8)
    st = abi.RtStats()
    check(lib().rt_render_multi_rgb8(abi.ptr(s, C.POINTER(abi.RtSphere)), len(s),
                                     abi.ptr(m, C.POINTER(abi.RtMaterial)), len(m), C.byref(_cam(camera, params)),
                                     C.byref(params), ngpu, abi.ptr(out, C.POINTER(C.c_uint8)), C.byref(st)))
    return out, st


class MultiContext:
    """Persistent row-tile context over ranks (rt_multi_create): rank r renders rows r, r+N, ...
    on devices[r]; tiles are gathered to rank 0 (RCCL when every rank has its own device,
    device copies for ranks sharing rank 0's device) and de-interleaved into the frame."""

    def __init__(self, scene, devices=None, n_ranks=0, options=None):
        s, m = _scene_arrays(scene)
        h = C.c_void_p()
        devs = None
        if devices is not None:
            devs = (C.c_int * len(devices))(*devices)
            n_ranks = len(devices)
        check(lib().rt_multi_create_ex(abi.ptr(s, C.POINTER(abi.RtSphere)), len(s),
                                       abi.ptr(m, C.POINTER(abi.RtMaterial)), len(m), devs, n_ranks,
                                       C.byref(options) if options is not None else None, C.byref(h)))
        self.handle = h
        n, r = C.c_int(0), C.c_int(0)
        check(lib().rt_multi_info(h, C.byref(n), C.byref(r)))
        self.n_ranks, self.uses_rccl = n.value, bool(r.value)

    def render_f32(self, params, camera=None):
        out = np.zeros((params.height, params.width, 3), dtype=np.float32)
        st = abi.RtStats()
        check(lib().rt_multi_render_f32(self.handle, C.byref(_cam(camera, params)), C.byref(params),
                                        abi.ptr(out, C.POINTER(C.c_float)), C.byref(st)))
        return out, st

    def render_rgb8(self, params, camera=None):
        out = np.zeros((params.height, params.width, 3), dtype=np.uint8)
        st = abi.RtStats()
        check(lib().rt_multi_render_rgb8(self.handle, C.byref(_cam(camera, params)), C.byref(params),
                                         abi.ptr(out, C.POINTER(C.c_uint8)), C.byref(st)))
        return out, st

    def render_device(self, camera, params, d_out, stream=None, rgb8=False):
        """Enqueue a full frame into device pointer d_out on rank 0's device, `stream` order."""
        check(lib().rt_multi_render_device(self.handle, C.byref(_cam(camera, params)), C.byref(params),
                                           abi.RT_OUTPUT_RGB8 if rgb8 else abi.RT_OUTPUT_F32, C.c_void_p(d_out),
                                           C.c_void_p(stream or 0)))

    def close(self):
        if self.handle:
            lib().rt_multi_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_cuda_impl(width, height):
    """cuda_impl(width, height, image_texels) (src/main.cxx:18, src/CUDA/cuda_impl.cu:384-453):
    the CUDA variant's scene, camera, 48 spp and 32 bounces; u8 RGB (height, width, 3)."""
    out = np.zeros((height, width, 3), dtype=np.uint8)
    check(lib().rt_render_cuda_impl(width, height, abi.ptr(out, C.POINTER(C.c_uint8))))
    return out


class DeviceScene:
    """A scene resident in HBM on one device (rt_scene_create); renders are stream-ordered."""

    def __init__(self, scene, device=0, options=None):
        s, m = _scene_arrays(scene)
        self.n_spheres, self.n_materials = len(s), len(m)
        h = C.c_void_p()
        check(lib().rt_scene_create_ex(abi.ptr(s, C.POINTER(abi.RtSphere)), len(s),
                                       abi.ptr(m, C.POINTER(abi.RtMaterial)), len(m), device,
                                       C.byref(options) if options is not None else None, C.byref(h)))
        self.handle = h
        self.device = device

    def update(self, scene):
        """rt_scene_update: new records into the live scene (the same number of spheres), in place;
        its streams, workspaces and sessions stay. Synchronous."""
        s, m = _scene_arrays(scene)
        check(lib().rt_scene_update(self.handle, abi.ptr(s, C.POINTER(abi.RtSphere)), len(s),
                                    abi.ptr(m, C.POINTER(abi.RtMaterial)), len(m)))
        self.n_materials = len(m)

    def motion(self):
        """rt_scene_motion as a dict: n_spheres, the device addresses centres and prev_centres of the
        two [n][4] tables (valid until the next update), geometry_epoch, appearance_epoch."""
        r = abi.RtSceneMotion()
        check(lib().rt_scene_motion(self.handle, C.byref(r)))
        return {"n_spheres": r.n_spheres, "centres": r.centres or 0, "prev_centres": r.prev_centres or 0,
                "geometry_epoch": r.geometry_epoch, "appearance_epoch": r.appearance_epoch}

    def render(self, camera, params, d_rgb, stream=None, d_segments=None):
        """Enqueue a render into device pointer d_rgb (int address) on `stream` (int handle).
        d_segments: optional device int64[3] accumulating {segments, sphere tests, box tests}."""
        check(lib().rt_render_device(self.handle, C.byref(_cam(camera, params)), C.byref(params),
                                     C.c_void_p(d_rgb), C.c_void_p(stream or 0),
                                     C.c_void_p(d_segments) if d_segments else None))

    def render_aov(self, camera, params, buffers, samples=0, stream=None):
        """Enqueue the first-hit feature buffers (rt_render_aov_device) on `stream`: `buffers` is a
        dict plane name (albedo, normal, depth, alpha, sphere_id) -> device address, laid out as
        `params` says; samples 0..samples-1 of every pixel (0: all of params.spp)."""
        rec = aov_buffers(buffers, samples)
        check(lib().rt_render_aov_device(self.handle, C.byref(_cam(camera, params)), C.byref(params), C.byref(rec),
                                         C.c_void_p(stream or 0)))

    def render_var(self, camera, params, rgb_ptr, var_ptr, stream=None, segments=None):
        """Enqueue rt_render_var_device on `stream`: the beauty into device address rgb_ptr as
        render() writes it, the variance of each pixel's mean luminance (one float per pixel,
        laid out as `params` says) into var_ptr. segments: optional device int64[3], as render()."""
        check(lib().rt_render_var_device(self.handle, C.byref(_cam(camera, params)), C.byref(params),
                                         C.c_void_p(rgb_ptr), C.c_void_p(var_ptr), C.c_void_p(stream or 0),
                                         C.c_void_p(segments) if segments else None))

    def preview(self, params, upscale=None):
        """A preview session on this scene (Preview; preview_params makes the record, preview_upscale
        the record of an upscaled one)."""
        return Preview(self, params, upscale)

    def progressive(self, camera, params):
        """A progressive session on this scene (Progressive): the frame of `params` in sample windows."""
        return Progressive(self, _cam(camera, params), params)

    def adaptive(self, camera, params, adaptive):
        """An adaptive session on this scene (Adaptive): the frame of `params` in sample windows that
        leave out the 64-pixel blocks retired by the rule of `adaptive` (adaptive_params)."""
        return Adaptive(self, _cam(camera, params), params, adaptive)

    def tile_order(self, camera, params, stream=None):
        """rt_tile_order_device: the pass's dealing order computed by the device's classification
        kernels from this scene's geometry, as tile_order() returns the host's:
        (perm, n_lead, n_sky), perm copied back from a device buffer (a torch tensor on the
        scene's device)."""
        import torch
        cam = _cam(camera, params)
        nb, nl, ns = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        st = C.c_void_p(stream or 0)
        check(lib().rt_tile_order_device(self.handle, C.byref(cam), C.byref(params), None, 0, C.byref(nb), C.byref(nl),
                                         C.byref(ns), st))
        if not nb.value:
            return np.zeros(0, dtype=np.uint32), nl.value, ns.value
        buf = torch.empty(nb.value, dtype=torch.int32, device=f"cuda:{self.device}")
        check(lib().rt_tile_order_device(self.handle, C.byref(cam), C.byref(params), C.c_void_p(buf.data_ptr()), nb.value,
                                         C.byref(nb), C.byref(nl), C.byref(ns), st))
        return buf.cpu().numpy().view(np.uint32), nl.value, ns.value

    def order_counts(self):
        """rt_scene_order_counts: dealing orders this scene computed on the host and on the device,
        and the calls that found theirs cached, as a dict (host_orders, device_orders, hits)."""
        h, d, n = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(lib().rt_scene_order_counts(self.handle, C.byref(h), C.byref(d), C.byref(n)))
        return {"host_orders": h.value, "device_orders": d.value, "hits": n.value}

    def ground_counts(self):
        """rt_scene_ground_counts: the ground kernel's samples in the last frame that used it and
        how many of them went to the redo launch, as (ground, redone). Waits for
        the device."""
        g, r = C.c_uint64(0), C.c_uint64(0)
        check(lib().rt_scene_ground_counts(self.handle, C.byref(g), C.byref(r)))
        return g.value, r.value

    def usage(self):
        """rt_scene_usage_get: device bytes held and the last render's cut, as a dict."""
        u = abi.RtSceneUsage()
        check(lib().rt_scene_usage_get(self.handle, C.byref(u)))
        return {k: getattr(u, k) for k, _ in abi.RtSceneUsage._fields_}

    def kernel_times(self, max_calls=256):
        """Render-kernel durations (ms) of the most recent render() calls, oldest first."""
        buf = (C.c_float * max_calls)()
        n = C.c_uint32(0)
        check(lib().rt_scene_kernel_times(self.handle, max_calls, buf, C.byref(n)))
        return list(buf[:n.value])

    def debug_counters(self, reset=True):
        """Counters of the instrumented kernel (options stats=True), see rt_scene_debug_counters."""
        buf = (C.c_uint64 * 16)()
        check(lib().rt_scene_debug_counters(self.handle, buf, 1 if reset else 0))
        keys = ["wave_iters", "wave_refills", "wave_blocks", "lane_blocks", "wave_roots", "lane_roots", "segments",
                "wave_member_blocks", "cyc_refill", "cyc_start", "cyc_hit", "cyc_shade", "cyc_fold"]
        out = dict(zip(keys, list(buf)))
        out["items_dealt"] = buf[13]  # items (the deep launch: queued paths) the waves took
        out["launch_start"] = (~buf[14]) & 0xffffffffffffffff if buf[14] else 0  # 100 MHz ticks
        return out

    EVENTS = ["iter", "refill_trip", "fresh", "reject_trip", "lens_done", "scatter_done", "root_gate_pass", "super",
              "super_pass", "cluster_req", "transposed", "t_round", "t_far", "per_lane_members", "sky", "hit",
              "lambert", "unit_dir", "dielectric", "store", "metal_absorb", "live_lanes", "dry_iter", "dry_lanes",
              "iso_lanes", "walk_skipped", "walk_1", "walk_2", "walk_3_4", "walk_5_8", "pair_sums", "both_deep_meets"]

    def debug_events(self, reset=True):
        """Block-execution counts of the instrumented kernel (options stats=True), see rt_scene_debug_events."""
        buf = (C.c_uint64 * 32)()
        check(lib().rt_scene_debug_events(self.handle, buf, 1 if reset else 0))
        return dict(zip(self.EVENTS, list(buf)))

    def debug_timeline(self, max_waves=65536):
        """Per-wave (dry, exit, iterations, cu_id, refills, iterations_after_dry, start, cycles) of
        the last instrumented launch (options stats=True). For a deep launch two fields hold walk
        counts instead: dry = (walks with a walking lane that has no hint sphere) << 32 | walks,
        iterations_after_dry = iterations in which the wave walked the clusters. Otherwise dry =
        when the wave found every queue empty;
        times in ticks of the 100 MHz clock; cycles = shader-clock cycles in the loop, so
        cycles / (exit - start) x 100 MHz is the clock the wave ran at), see rt_scene_debug_timeline."""
        buf = (C.c_uint64 * (4 * max_waves))()
        n = C.c_uint32(0)
        check(lib().rt_scene_debug_timeline(self.handle, buf, max_waves, C.byref(n)))
        out = []
        for i in range(n.value):
            dry, ex, a, b = buf[4 * i], buf[4 * i + 1], buf[4 * i + 2], buf[4 * i + 3]
            start = (ex & ~0xffffffff) | (b & 0xffffffff)  # the start's low 32 bits, in the exit's epoch
            if start > ex:
                start -= 1 << 32
            out.append((dry, ex, a & 0xffff, b >> 48, (a >> 16) & 0xffff, (b >> 32) & 0xffff, start, a >> 32))
        return out

    def close(self):
        if self.handle:
            lib().rt_scene_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def epilogue_rgb8_device(d_rgb, d_out, n_pixels, stream=None):
    check(lib().rt_epilogue_rgb8_device(C.c_void_p(d_rgb), C.c_void_p(d_out), n_pixels, C.c_void_p(stream or 0)))


def save_ppm(path, rgb8):
    """app::save_to_file (src/main.cxx:87-101) through rt_write_ppm: binary P6,
    'P6\\n<w> <h>\\n255\\n' then the (h, w, 3) texels."""
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    h, w, _ = rgb8.shape
    check(lib().rt_write_ppm(os.fsencode(path), abi.ptr(rgb8, C.POINTER(C.c_uint8)), w, h))
