"""ctypes mirror of include/rt_api.h (the C-ABI boundary).

Record layouts are the C structs one for one; numpy dtypes are provided for the arrays
(spheres, materials) so scenes can be built and inspected without copies.
"""
import ctypes as C

import numpy as np

RT_OK = 0
RT_ERR_INVALID = -1
RT_ERR_DEVICE = -2
RT_ERR_CAPACITY = -3
RT_ERR_UNSUPPORTED = -4
RT_ERR_COMM = -5
RT_ERR_IO = -6

RT_OUTPUT_F32, RT_OUTPUT_RGB8 = 0, 1

RT_LAMBERT, RT_METAL, RT_DIELECTRIC = 0, 1, 2
RT_CAMERA_REFERENCE, RT_CAMERA_CORRECTED = 0, 1

RT_FLAG_FULL_FRAME = 1 << 0
RT_FLAG_FAST_MATH = 1 << 1
RT_FLAG_SCALAR_SCENE = 1 << 2
RT_FLAG_BRUTE_FORCE = 1 << 3
RT_FLAG_CUDA_COMPAT = 1 << 4  # semantics of src/CUDA/cuda_impl.cu
RT_FLAG_WAVEFRONT = 1 << 5  # A/B: per-segment launches with HBM ray queues (same bits)

RT_DENOISE_DEMODULATE = 1 << 0  # filter beauty / albedo', multiply back at the end
RT_DENOISE_DIRECT = 1 << 1  # A/B: every level by the direct-load kernel (same bits)

RT_PREVIEW_DEMODULATE = 1 << 0  # the temporal stage and the filter work on beauty / albedo'
RT_PREVIEW_FEEDBACK = 1 << 1  # the first filter level's output is what the next frame reprojects
RT_PREVIEW_NO_TEMPORAL = 1 << 2  # every frame filtered on its own


class RtSphere(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float), ("material", C.c_uint32)]


class RtMaterial(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("albedo", C.c_float * 3), ("param", C.c_float)]


class RtCamera(C.Structure):
    _fields_ = [
        ("origin", C.c_float * 3),
        ("lower_left_corner", C.c_float * 3),
        ("horizontal", C.c_float * 3),
        ("vertical", C.c_float * 3),
        ("lens_radius", C.c_float),
        ("mode", C.c_uint32),
    ]


class RtParams(C.Structure):
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("spp", C.c_uint32), ("max_depth", C.c_uint32),
        ("seed", C.c_uint64),
        ("row_offset", C.c_uint32), ("row_stride", C.c_uint32), ("num_rows", C.c_uint32),
        ("flags", C.c_uint32),
    ]


class RtOptions(C.Structure):
    """rt_options (include/rt_api.h): resource bounds and same-bits variants of a scene."""
    _fields_ = [
        ("size", C.c_uint32), ("render_streams", C.c_uint32), ("workspaces_per_stream", C.c_uint32),
        ("deep_split", C.c_uint32), ("max_pass_bytes", C.c_uint64), ("max_workspace_bytes", C.c_uint64),
        ("deep_min_items", C.c_uint64), ("cluster_size", C.c_uint32), ("transpose_max", C.c_uint32),
        ("wave_queue_rays", C.c_uint32), ("diag", C.c_uint32), ("ring_pass_bytes", C.c_uint64),
        ("tile_classes", C.c_uint32), ("sky_moments", C.c_uint32),
    ]


class RtSceneUsage(C.Structure):
    _fields_ = [
        ("device_bytes", C.c_uint64), ("workspace_bytes", C.c_uint64), ("render_streams", C.c_uint32),
        ("workspaces", C.c_uint32), ("pass_samples", C.c_uint32), ("static_lds_bytes", C.c_uint32),
        ("max_lds_bytes", C.c_uint32), ("deep_launch", C.c_uint32), ("pair_passes", C.c_uint32),
        ("split_passes", C.c_uint32), ("lead_tiles", C.c_uint32), ("sky_tiles", C.c_uint32),
    ]


RT_DIAG = {
    "ieee_roots": 1 << 0, "no_shortcut": 1 << 1, "no_neighbours": 1 << 2, "no_root_box": 1 << 3,
    "shade_lds": 1 << 4, "shade_global": 1 << 5, "stats": 1 << 6, "stats_deep_only": 1 << 7, "verbose": 1 << 8,
    "standin_transport": 1 << 9, "unbounded_nb": 1 << 10, "no_pairs": 1 << 11, "pairs": 1 << 12,
    "in_flight": 1 << 13, "natural_order": 1 << 14, "no_sky": 1 << 15, "lone_unsplit": 1 << 16,
    "sky_serial": 1 << 17, "no_trap_end": 1 << 19,
}


class RtProgressiveOutputs(C.Structure):
    """rt_progressive_outputs (include/rt_api.h): what a step's resolve writes, NULL = not wanted."""
    _fields_ = [
        ("size", C.c_uint32), ("noise_tau", C.c_float),
        ("rgb", C.c_void_p), ("variance", C.c_void_p), ("rgb8", C.c_void_p), ("noisy", C.c_void_p),
    ]


class RtProgressiveInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint32), ("done", C.c_uint32), ("spp", C.c_uint32), ("reserved", C.c_uint32),
        ("n_pixels", C.c_uint64), ("state_bytes", C.c_uint64), ("device_bytes", C.c_uint64),
    ]


class RtAdaptiveParams(C.Structure):
    """rt_adaptive_params (include/rt_api.h): the retire rule of an adaptive session."""
    _fields_ = [
        ("size", C.c_uint32), ("noise_tau", C.c_float), ("max_noisy", C.c_uint32), ("min_samples", C.c_uint32),
    ]


class RtAdaptiveOutputs(C.Structure):
    """rt_adaptive_outputs (include/rt_api.h): what a step's resolve writes, NULL = not wanted."""
    _fields_ = [
        ("size", C.c_uint32), ("reserved", C.c_uint32),
        ("rgb", C.c_void_p), ("variance", C.c_void_p), ("rgb8", C.c_void_p), ("samples", C.c_void_p), ("noisy", C.c_void_p),
    ]


class RtAdaptiveInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint32), ("done", C.c_uint32), ("spp", C.c_uint32), ("n_blocks", C.c_uint32),
        ("active_blocks", C.c_uint32), ("finished", C.c_uint32),
        ("n_pixels", C.c_uint64), ("samples_rendered", C.c_uint64), ("device_bytes", C.c_uint64),
    ]


class RtStats(C.Structure):
    _fields_ = [
        ("primaries", C.c_uint64), ("segments", C.c_uint64), ("sphere_tests", C.c_uint64),
        ("box_tests", C.c_uint64),
        ("kernel_ms", C.c_double), ("wall_ms", C.c_double),
    ]


class RtAovBuffers(C.Structure):
    """rt_aov_buffers (include/rt_api.h): the first-hit feature planes of a call, NULL = not wanted."""
    _fields_ = [
        ("size", C.c_uint32), ("samples", C.c_uint32),
        ("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("alpha", C.c_void_p),
        ("sphere_id", C.c_void_p),
    ]


class RtDenoiseParams(C.Structure):
    """rt_denoise_params (include/rt_api.h): the à-trous denoiser's image size, levels and sigmas."""
    _fields_ = [
        ("size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("levels", C.c_uint32),
        ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
        ("sigma_albedo", C.c_float), ("flags", C.c_uint32),
    ]


class RtDenoiseBuffers(C.Structure):
    """rt_denoise_buffers (include/rt_api.h): the planes of a denoise call, NULL = guide not given."""
    _fields_ = [
        ("size", C.c_uint32),
        ("beauty", C.c_void_p), ("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p),
        ("out", C.c_void_p), ("scratch", C.c_void_p),
    ]


class RtDenoiseVarBuffers(C.Structure):
    """rt_denoise_var_buffers (include/rt_api.h): the variance planes of a variance-guided denoise."""
    _fields_ = [
        ("size", C.c_uint32), ("var_floor", C.c_float),
        ("variance", C.c_void_p), ("variance_out", C.c_void_p), ("var_scratch", C.c_void_p),
    ]


class RtTemporalParams(C.Structure):
    """rt_temporal_params (include/rt_api.h): the temporal accumulation's image size, blend and tests."""
    _fields_ = [
        ("size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
        ("alpha_min", C.c_float), ("max_history", C.c_float), ("normal_tol", C.c_float), ("depth_tol", C.c_float),
        ("flags", C.c_uint32),
    ]


# the planes of rt_temporal_buffers, in the record's order: name -> (channels, numpy dtype)
TEMPORAL_PLANES = {
    "beauty": (3, np.float32), "variance": (1, np.float32), "normal": (3, np.float32), "depth": (1, np.float32),
    "alpha": (1, np.float32), "sphere_id": (1, np.uint32),
    "prev_color": (3, np.float32), "prev_variance": (1, np.float32), "prev_history": (1, np.float32),
    "prev_normal": (3, np.float32), "prev_depth": (1, np.float32), "prev_sphere_id": (1, np.uint32),
    "out_color": (3, np.float32), "out_variance": (1, np.float32), "out_history": (1, np.float32),
}


class RtTemporalBuffers(C.Structure):
    """rt_temporal_buffers (include/rt_api.h): the current frame's planes, the previous frame's (all
    NULL: no history yet) and the outputs of a temporal accumulation."""
    _fields_ = [("size", C.c_uint32)] + [(n, C.c_void_p) for n in TEMPORAL_PLANES]


class RtTemporalMotion(C.Structure):
    """rt_temporal_motion_t (include/rt_api.h): the two sphere tables [n_spheres][4] {cx, cy, cz, r} of
    the temporal stage with object motion, now and at the previous frame."""
    _fields_ = [("size", C.c_uint32), ("n_spheres", C.c_uint32), ("centres", C.c_void_p), ("prev_centres", C.c_void_p)]


class RtSceneMotion(C.Structure):
    """rt_scene_motion_t (include/rt_api.h): a device scene's two sphere tables and its epochs."""
    _fields_ = [("size", C.c_uint32), ("n_spheres", C.c_uint32), ("centres", C.c_void_p), ("prev_centres", C.c_void_p),
                ("geometry_epoch", C.c_uint64), ("appearance_epoch", C.c_uint64)]


assert C.sizeof(RtTemporalMotion) == 24 and C.sizeof(RtSceneMotion) == 40


class RtTemporalClip(C.Structure):
    """rt_temporal_clip_t (include/rt_api.h): the window and the box width of the temporal stage's
    history clamp."""
    _fields_ = [("size", C.c_uint32), ("radius", C.c_uint32), ("gamma", C.c_float), ("flags", C.c_uint32)]


assert C.sizeof(RtTemporalClip) == 16


class RtUpsampleParams(C.Structure):
    """rt_upsample_params (include/rt_api.h): the guided upsample's two image sizes and tap tests."""
    _fields_ = [
        ("size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
        ("lo_width", C.c_uint32), ("lo_height", C.c_uint32),
        ("normal_tol", C.c_float), ("depth_tol", C.c_float), ("flags", C.c_uint32),
    ]


# the planes of rt_upsample_buffers, in the record's order: name -> (channels, numpy dtype); the lo_
# planes have the low-resolution size, the others the output's
UPSAMPLE_PLANES = {
    "lo_color": (3, np.float32), "lo_variance": (1, np.float32), "lo_normal": (3, np.float32),
    "lo_depth": (1, np.float32), "lo_sphere_id": (1, np.uint32),
    "normal": (3, np.float32), "depth": (1, np.float32), "alpha": (1, np.float32), "sphere_id": (1, np.uint32),
    "out_color": (3, np.float32), "out_variance": (1, np.float32),
}


class RtUpsampleBuffers(C.Structure):
    """rt_upsample_buffers (include/rt_api.h): the low-resolution image and guides, the guides of the
    output size and the outputs of a guided upsample."""
    _fields_ = [("size", C.c_uint32)] + [(n, C.c_void_p) for n in UPSAMPLE_PLANES]


class RtPreviewUpscale(C.Structure):
    """rt_preview_upscale (include/rt_api.h): the output size, guide samples and tap tests of an
    upscaled preview session."""
    _fields_ = [
        ("size", C.c_uint32), ("out_width", C.c_uint32), ("out_height", C.c_uint32), ("guide_samples", C.c_uint32),
        ("normal_tol", C.c_float), ("depth_tol", C.c_float),
    ]


# the planes of rt_preview_output_t, in the record's order: name -> (channels, numpy dtype)
PREVIEW_OUTPUT_PLANES = {
    "upsampled": (3, np.float32), "albedo": (3, np.float32), "normal": (3, np.float32), "depth": (1, np.float32),
    "alpha": (1, np.float32), "sphere_id": (1, np.uint32),
}


class RtPreviewOutput(C.Structure):
    """rt_preview_output_t (include/rt_api.h): what an upscaled session's last frame wrote at the
    output size."""
    _fields_ = ([("size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32)]
                + [(n, C.c_void_p) for n in PREVIEW_OUTPUT_PLANES])


class RtPreviewParams(C.Structure):
    """rt_preview_params (include/rt_api.h): a preview session's frame size, render, switches and the
    records of its temporal stage and its filter."""
    _fields_ = [
        ("size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32),
        ("max_depth", C.c_uint32), ("flags", C.c_uint32), ("var_floor", C.c_float),
        ("temporal", RtTemporalParams), ("denoise", RtDenoiseParams),
    ]


# the planes of rt_preview_planes_t, in the record's order: name -> (channels, numpy dtype)
PREVIEW_PLANES = {
    "out_color": (3, np.float32), "out_variance": (1, np.float32), "out_history": (1, np.float32),
    "albedo": (3, np.float32), "normal": (3, np.float32), "depth": (1, np.float32), "alpha": (1, np.float32),
    "sphere_id": (1, np.uint32),
    "prev_color": (3, np.float32), "prev_variance": (1, np.float32), "prev_history": (1, np.float32),
    "prev_normal": (3, np.float32), "prev_depth": (1, np.float32), "prev_sphere_id": (1, np.uint32),
}


class RtPreviewPlanes(C.Structure):
    """rt_preview_planes_t (include/rt_api.h): the device planes a session's last frame wrote."""
    _fields_ = [("size", C.c_uint32), ("frames", C.c_uint32)] + [(n, C.c_void_p) for n in PREVIEW_PLANES]


# the planes of rt_denoise_buffers: name -> channels
DENOISE_PLANES = {"beauty": 3, "albedo": 3, "normal": 3, "depth": 1, "out": 3, "scratch": 3}

# the planes of rt_denoise_var_buffers: name -> floats per pixel (var_scratch holds two planes)
DENOISE_VAR_PLANES = {"variance": 1, "variance_out": 1, "var_scratch": 2}

# the planes of rt_aov_buffers: name -> (channels, numpy dtype, value of a pixel no call wrote)
AOV_PLANES = {"albedo": (3, np.float32, 0), "normal": (3, np.float32, 0), "depth": (1, np.float32, 0),
              "alpha": (1, np.float32, 0), "sphere_id": (1, np.uint32, 0xffffffff)}

SPHERE_DTYPE = np.dtype([("center", "<f4", (3,)), ("radius", "<f4"), ("material", "<u4")])
MATERIAL_DTYPE = np.dtype([("kind", "<u4"), ("albedo", "<f4", (3,)), ("param", "<f4")])
assert SPHERE_DTYPE.itemsize == C.sizeof(RtSphere) == 20
assert MATERIAL_DTYPE.itemsize == C.sizeof(RtMaterial) == 20
assert C.sizeof(RtParams) == 40
assert C.sizeof(RtOptions) == 72 and C.sizeof(RtSceneUsage) == 56
assert C.sizeof(RtAovBuffers) == 48
assert C.sizeof(RtDenoiseParams) == 36 and C.sizeof(RtDenoiseBuffers) == 56
assert C.sizeof(RtDenoiseVarBuffers) == 32
assert C.sizeof(RtTemporalParams) == 32 and C.sizeof(RtTemporalBuffers) == 128
assert C.sizeof(RtPreviewParams) == 96 and C.sizeof(RtPreviewPlanes) == 120
assert C.sizeof(RtUpsampleParams) == 32 and C.sizeof(RtUpsampleBuffers) == 96
assert C.sizeof(RtPreviewUpscale) == 24 and C.sizeof(RtPreviewOutput) == 64


def ptr(arr, ctype=C.c_void_p):
    """Pointer to a contiguous numpy array's data, typed for a ctypes argument."""
    assert arr.flags["C_CONTIGUOUS"]
    return C.cast(arr.ctypes.data, ctype)


def rows_of(params):
    """Number of rows a render covers (rt_params num_rows rule, include/rt_api.h)."""
    if params.num_rows:
        return params.num_rows
    st = params.row_stride or 1
    if params.row_offset >= params.height:
        return 0
    return (params.height - params.row_offset + st - 1) // st


def load_scene_file(path):
    """Scene fixture: 'RTSC' u32 version=1, u32 n_spheres, u32 n_materials, records."""
    raw = np.fromfile(path, dtype=np.uint8)
    hdr = raw[:16].view("<u4")
    if hdr[0] != 0x43535452 or hdr[1] != 1:
        raise ValueError(f"{path}: not an RTSC v1 scene file")
    ns, nm = int(hdr[2]), int(hdr[3])
    s = raw[16:16 + 20 * ns].view(SPHERE_DTYPE).copy()
    m = raw[16 + 20 * ns:16 + 20 * ns + 20 * nm].view(MATERIAL_DTYPE).copy()
    return s, m


def save_scene_file(path, spheres, materials):
    hdr = np.array([0x43535452, 1, len(spheres), len(materials)], dtype="<u4")
    with open(path, "wb") as f:
        f.write(hdr.tobytes())
        f.write(np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE).tobytes())
        f.write(np.ascontiguousarray(materials, dtype=MATERIAL_DTYPE).tobytes())
