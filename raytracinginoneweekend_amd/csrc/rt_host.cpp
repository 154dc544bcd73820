// rt_host.cpp — the render path of the C-ABI's host side (include/rt_api.h): the checks of a
// call's params, the stages of a render under the scene's options (kernel choice, the frame's plan
// from rt_plan.cpp, workspaces, the launches of every pass), frames in flight, the compat and
// feature-buffer renders, and the device entry points (rt_render_device, rt_render_var_device,
// rt_render_aov_device, rt_epilogue_rgb8_device). The scene record is rt_scene.h's: its lifecycle
// is rt_host_scene.cpp, its dealing orders rt_host_order.cpp, the synchronous host-buffer calls
// rt_host_synccall.cpp. The multi-GPU context is rt_host_multi.cpp; the filters and temporal
// accumulation are rt_host_post.cpp; the host-only half is rt_host_build.cpp (camera and scene
// constructors, cluster builder, the scene derivation, options, PPM writer, the synchronous calls'
// plane layout) and rt_plan.cpp (the pass planner).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rt_api.h"
#include "rt_device.h"
#include "rt_host_build.h"
#include "rt_host_sync.h"
#include "rt_plan.h"
#include "rt_scene.h"

using namespace rthost;

#ifndef RT_LONE_DEEP_TMAX
#define RT_LONE_DEEP_TMAX 4u  // the lone deep launch's transposition threshold (below)
#endif

// the deep launch of a lone pass stages the shading records in LDS (A/B build switch)
// lone split passes accumulate in two parts, the first beside the deep launch (A/B build switch)
#ifndef RT_LONE_SKY_ROOM
#define RT_LONE_SKY_ROOM -1  // -1: by the sky's share of the pass (see the main launch's grid)
#endif
#ifndef RT_TWO_PART
#define RT_TWO_PART 1
#endif
#ifndef RT_DEEP_LDS_STAGE
#define RT_DEEP_LDS_STAGE 1
#endif
// ... in 8-wave workgroups (one LDS copy of the scene for twice the waves), every workgroup
// resident at once, dealing the queued paths statically (A/B build switches)
#ifndef RT_DEEP_WIDE
#define RT_DEEP_WIDE 1
#endif
#ifndef RT_DEEP_STATIC
#define RT_DEEP_STATIC 1
#endif

// (rt_host_sync.h: rt_host_multi.cpp's entry points check their params the same way)
int rthost::check_params(const rt_params *p)
{
    if (!p) return fail(RT_ERR_INVALID, "params: null");
    if (!p->width || !p->height || !p->spp) return fail(RT_ERR_INVALID, "params: width, height and spp must be > 0");
    // the kernel forms the pixel index y W + x in 32 bits (sample streams' keys)
    if (static_cast<uint64_t>(p->width) * p->height >= (1ull << 32))
        return fail(RT_ERR_INVALID, "params: width * height must be below 2^32");
    const uint32_t st = p->row_stride ? p->row_stride : 1;
    const uint32_t rows = rows_of(*p);
    if (rows && static_cast<uint64_t>(p->row_offset) + static_cast<uint64_t>(rows - 1) * st >= p->height)
        return fail(RT_ERR_INVALID, "params: rows exceed the image height");
    if (p->flags & ~(RT_FLAG_FULL_FRAME | RT_FLAG_FAST_MATH | RT_FLAG_SCALAR_SCENE | RT_FLAG_BRUTE_FORCE | RT_FLAG_CUDA_COMPAT |
                     RT_FLAG_WAVEFRONT))
        return fail(RT_ERR_INVALID, "params: unknown flag");
    return RT_OK;
}

namespace {
// the feature-buffer and variance renders: the exact kernel only
int exact_only(const rt_params *p, const std::string &w)
{
    static const struct { uint32_t bit; const char *name; } unsupported[] = {
        {RT_FLAG_FAST_MATH, "RT_FLAG_FAST_MATH"}, {RT_FLAG_SCALAR_SCENE, "RT_FLAG_SCALAR_SCENE"},
        {RT_FLAG_WAVEFRONT, "RT_FLAG_WAVEFRONT"}, {RT_FLAG_CUDA_COMPAT, "RT_FLAG_CUDA_COMPAT"}};
    for (const auto &u : unsupported)
        if (p->flags & u.bit) return fail(RT_ERR_UNSUPPORTED, w + ": " + u.name + " is not supported (the exact kernel only)");
    return RT_OK;
}
} // namespace

// The arguments of the feature-buffer calls, decided before any HIP call.
int rthost::check_aov(const rt_params *p, const rt_aov_buffers *a, const char *who)
{
    const std::string w(who);
    if (!a) return fail(RT_ERR_INVALID, w + ": null aov");
    if (a->size != sizeof(rt_aov_buffers))
        return fail(RT_ERR_INVALID, w + ": aov size " + std::to_string(a->size) + " is not sizeof(rt_aov_buffers) = " +
                                        std::to_string(sizeof(rt_aov_buffers)));
    if (int rc = check_params(p); rc != RT_OK) return rc;
    if (a->samples > p->spp)
        return fail(RT_ERR_INVALID, w + ": aov samples " + std::to_string(a->samples) + " exceed spp " + std::to_string(p->spp));
    if (!a->albedo && !a->normal && !a->depth && !a->alpha && !a->sphere_id)
        return fail(RT_ERR_INVALID, w + ": no plane requested");
    return exact_only(p, w);
}

namespace {

void fill_frame_consts(rt::KParams &k)
{
    rt::FrameConsts &f = k.fc;
    for (int c = 0; c < 3; ++c) { f.org[c] = k.org[c]; f.llc[c] = k.llc[c]; f.hor[c] = k.hor[c]; f.ver[c] = k.ver[c]; }
    f.lens = k.lens;
    f.fW = static_cast<float>(k.W);
    f.fH = static_cast<float>(k.H);
    f.corrected = k.corrected;
    f.W = k.W;
    f.spp = k.spp;
    f.inc_data_lo = static_cast<uint32_t>(k.inc_data);
    f.inc_data_hi = static_cast<uint32_t>(k.inc_data >> 32);
    f.inc_cam_lo = static_cast<uint32_t>(k.inc_cam);
    f.inc_cam_hi = static_cast<uint32_t>(k.inc_cam >> 32);
    f.row_offset = k.row_offset;
    f.row_stride = k.row_stride;
    f.tiled_rows = k.tiled_rows;
    f.tiles_x = k.tiles_x;
    f.tile_lw = k.tile_lw;
    f.n_pixels = k.n_pixels;
    f.sample_begin = k.sample_begin;
    f.div_W = make_udiv(k.W);
    f.div_tiles_x = make_udiv(k.tiles_x);
    f.div_n_pixels = make_udiv(k.n_pixels);
    f.rW = 1.f / f.fW;
    f.rH = 1.f / f.fH;
    f.div_fast = (exact_by_reciprocal(f.fW) ? 1u : 0u) | (exact_by_reciprocal(f.fH) ? 2u : 0u);
    f.n_pairs = k.n_pair_items / k.n_pixels;
}

bool camera_in_fast_range(const rt_camera &c)
{
    for (int i = 0; i < 3; ++i)
        for (float v : {c.origin[i], c.lower_left_corner[i], c.horizontal[i], c.vertical[i]})
            if (!(std::fabs(v) <= 0x1p19f)) return false;
    return std::fabs(c.lens_radius) <= 0x1p19f;
}

// a nonzero key of the camera basis and the depth limit (FNV-1a over their bytes)
unsigned long long camera_key(const rt_camera &c, uint32_t max_depth)
{
    unsigned long long h = 1469598103934665603ull;
    auto mix = [&](const void *p, size_t n) {
        for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const unsigned char *>(p)[i]) * 1099511628211ull;
    };
    mix(&c, sizeof(c));
    mix(&max_depth, sizeof(max_depth));
    return h ? h : 1ull;
}

// RT_FLAG_CUDA_COMPAT: the reference's CUDA variant semantics (compat_kernel), on the caller
// stream, spheres read from the index-ordered shading records of the brute-force blob.
int render_compat(rt_scene *sc, const rt_camera *camera, const rt_params &P, float *d_rgb, hipStream_t st,
                  uint64_t *d_segments);

// Render streams (rt_options.render_streams): 1 runs the render kernels on the caller stream;
// 2..kMaxBufs rotate that many internal streams. 0 (auto): one stream fewer than the process's
// hardware queues (GPU_MAX_HW_QUEUES, HIP's default 4; the caller's stream takes one), 2..7.
// The max-depth paths give every launch a drain of ~64 iterations whatever its size; with 3
// streams (and partial grids, grid_wg_per_cu) two other renders fill the machine while one
// drains. Measured on config 3 (frame stream): 3.81-3.87 ms/frame with 3 streams vs 3.90-3.93
// with 2; an 8-way row share (14.7 M samples) 0.63-0.64 vs 0.68. Round 3, with row shares split
// in flight: 7 streams beat 4 (config 3's 8-way share 0.50 vs 0.58 ms, 4-way 0.88 vs 0.95; the
// full frame 2.99-3.04 vs 3.06-3.08) and 8 (on 12 hardware queues) is slower again
// (profiles/r03/ab). More streams than hardware queues share queues and serialise.
uint32_t render_streams_of(const rt_options &o)
{
    if (o.render_streams) return o.render_streams;
    static const uint32_t hw_streams = [] {
        const char *q = std::getenv("GPU_MAX_HW_QUEUES");
        const unsigned long hw = q && *q ? std::strtoul(q, nullptr, 10) : 4ul;
        return static_cast<uint32_t>(std::clamp<unsigned long>(hw > 1 ? hw - 1 : 1, 2, 7));
    }();
    return hw_streams;
}

// Calls on one scene may come on different caller streams: order a call after everything the
// previous call enqueued on its stream (the accumulation buffer and counters are
// per scene), then remember this call's stream and its last work.
int stream_enter(rt_scene *sc, hipStream_t st)
{
    if (sc->tail_valid && st != sc->last_stream) RT_HIP(hipStreamWaitEvent(st, sc->ev_tail.get(), 0));
    return RT_OK;
}
int stream_leave(rt_scene *sc, hipStream_t st)
{
    RT_HIP(hipEventRecord(sc->ev_tail.get(), st));
    sc->last_stream = st;
    sc->tail_valid = true;
    return RT_OK;
}
// A sample window of a frame (a progressive session's step): samples [a, b) of
// the P.spp-sample frame, a a multiple of 4 and b a multiple of 4 or P.spp, folded into the caller's
// own planes (indexed like KAccum::acc / KAccum::mom) and never divided: no pass of a window is
// the frame's last.
// `blocks` (an adaptive session's): the window's passes are over these blocks' pixels alone.
struct Window {
    uint32_t a, b;
    float *acc, *mom;
    const WindowBlocks *blocks;
};
int render_device_impl(rt_scene *sc, const rt_camera *camera, const rt_params &P, float *d_rgb, hipStream_t st,
                       uint64_t *d_segments, float *d_var = nullptr, const Window *win = nullptr);
int window_first_order(rt_scene *sc, const rt_camera *camera, const rt_params &P, hipStream_t st, WindowBlocks &blocks);
} // namespace

extern "C" int rt_render_device(rt_scene *sc, const rt_camera *camera, const rt_params *params, float *d_rgb, void *stream,
                     uint64_t *d_segments)
{
    if (!sc || !camera || !d_rgb) return fail(RT_ERR_INVALID, "rt_render_device: null argument");
    if (int rc = check_params(params); rc != RT_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    RT_HIP(hipSetDevice(sc->device));
    if (int rc = stream_enter(sc, st); rc != RT_OK) return rc;
    const int rc = (params->flags & RT_FLAG_CUDA_COMPAT) ? render_compat(sc, camera, *params, d_rgb, st, d_segments)
                                                         : render_device_impl(sc, camera, *params, d_rgb, st, d_segments);
    if (rc != RT_OK) return rc;
    return stream_leave(sc, st);
}

// The params of a variance render (rt_render_var*, rt_progressive_create), decided before any HIP call.
int rthost::check_var_params(const rt_params *p, const char *who)
{
    if (int rc = check_params(p); rc != RT_OK) return rc;
    const std::string w(who);
    if (p->spp < 2u) return fail(RT_ERR_INVALID, w + ": spp must be at least 2 (a variance needs two samples)");
    return exact_only(p, w);
}

extern "C" int rt_render_var_device(rt_scene *sc, const rt_camera *camera, const rt_params *params, float *d_rgb, float *d_var,
                         void *stream, uint64_t *d_segments)
{
    if (!sc) return fail(RT_ERR_INVALID, "rt_render_var_device: null scene");
    if (!camera) return fail(RT_ERR_INVALID, "rt_render_var_device: null camera");
    if (!d_rgb) return fail(RT_ERR_INVALID, "rt_render_var_device: null d_rgb");
    if (!d_var) return fail(RT_ERR_INVALID, "rt_render_var_device: null d_var");
    if (d_var == d_rgb) return fail(RT_ERR_INVALID, "rt_render_var_device: d_var is also d_rgb");
    if (int rc = check_var_params(params, "rt_render_var_device"); rc != RT_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    RT_HIP(hipSetDevice(sc->device));
    if (int rc = stream_enter(sc, st); rc != RT_OK) return rc;
    if (int rc = render_device_impl(sc, camera, *params, d_rgb, st, d_segments, d_var); rc != RT_OK) return rc;
    return stream_leave(sc, st);
}

// A progressive session's step (rt_host_post.cpp; an adaptive session's, rt_host_adaptive.cpp, with
// `blocks`): samples [a, b) of the frame into the session's
// planes as one call on the scene (a == b: no render), then `after` (the resolve, which reads
// those planes) on the caller's stream, inside the call's stream order.
int rthost::render_window(rt_scene *sc, const rt_camera *camera, const rt_params &P, uint32_t a, uint32_t b, float *acc,
                          float *mom, hipStream_t st, uint64_t *d_segments, const std::function<int()> &after, WindowBlocks *blocks)
{
    RT_HIP(hipSetDevice(sc->device));
    if (int rc = stream_enter(sc, st); rc != RT_OK) return rc;
    if (blocks && blocks->first)
        if (int rc = window_first_order(sc, camera, P, st, *blocks); rc != RT_OK) return rc;
    const Window win{a, b, acc, mom, blocks};
    if (a < b && (!blocks || blocks->n_active))
        if (int rc = render_device_impl(sc, camera, P, nullptr, st, d_segments, nullptr, &win); rc != RT_OK) return rc;
    if (after)
        if (int rc = after(); rc != RT_OK) return rc;
    return stream_leave(sc, st);
}

// The rows and the pixel decomposition of the pass that P describes (rt_host_sync.h).
rthost::PixelLayout rthost::pixel_layout(const rt_params &P)
{
    PixelLayout l{};
    l.W = P.width;
    l.row_offset = P.row_offset;
    l.row_stride = P.row_stride ? P.row_stride : 1;
    l.num_rows = rows_of(P);
    l.full_frame = (P.flags & RT_FLAG_FULL_FRAME) ? 1u : 0u;
    l.n_pixels = static_cast<uint64_t>(P.width) * l.num_rows;
    // 64-pixel tiles (one wave's lanes for one sample), 8 x 8 (the kernel's decomposition takes
    // 2^lw x 64/2^lw; 16x4, 32x2 and 64x1 measured alike or slower for strided row shares:
    // 8-way share 0.61-0.62 ms at 8x8, 0.62 at 32x2, 0.66 at 64x1)
    l.tile_lw = 3u;
    const uint32_t tw = 1u << l.tile_lw, th = 64u >> l.tile_lw;
    const bool tiled = (P.width % tw) == 0u;
    l.tiles_x = tiled ? P.width / tw : 1u;
    l.tiled_rows = tiled ? (l.num_rows / th) * th : 0u;
    return l;
}

namespace {
// The camera, frame, rows and pixel decomposition of the pass that camera + P describe, into k
// (every render entry point fills them the same way); k.n_pixels = 0: no rows to render.
int frame_params(const rt_scene *sc, const rt_camera *camera, const rt_params &P, rt::KParams &k, const char *who)
{
    for (int c = 0; c < 3; ++c) {
        k.org[c] = camera->origin[c];
        k.llc[c] = camera->lower_left_corner[c];
        k.hor[c] = camera->horizontal[c];
        k.ver[c] = camera->vertical[c];
    }
    k.lens = camera->lens_radius;
    k.corrected = camera->mode == RT_CAMERA_CORRECTED;
    k.W = P.width;
    k.H = P.height;
    k.spp = P.spp;
    k.max_depth = P.max_depth;
    const PixelLayout l = pixel_layout(P);
    k.row_offset = l.row_offset;
    k.row_stride = l.row_stride;
    k.num_rows = l.num_rows;
    k.full_frame = l.full_frame;
    k.inc_data = ((2ull * P.seed) << 1u) | 1ull;
    k.inc_cam = ((2ull * P.seed + 1ull) << 1u) | 1ull;
    if (l.n_pixels >= (1ull << 31)) return fail(RT_ERR_INVALID, std::string(who) + ": more than 2^31 pixels in one call");
    k.n_pixels = static_cast<uint32_t>(l.n_pixels);
    k.tile_lw = l.tile_lw;
    k.tiles_x = l.tiles_x;
    k.tiled_rows = l.tiled_rows;
    k.n_spheres = sc->dev.n_spheres;
    k.n_materials = sc->dev.n_materials;
    return RT_OK;
}

// ---- the stages of a render (render_device_impl, below, is their sequence) ----------------------

// The shading records (the blob's tail) join the geometry in LDS unless that costs workgroups
// per CU; RT_DIAG_SHADE_LDS / RT_DIAG_SHADE_GLOBAL force the choice (same bits). occ_for(in_lds,
// &occ): the kernel's (cached) blocks per CU with the geometry alone or the whole blob in LDS;
// `fits`: the whole blob fits beside the kernel's static LDS; `query_unfit`: the second
// occupancy is asked for also when it does not.
struct ShadePlace {
    bool in_lds;
    int occ;  // of the placement chosen
};
template <class OccFor>
int place_shade(uint32_t diag, bool fits, bool query_unfit, OccFor occ_for, ShadePlace &out)
{
    int occ_geo = 0, occ_all = 0;
    if (int rc = occ_for(0, &occ_geo); rc) return rc;
    if (fits || query_unfit)
        if (int rc = occ_for(1, &occ_all); rc) return rc;
    out.in_lds = fits && ((diag & RT_DIAG_SHADE_LDS) ? true : (diag & RT_DIAG_SHADE_GLOBAL) ? false : occ_all >= occ_geo);
    out.occ = out.in_lds ? occ_all : occ_geo;
    return RT_OK;
}

// The kernel of a render call: what choose_kernel decides (and pair_occupancy completes).
struct KernelChoice {
    int variant, cull_mode;
    bool cull, wave;
    bool shade_fits;  // an LDS variant whose whole blob fits beside the kernel's static LDS
    size_t lds;       // dynamic LDS bytes (k.lds_units)
    int occ;          // workgroups per CU of the single-sample kernel
    int occ_pr;       // ... of its sample-pair instantiation (occ when there is none)
    bool pairs_ok;    // passes may store sample pairs
    bool order_ok;    // passes may be dealt by tile classes
};

// Variant: exact (bit-exact) or fast (tolerance); clustered culling unless brute force is
// asked for; the scalar-cache A/B variant is brute force only. Each needs its blob in LDS
// next to the static LDS of the kernel of its traversal (sc->static_lds[culled]). Fills the
// scene's part of k (blob, traversal switches, trap windows, where the shading records sit).
int choose_kernel(rt_scene *sc, const rt_camera &camera, const rt_params &P, bool moments, rt::KParams &k, KernelChoice &c)
{
    const rt_options &O = sc->opt;
    int variant = (P.flags & RT_FLAG_FAST_MATH) ? rt::V_FAST_LDS : rt::V_EXACT_LDS;
    bool cull = !(P.flags & RT_FLAG_BRUTE_FORCE) && sc->dev.meta[1].n_clusters > 0;
    const bool wave = (P.flags & RT_FLAG_WAVEFRONT) != 0u;
    if (wave && (P.flags & (RT_FLAG_FAST_MATH | RT_FLAG_SCALAR_SCENE)))
        return fail(RT_ERR_UNSUPPORTED, "rt_render_device: the wavefront variant is the exact kernel only");
    if (P.flags & RT_FLAG_SCALAR_SCENE) { variant = rt::V_EXACT_SCALAR; cull = false; }
    if (variant != rt::V_EXACT_SCALAR && static_cast<size_t>(sc->dev.meta[cull].shade_offset) * 16u + sc->static_lds[cull] > sc->max_lds) {
        if (variant == rt::V_FAST_LDS || cull) return fail(RT_ERR_UNSUPPORTED, "rt_render_device: scene too large for LDS");
        variant = rt::V_EXACT_SCALAR;
    }
    if (wave && variant != rt::V_EXACT_LDS)
        return fail(RT_ERR_UNSUPPORTED, "rt_render_device: the wavefront variant needs the scene in LDS");
    if (variant == rt::V_EXACT_LDS && (O.diag & RT_DIAG_STATS) && !wave) {
        variant = rt::V_STATS_LDS;
        if (!sc->dbg) {
            RT_HIP(sc->dbg.alloc(rt::kDbgWords * sizeof(unsigned long long)));
            RT_HIP(hipMemset(sc->dbg.get(), 0, rt::kDbgWords * sizeof(unsigned long long)));
        }
        k.dbg = sc->dbg.get();
    }
    const int b = cull ? 1 : 0;
    const int cull_mode = cull ? 7 : 0;
    fill_traversal(k, sc->dev, b);
    k.blob_units = sc->dev.meta[b].units;
    k.n_clusters = sc->dev.meta[b].n_clusters;
    k.use_root = (O.diag & RT_DIAG_NO_ROOT_BOX) ? 0u : 1u;
    k.iso = (O.diag & RT_DIAG_NO_SHORTCUT) ? 0u : 1u;
    k.transpose_max = O.transpose_max;
    k.diag_unbounded_nb = (O.diag & RT_DIAG_UNBOUNDED_NB) ? 1u : 0u;
    k.fast_roots = sc->dev.in_fast_range && camera_in_fast_range(camera) && !(O.diag & RT_DIAG_IEEE_ROOTS) ? 1u : 0u;
    // the windows hold for paths of at most rt::kTrapDepth segments: deeper renders get the empty set
    k.trap = reinterpret_cast<const float2 *>(sc->dev.trap.get()) +
             (P.max_depth > rt::kTrapDepth ? std::max<size_t>(sc->dev.n_spheres, 1u) : 0u);
    auto occ_for = [&](int in_lds, int *out) -> int {
        int &o = sc->occ.render[variant][b][in_lds];
        if (o < 0) {
            const size_t bytes = variant == rt::V_EXACT_SCALAR ? 0 : static_cast<size_t>(in_lds ? k.blob_units : k.shade_offset) * 16u;
            RT_HIP(rt::occupancy_render(variant, cull_mode, &o, bytes));
            o = std::max(o, 1);
        }
        *out = o;
        return RT_OK;
    };
    c.shade_fits = variant != rt::V_EXACT_SCALAR && static_cast<size_t>(k.blob_units) * 16u + sc->static_lds[b] <= sc->max_lds;
    ShadePlace place{};
    if (int rc = place_shade(O.diag, c.shade_fits, true, occ_for, place); rc) return rc;
    k.shade_lds = place.in_lds;
    k.lds_units = variant == rt::V_EXACT_SCALAR ? 0u : (k.shade_lds ? k.blob_units : k.shade_offset);
    c.variant = variant;
    c.cull_mode = cull_mode;
    c.cull = cull;
    c.wave = wave;
    c.lds = static_cast<size_t>(k.lds_units) * 16u;
    c.occ = c.occ_pr = place.occ;
    // (sample pairs, rt_plan.cpp: culled LDS kernels only; the variance render's samples must
    // reach the accumulation one by one)
    c.pairs_ok = !wave && cull_mode == 7 && variant != rt::V_EXACT_SCALAR && !(O.diag & RT_DIAG_NO_PAIRS) && !moments &&
                 c.lds + sc->static_lds_pairs <= sc->max_lds;
    // passes dealt by tile classes: the culled LDS kernels with a scene geometry to classify
    c.order_ok = sc->dev.has_geom && cull_mode == 7 && !wave && variant != rt::V_EXACT_SCALAR && !(O.diag & RT_DIAG_NATURAL_ORDER);
    return RT_OK;
}

// the pair instantiation's own occupancy (its parked colours add static LDS): the
// grid of a paired pass is sized by it
int pair_occupancy(rt_scene *sc, const rt::KParams &k, KernelChoice &c)
{
    if (!c.pairs_ok) return RT_OK;
    int &o = sc->occ.pairs[c.variant][k.shade_lds ? 1 : 0];
    if (o < 0) {
        RT_HIP(rt::occupancy_render(c.variant, c.cull_mode, &o, c.lds, true));
        o = std::max(o, 1);
    }
    c.occ_pr = o;
    return RT_OK;
}

// The split depth of a render with this camera key: rt_options.deep_split, unless a pass with
// this camera (and depth limit) has overflowed the deep queue on this scene: paths that long are
// common there (the corrected camera: 8.4% of the samples pass 8 segments, 59% of the segments),
// and a partial split only adds a tail. Takes the overflow reports the device left since the
// last call into sc->deep_off first.
uint32_t deep_split_for(rt_scene *sc, unsigned long long deep_key)
{
    for (uint32_t w = 0; w < kMaxWs; ++w) {
        // take-and-clear in one atomic step: a report the device writes meanwhile is kept
        const unsigned long long v = __atomic_exchange_n(sc->deep_over.get() + w, 0ull, __ATOMIC_ACQ_REL);
        if (!v) continue;
        auto it = std::find_if(sc->deep_off.begin(), sc->deep_off.end(), [&](const auto &e) { return e.first == v; });
        if (it != sc->deep_off.end()) sc->deep_off.erase(it);
        else if (sc->deep_off.size() >= rt_scene::kDeepOffKeys) sc->deep_off.erase(sc->deep_off.begin());
        sc->deep_off.emplace_back(v, sc->calls);  // most recent last
    }
    // reports expire: a camera is tried split again kDeepOffCalls calls after its last overflow
    sc->deep_off.erase(std::remove_if(sc->deep_off.begin(), sc->deep_off.end(),
                                      [&](const auto &e) { return sc->calls - e.second > rt_scene::kDeepOffCalls; }),
                       sc->deep_off.end());
    const bool deep_off = std::find_if(sc->deep_off.begin(), sc->deep_off.end(),
                                       [&](const auto &e) { return e.first == deep_key; }) != sc->deep_off.end();
    return deep_off ? 0u : sc->opt.deep_split;
}

// wavefront variant: two ray queues of cap rays (52 B each) and their counters, and the bounce
// kernel's grid
struct WaveQueues {
    uint32_t cap = 0;
    rt::RayQueue a{}, b{};
    int grid = 0;
};

// The plan's memory: under a cap, workspaces left larger (or more numerous) by earlier frames are
// re-cut once; then the multi-pass sums, the ring's slots, the lone passes' and the ray queues.
// (The deep queues are bound pass by pass, bind_deep_queue.) Records the cut for rt_scene_usage_get.
int reserve(rt_scene *sc, const Plan &pl, const KernelChoice &c, WaveQueues &wq, bool carried = false)
{
    const PlanInput &in = pl.in;
    const uint64_t per_sample = in.n_pixels * 12ull;
    // (carried: a window's sums live in its session's planes, whatever the number of its passes)
    const bool multi_pass = pl.ring_samples < in.spp && !carried;
    if (in.max_workspace_bytes) {
        uint64_t after = 0;
        for (uint32_t w = 0; w < kMaxWs; ++w) {
            const bool used = w < pl.n_ws || w == pl.lone_ws;
            after += used ? std::max<uint64_t>(sc->ws.slots[w].bytes(), pl.slot_bytes(w)) : sc->ws.slots[w].bytes();
            after += used && in.may_split ? std::max<uint64_t>(sc->ws.deep[w].bytes(), pl.deep_bytes(w)) : sc->ws.deep[w].bytes();
        }
        after += multi_pass ? std::max<uint64_t>(sc->ws.acc.bytes(), per_sample) : sc->ws.acc.bytes();
        after += multi_pass && in.moments ? std::max<uint64_t>(sc->ws.mom.bytes(), per_sample) : sc->ws.mom.bytes();
        after += in.wave ? std::max<uint64_t>(sc->ws.wq.bytes(), pl.wave_bytes()) : sc->ws.wq.bytes();
        if (after > in.max_workspace_bytes)
            if (int rc = sc->ws.release_all(); rc) return rc;
    }
    sc->used.streams = pl.streams;
    sc->used.ws = pl.n_ws + (pl.has_lone() ? 1u : 0u);
    sc->used.pass = static_cast<uint32_t>(pl.ring_samples);
    sc->used.deep = 0;
    sc->used.pairs = sc->used.split = sc->used.lead = sc->used.sky = 0;
    if (multi_pass)
        if (int rc = sc->ws.acc.ensure(per_sample); rc) return rc;
    if (multi_pass && in.moments)
        if (int rc = sc->ws.mom.ensure(per_sample); rc) return rc;
    for (uint32_t w = 0; w < pl.n_ws; ++w)
        if (int rc = sc->ws.slots[w].ensure(pl.slot_bytes(w)); rc) return rc;
    if (pl.has_lone())
        if (int rc = sc->ws.slots[pl.lone_ws].ensure(pl.slot_bytes(pl.lone_ws)); rc) return rc;
    if (in.wave) {
        wq.cap = pl.wave_cap;
        const size_t qbytes = static_cast<size_t>(wq.cap) * 52u;
        if (int rc = sc->ws.wq.ensure(2 * qbytes + 512); rc) return rc;
        auto carve = [&](char *base, rt::RayQueue &q) {
            q.f = reinterpret_cast<float *>(base);
            q.rng = reinterpret_cast<uint64_t *>(base + static_cast<size_t>(wq.cap) * 36u);
            q.item = reinterpret_cast<uint32_t *>(base + static_cast<size_t>(wq.cap) * 44u);
            q.depth = reinterpret_cast<uint32_t *>(base + static_cast<size_t>(wq.cap) * 48u);
        };
        char *w0 = sc->ws.wq.get();
        carve(w0, wq.a);
        carve(w0 + qbytes, wq.b);
        wq.a.count = reinterpret_cast<uint32_t *>(w0 + 2 * qbytes);
        wq.b.count = reinterpret_cast<uint32_t *>(w0 + 2 * qbytes + 256);
        int &ow = sc->occ.wave[c.cull ? 1 : 0];
        if (ow < 0) {
            RT_HIP(rt::occupancy_wave_bounce(c.cull_mode, &ow, c.lds));
            ow = std::max(ow, 1);
        }
        wq.grid = ow * sc->cu_count;
    }
    return RT_OK;
}

// What every pass of a call shares.
struct Frame {
    rt_scene *sc;
    const rt_params &P;
    hipStream_t st;  // the caller's stream
    float *d_rgb, *d_var;
    uint64_t *d_segments;
    KernelChoice c;
    Plan pl;  // (pl.in.may_split: the passes may have a deep queue)
    uint32_t deep_split;  // the split depth for this camera (0: none)
    unsigned long long deep_key;
    const Order *ord;  // the frame's dealing order, if any
    const WindowBlocks *blocks;  // a window over a block list: its own dealing order instead (ord stays null)
    bool sky_kernel;             // the proven-sky tiles are rendered by sky_kernel at the last pass
                                 // (a frame with moments: by sky_moments_kernel, at the call's last pass)
    uint32_t sky_pos0;           // the first pixel position of those tiles (n_pixels: none)
    // the ground tiles (the tiled blocks of the order's middle class, which come
    // before its untiled blocks) are rendered by ground_kernel pass by pass, the samples it punts
    // by the redo launch; positions [ground_pos0, ground_pos1)
    bool ground;
    uint32_t ground_pos0, ground_pos1;
    uint32_t ring;               // the call's slot in the timing events' ring
    // the call's samples [s_begin, s_end) of the frame's P.spp (a whole frame: all of them), and
    // the window's own planes (null: the scene's multi-pass sums)
    uint32_t s_begin, s_end;
    float *win_acc, *win_mom;
    // more than one render stream: passes rotate over sc->xs and the ring's workspaces
    bool pipe() const { return pl.streams > 1; }
};

// One render pass: samples [s0, s1) of every pixel.
struct Pass {
    uint32_t s0, s1;
    bool in_flight;   // another render still running (then this one takes a partial grid, grid_wg_per_cu)
    bool pass_pairs;  // its full blocks of 4 samples stored as pairs
    uint32_t wb;      // its workspace
    hipStream_t xst;  // its stream
    bool ordered;     // dealt by tile classes
    uint32_t grid;    // workgroups of the main launch
    bool two_part;    // the accumulation in two parts, the first beside the deep launch
    bool sky_aside;   // the sky kernel on another stream (then the accumulation waits for ev_sky)
    bool ground;      // its ground tiles go to ground_kernel (single samples, dealt by tile classes)
    bool ground_aside;  // ... on another stream (then the redo launch waits for ev_ground)
    uint32_t stats_waves;  // the instrumented build: waves of the launch the counters cover
};

unsigned long long *seg_counters(const rt_scene *sc, uint32_t wb)
{
    return reinterpret_cast<unsigned long long *>(sc->queue_ctr.get() + kSegWords) + 4u * wb;
}

// Every pass takes the next workspace and stream: pass p + 1's render overlaps pass p's drain
// and accumulation, within a frame and across frames; a whole lone frame, and a pass issued
// alone when the ring holds pairs, take the lone passes' workspace (single samples). The
// stream waits until the workspace is free, and the pass's counters are zeroed on it.
int begin_pass(const Frame &f, Pass &p, rt::KParams &k)
{
    rt_scene *sc = f.sc;
    const Plan &pl = f.pl;
    p.wb = 0;
    if (pl.has_lone() && ((p.s1 - p.s0) > pl.ring_samples || (pl.ring_pairs && !p.in_flight))) {
        p.wb = pl.lone_ws;
    } else if (f.pipe()) {
        p.wb = sc->next_buf % pl.n_ws;
        sc->next_buf = p.wb + 1u;
    }
    const uint32_t wb = p.wb;
    p.xst = f.pipe() ? sc->xs[wb % pl.streams].get() : f.st;
    k.slots = sc->ws.slots[wb].get();
    k.queue_ctr = sc->queue_ctr.get() + wb * 8u * rt::kQueueStride;
    unsigned long long *seg_b = seg_counters(sc, wb);
    k.segments = f.d_segments ? (f.pipe() ? seg_b : reinterpret_cast<unsigned long long *>(f.d_segments)) : nullptr;
    if (f.pipe() && sc->free_valid[wb]) RT_HIP(hipStreamWaitEvent(p.xst, sc->ev_free[wb].get(), 0));
    if (sc->ctr_dirty[wb]) {
        RT_HIP(hipMemsetAsync(k.queue_ctr, 0, 8 * rt::kQueueStride * sizeof(uint32_t), p.xst));
        RT_HIP(hipMemsetAsync(seg_b, 0, 3 * sizeof(unsigned long long), p.xst));
    }
    sc->ctr_dirty[wb] = true;
    if (p.s0 == f.s_begin) RT_HIP(hipEventRecord(sc->ev_begin[f.ring].get(), p.xst));
    k.sample_begin = p.s0;
    k.sample_end = p.s1;
    k.n_pair_items = static_cast<uint32_t>(((p.s1 - p.s0) - pl.slot_rows(p.s0, p.s1, p.pass_pairs)) * pl.in.n_pixels);
    if (k.n_pair_items) ++sc->used.pairs;
    return RT_OK;
}

// Whether a pass is split (bind_deep_queue): a pass of fewer than rt_options.deep_min_items samples
// issued alone is not, nor a lone pass dealt by tile classes under the lone_unsplit diagnostic.
bool pass_is_split(const Frame &f, const Pass &p, uint64_t n_samples)
{
    const rt_options &O = f.sc->opt;
    return f.pl.in.may_split && (n_samples >= O.deep_min_items || p.in_flight) &&
           (p.in_flight || !p.ordered || !(O.diag & RT_DIAG_LONE_UNSPLIT));
}

// The pass's items, its main launch's grid and its dealing groups: lead tiles
// first, then the others (then the proven sky tiles, unless the sky kernel renders them) in
// single-sample passes of the culled LDS kernels, else the natural order.
void deal_groups(const Frame &f, Pass &p, rt::KParams &k)
{
    rt_scene *sc = f.sc;
    const Order *ord = f.ord;
    const uint64_t n_pixels = k.n_pixels;  // (the pass's positions: under a block list fewer than the frame's pixels)
    const uint32_t s0 = p.s0, s1 = p.s1;
    const WindowBlocks *bl = f.blocks;
    const uint32_t *perm = bl ? bl->d_perm : ord ? ord->d_perm : nullptr;
    p.ordered = perm && !k.n_pair_items;
    fill_frame_consts(k);
    // items: the pass's pair items and its single tail samples (one slot each); with the sky
    // kernel, the positions before the sky tiles'
    const uint64_t n_samples = n_pixels * (s1 - s0);
    const uint64_t rows = f.pl.slot_rows(s0, s1, p.pass_pairs);
    // The ground kernel for split passes only: the few punted samples that meet a glass ball are
    // chains of up to max_depth segments, which a split pass hands to its deep launch; in an
    // unsplit one they would run in the redo launch, a serial tail behind the main launch (config
    // 3's 8-way share alone: 0.90-0.91 ms against 0.65-0.68)
    p.ground = f.ground && p.ordered && pass_is_split(f, p, n_pixels * (s1 - s0));
    const uint64_t ground_px = p.ground ? f.ground_pos1 - f.ground_pos0 : 0u;
    k.n_items = static_cast<uint32_t>(((p.ordered && f.sky_kernel ? f.sky_pos0 : n_pixels) - ground_px) * rows);
    k.n_slots = static_cast<uint32_t>(n_pixels * rows);
    int wg_cu = grid_wg_per_cu(p.pass_pairs ? f.c.occ_pr : f.c.occ, p.in_flight, f.pl.streams, n_samples);
    // A lone pass whose sky kernel runs beside it: the main launch's workgroups fill every
    // CU's registers (72 VGPRs x 7 waves per SIMD), so the sky kernel would start only as they
    // retire and end the frame after them. The main launch leaves room in proportion to the
    // sky's share of the pixels (config 3, 73% sky: 2 of 7 workgroups per CU; lone frame
    // 2.466-2.474 ms vs 2.528-2.547 with none, 2.474-2.495 with 1; period unchanged;
    // profiles/r06/ab/sky_room.txt). RT_LONE_SKY_ROOM >= 0 (A/B build switch) fixes it.
    // (with a ground kernel, which then runs beside it too: the share of both)
    if (!p.in_flight && f.sky_kernel && p.ordered && s1 == f.s_end && f.pipe() && !(sc->opt.diag & RT_DIAG_SKY_SERIAL)) {
        const double sky_frac = 1.0 - static_cast<double>(f.sky_pos0 - ground_px) / static_cast<double>(n_pixels);
        const int room = RT_LONE_SKY_ROOM >= 0 ? RT_LONE_SKY_ROOM : static_cast<int>(wg_cu * sky_frac * 0.4 + 0.5);
        wg_cu = std::max(1, wg_cu - room);
    }
    p.grid = static_cast<uint32_t>(
        std::max<uint64_t>(1, std::min<uint64_t>(static_cast<uint64_t>(wg_cu) * sc->cu_count, (k.n_items + 255u) / 256u)));
    k.n_blocks = (k.n_items + 63u) / 64u;
    k.guided_l2b = guided_l2b(p.grid * 4u, p.in_flight);
    k.block_perm = nullptr;
    k.n_groups = 1;
    k.grp_blocks[0] = k.n_blocks;
    k.grp_items[0] = k.n_items;
    k.grp_pix[0] = 0;
    k.grp_pix[1] = k.grp_pix[2] = k.grp_pix[3] = k.n_pixels;
    k.div_grp[0] = make_udiv(k.n_pixels);
    if (p.ordered) {
        // the order's lead and sky blocks and all of them: the frame's, or the block list's own
        rthost::tile_order t;
        t.n_lead = bl ? bl->cls[0] : ord->t.n_lead;
        t.n_sky = bl ? bl->cls[2] : ord->t.n_sky;
        const uint32_t n_ordered = bl ? bl->n_active : ord->n_blocks;
        const uint64_t S = s1 - s0;
        const uint64_t nbl[3] = {t.n_lead, n_ordered - t.n_lead - t.n_sky, f.sky_kernel ? 0u : t.n_sky};
        k.block_perm = perm;
#ifdef RT_ORDER_NULLPERM  // A/B build switch (with RT_ORDER_IDENTITY): the identity permutation not read
        k.block_perm = nullptr;
#endif
        k.n_groups = f.sky_kernel ? 2 : 3;
        for (int g = 0; g < 3; ++g) {
            k.grp_pix[g + 1] = k.grp_pix[g] + static_cast<uint32_t>(64u * nbl[g]);
            k.grp_items[g] = static_cast<uint32_t>(64u * nbl[g] * S);
            k.grp_blocks[g] = static_cast<uint32_t>(nbl[g] * S);  // nbl[g] blocks per sample
            k.div_grp[g] = make_udiv(static_cast<uint32_t>(std::max<uint64_t>(64u * nbl[g], 1u)));
        }
        if (p.ground) {
            // lead, (ground: no item), the untiled blocks; without untiled blocks the lead group alone
            const uint64_t n_ground = ground_px / 64u, n_rest = nbl[1] - n_ground;
            const uint64_t nb3[3] = {t.n_lead, 0u, n_rest};
            k.n_groups = n_rest ? 3 : 1;
            k.grp_pix[1] = f.ground_pos0;
            k.grp_pix[2] = f.ground_pos1;
            k.grp_pix[3] = f.sky_pos0;
            for (int g = 1; g < 3; ++g) {
                k.grp_items[g] = static_cast<uint32_t>(64u * nb3[g] * S);
                k.grp_blocks[g] = static_cast<uint32_t>(nb3[g] * S);
                k.div_grp[g] = make_udiv(static_cast<uint32_t>(std::max<uint64_t>(64u * nb3[g], 1u)));
            }
        }
        sc->used.lead = t.n_lead;
        sc->used.sky = f.sky_kernel ? t.n_sky : 0u;
    } else {
        sc->used.lead = sc->used.sky = 0;
    }
}

// deep-path split: this workspace's deep queue (its counters in the queue-counter block), for
// the passes that are split. Leaves k.deep_depth = 0 for the others.
int bind_deep_queue(const Frame &f, Pass &p, rt::KParams &k)
{
    rt_scene *sc = f.sc;
    const uint64_t n_pixels = k.n_pixels, n_samples = n_pixels * (p.s1 - p.s0);
    const uint32_t wb = p.wb;
    k.deep_depth = 0;
    k.deep_mode = 0;
    p.two_part = false;
    // (diag lone_unsplit: a lone pass dealt by tile classes is not split, its trapped paths
    // starting in its first items; slower, the accumulation then waits for the whole launch)
    if (!pass_is_split(f, p, n_samples)) return RT_OK;
    const uint32_t rcap = deep_region_cap(n_samples), cap = 8u * rcap;
    const size_t px_bytes = deep_px_bytes(n_pixels);
    bool fresh = false;
    if (int rc = sc->ws.deep[wb].ensure(deep_queue_bytes(n_pixels, n_samples), &fresh); rc)
        return rc;
    if (fresh) {  // new memory: no flag set, no pair arrival counted
        sc->ws.deep_clean[wb] = 0;
        RT_HIP(hipMemsetAsync(sc->ws.deep[wb].get(), 0, sc->ws.deep[wb].bytes(), p.xst));
    } else if (sc->ws.deep_meet_at[wb] != px_bytes + static_cast<size_t>(cap) * 56u) {
        // another layout: its arrival words lie where other arrays were (every pass that
        // keeps the layout leaves them zero: the second arrival of a pair resets its word)
        RT_HIP(hipMemsetAsync(sc->ws.deep[wb].get() + px_bytes + static_cast<size_t>(cap) * 56u, 0,
                              static_cast<size_t>(cap) * 4u, p.xst));
    }
    sc->ws.deep_meet_at[wb] = px_bytes + static_cast<size_t>(cap) * 56u;
    if (sc->ws.deep_clean[wb] < px_bytes)  // flags over bytes a queue may have used
        RT_HIP(hipMemsetAsync(sc->ws.deep[wb].get(), 0, px_bytes, p.xst));
    // every accumulation clears the flags its pass set, and the bytes past px_bytes are
    // this pass's queue storage: only the leading px_bytes are known to be zero after it
    sc->ws.deep_clean[wb] = px_bytes;
    char *base = sc->ws.deep[wb].get();
    k.deep.px = reinterpret_cast<uint8_t *>(base);
    base += px_bytes;
    k.deep.f = reinterpret_cast<float *>(base);
    k.deep.rng = reinterpret_cast<uint64_t *>(base + static_cast<size_t>(cap) * 36u);
    k.deep.slot = reinterpret_cast<uint32_t *>(base + static_cast<size_t>(cap) * 44u);
    k.deep.hid = reinterpret_cast<uint32_t *>(base + static_cast<size_t>(cap) * 48u);
    k.deep.link = reinterpret_cast<uint32_t *>(base + static_cast<size_t>(cap) * 52u);
    k.deep.meet = reinterpret_cast<uint32_t *>(base + static_cast<size_t>(cap) * 56u);
    k.deep.ctr = k.queue_ctr;
    k.deep.rcap = rcap;
    k.deep_depth = f.deep_split;
    p.two_part = RT_TWO_PART && f.pipe() && !p.in_flight;
    return RT_OK;
}

// wavefront variant: the pass's items in chunks of the queues' capacity: one generation launch,
// then max_depth bounce launches (each takes every ray of its input queue; continuing rays go
// to the other queue)
int launch_wavefront(const Frame &f, const Pass &p, const rt::KParams &k, const WaveQueues &wq)
{
    rt::KWave w{};
    w.p = k;
    w.cap = wq.cap;
    for (uint32_t c0 = 0; c0 < k.n_items; c0 += wq.cap) {
        w.item_begin = c0;
        w.n_chunk = std::min(wq.cap, k.n_items - c0);
        w.out = wq.a;
        RT_HIP(rt::launch_wave_gen(w, p.xst));
        rt::RayQueue qi = wq.a, qo = wq.b;
        for (uint32_t b = 0; b < std::max(1u, f.P.max_depth); ++b) {
            RT_HIP(hipMemsetAsync(qo.count, 0, sizeof(uint32_t), p.xst));
            w.in = qi;
            w.out = qo;
            RT_HIP(rt::launch_wave_bounce(f.c.cull_mode, w, static_cast<uint32_t>(wq.grid), p.xst));
            std::swap(qi, qo);
        }
    }
    return RT_OK;
}

// The workspace's ev_main (made by the first pass that needs one) after the pass's last launch so far.
hipError_t record_main(rt_scene *sc, const Pass &p)
{
    rthost::Event &ev = sc->ev_main[p.wb];
    const hipError_t e = ev.make(hipEventDisableTiming);
    return e == hipSuccess ? hipEventRecord(ev.get(), p.xst) : e;
}

// The main launch on the pass's stream, and ev_main after it where the first part of the
// accumulation waits for it alone.
int launch_main(const Frame &f, Pass &p, const rt::KParams &k)
{
    rt_scene *sc = f.sc;
    RT_HIP(rt::launch_render(f.c.variant, f.c.cull_mode, k, p.grid, p.xst));
    p.stats_waves = p.grid * 4u;
    if (p.two_part && !p.ground) {  // (with a ground kernel: after the redo launch)
        RT_HIP(record_main(sc, p));
    }
    return RT_OK;
}

// The ground kernel of a pass: the pass's samples of the ground tiles' pixels into
// their slots, the punted ones into the workspace's redo list (sized for every ground sample of
// the pass; its count words are the queue-counter block's, zeroed with it). Beside other renders
// it runs on the pass's stream before the main launch; a pass issued alone runs it on another
// render stream, beside the main launch (which leaves room for it and the sky kernel), after the
// pass's counters are zeroed (ev_gpre), and the redo launch waits for it (ev_ground).
#ifndef RT_GROUND_SPT
#define RT_GROUND_SPT 32u  // samples per thread of the ground kernel (A/B build switch)
#endif
#ifndef RT_GROUND_ASIDE
#define RT_GROUND_ASIDE 1  // A/B build switch: 0 runs the lone pass's ground kernel before its main launch
#endif
int launch_ground_tiles(const Frame &f, Pass &p, const rt::KParams &k, rt::RedoList &redo)
{
    rt_scene *sc = f.sc;
    const uint32_t wb = p.wb, n_pix = f.ground_pos1 - f.ground_pos0, S = p.s1 - p.s0;
    const uint64_t n_samples = static_cast<uint64_t>(n_pix) * S;
    if (int rc = sc->ws.redo[wb].ensure(n_samples * sizeof(uint32_t)); rc) return rc;
    if (!sc->redo_stat) {
        RT_HIP(sc->redo_stat.alloc(rt_scene::kRing * sizeof(uint32_t)));
        RT_HIP(hipMemset(sc->redo_stat.get(), 0, rt_scene::kRing * sizeof(uint32_t)));
    }
    if (sc->ground_call != sc->calls) {
        // the frame's first pass with a ground kernel (calls is the frame's own number, from 1):
        // the frame's slot of redo_stat; the slot half a ring ahead is zeroed for the frame that will
        // take it. Its last writer is 128 ground frames back, and at most kMaxWs passes are ever in
        // flight (begin_pass waits for the workspace's ev_free, recorded behind every earlier pass's
        // accumulation on the caller's stream), so that writer has long ended.
        sc->ground_call = sc->calls;
        sc->ground_ring = (sc->ground_ring + 1u) % rt_scene::kRing;
        sc->ground_samples = 0;
        RT_HIP(hipMemsetAsync(sc->redo_stat.get() + (sc->ground_ring + rt_scene::kRing / 2u) % rt_scene::kRing, 0, sizeof(uint32_t), p.xst));
    }
    sc->ground_samples += n_samples;
    redo = rt::RedoList{sc->ws.redo[wb].get(), k.queue_ctr, static_cast<uint32_t>(n_samples), sc->redo_stat.get() + sc->ground_ring};
    rt::KGround g{};
    g.fc = k.fc;
    g.block_perm = k.block_perm;
    g.pos0 = f.ground_pos0;
    g.n_pix = n_pix;
    g.n_samp = S;
    g.spt = RT_GROUND_SPT;
    g.n_wg = (n_pix + 63u) / 64u;
    g.slots = k.slots;
    g.n_slots = k.n_slots;
    g.blob = k.blob;
    g.n_geo = k.n_geo;
    g.n_always = k.n_always;
    g.n_supers = k.n_supers;
    g.supers_offset = k.supers_offset;
    g.shade_offset = k.shade_offset;
    g.n_spheres = k.n_spheres;
    g.fast_roots = k.fast_roots;
    g.clus_pad = k.clus_pad;
    g.redo = redo;
    g.segments = k.segments;
    g.dbg = k.dbg;
    p.ground_aside = RT_GROUND_ASIDE && f.pipe() && f.pl.streams >= 3u && !p.in_flight && !(sc->opt.diag & RT_DIAG_SKY_SERIAL);
    if (!p.ground_aside) {
        RT_HIP(rt::launch_ground(f.c.variant, g, p.xst));
        return RT_OK;
    }
    RT_HIP(sc->ev_gpre.make(hipEventDisableTiming));
    RT_HIP(sc->ev_ground.make(hipEventDisableTiming));
    // (the stream after the sky kernel's: consecutive render streams sit on different queues)
    hipStream_t g_st = sc->xs[(wb % f.pl.streams + 2u) % f.pl.streams].get();
    RT_HIP(hipEventRecord(sc->ev_gpre.get(), p.xst));
    RT_HIP(hipStreamWaitEvent(g_st, sc->ev_gpre.get(), 0));
    RT_HIP(rt::launch_ground(f.c.variant, g, g_st));
    RT_HIP(hipEventRecord(sc->ev_ground.get(), g_st));
    return RT_OK;
}

// The redo launch of a pass with a ground kernel: the punted samples from scratch through the
// general kernel's list instantiation, a fixed grid of one workgroup per CU (the count is on the
// device); its paths reach the deep queue like the main launch's.
int launch_redo(const Frame &f, const Pass &p, const rt::KParams &k, const rt::RedoList &redo)
{
    if (p.ground_aside) RT_HIP(hipStreamWaitEvent(p.xst, f.sc->ev_ground.get(), 0));
    const rt::KList kl{k, redo};
    rt_scene *sc = f.sc;
    RT_HIP(rt::launch_render_list(f.c.variant, kl, static_cast<uint32_t>(std::max(1, sc->cu_count)), p.xst));
    // the first part of the accumulation reads the ground tiles' slots too: ev_main after this launch
    if (p.two_part) {
        RT_HIP(record_main(sc, p));
    }
    return RT_OK;
}

// The deep launch of a split pass: the queued paths, same stream; the main launch's grid, or for
// a pass issued alone 8-wave workgroups with the shading records in LDS where that holds more waves.
int launch_deep(const Frame &f, Pass &p, const rt::KParams &k)
{
    rt_scene *sc = f.sc;
    const rt_options &O = sc->opt;
    const int variant = f.c.variant;
    ++sc->used.split;
    rt::KParams kd = k;
    kd.deep_mode = k.deep_depth;
    kd.deep_depth = 0;
    // the deep paths bounce inside glass spheres, inside the box over all clusters:
    // the level-3 gate only costs there (alike within box noise, fewer box tests;
    // same bits)
    kd.use_root = 0u;
#ifdef RT_DEEP_TMAX  // A/B build switch: every deep launch's transposition threshold
    kd.transpose_max = std::min<uint32_t>(O.transpose_max, RT_DEEP_TMAX);
#endif
    // its waves at the top issue priority: each path is a chain of ~56 dependent
    // iterations, and beside other renders' waves every iteration waits for the
    // SIMD's other waves (config 3's 8-way share, split, 7 streams: 0.513-0.515 ms vs
    // 0.569-0.571; profiles/r03/ab/deep_prio.txt)
    kd.deep_prio = 1u;
    // the shading records in LDS for the deep launch of a pass issued alone: its
    // paths bounce in glass and shade every segment, and its few busy waves wait on
    // each global round trip (config 3 single frame: deep launch 0.59 vs 0.65 ms).
    // Not beside other renders: its larger workgroups then displace theirs (frame
    // stream 2.69-2.73 vs 2.57-2.59 ms per frame, 8-way share 0.45 vs 0.42)
    int wpb = 4;
    uint32_t dgrid = p.grid;
    if (RT_DEEP_LDS_STAGE && !p.in_flight && variant != rt::V_EXACT_SCALAR && !k.shade_lds && f.c.shade_fits) {
        kd.shade_lds = 1u;
        kd.lds_units = k.blob_units;
        // 8-wave groups share the LDS copy (3 x 8 waves per CU instead of 3 x 4), the
        // grid is what is resident at once, and the chunks are dealt statically: the
        // launch was ~0.28 ms even for paths of one segment, most of it thousands of
        // waves probing the regions' counters and groups waiting for residency
        int &ow = sc->occ.deep_wide[variant];
        if (ow < 0) {
            const size_t bytes = static_cast<size_t>(k.blob_units) * 16u;
            size_t st8 = 0, st4 = 0;
            int o8 = 0, o4 = 0;
            RT_HIP(rt::deep_occupancy(variant, 8, bytes, &o8, &st8));
            // against the 4-wave deep kernel it replaces, with the same blob in LDS
            // (the main kernel's occupancy stood in for it)
            RT_HIP(rt::deep_occupancy(variant, 4, bytes, &o4, &st4));
            // (the instrumented kernel follows the product's choice: wide whenever it fits)
            ow = bytes + st8 <= sc->max_lds && (o8 * 8 > o4 * 4 || (variant == rt::V_STATS_LDS && o8 > 0)) ? o8 : 0;
        }
        if (RT_DEEP_WIDE && ow > 0) {
            wpb = 8;
            dgrid = static_cast<uint32_t>(ow * sc->cu_count);
            kd.deep_static = RT_DEEP_STATIC ? 1u : 0u;
            // its waves run alone on their SIMDs, so a cluster's transposed member
            // test (three LDS round trips) pays off for fewer requesting lanes: at
            // most 4 here (lone deep launch 0.351-0.360 vs 0.370-0.377 ms at 16;
            // 1-8 alike, per-lane tests always 0.400-0.405; profiles/r05/deep/
            // lone_deep_tmax.txt)
            kd.transpose_max = std::min<uint32_t>(O.transpose_max, RT_LONE_DEEP_TMAX);
        }
    }
    const bool stats_deep_only = variant == rt::V_STATS_LDS && (O.diag & RT_DIAG_STATS_DEEP_ONLY);
    if (stats_deep_only) {
        // diagnostics: the counters and events of the deep launch alone
        RT_HIP(hipMemsetAsync(sc->dbg.get(), 0, 16 * sizeof(unsigned long long), p.xst));
        RT_HIP(hipMemsetAsync(sc->dbg.get() + rt::kDbgEvBase, 0, rt::kDbgEvents * sizeof(unsigned long long), p.xst));
    }
    RT_HIP(rt::launch_render(variant, f.c.cull_mode, kd, dgrid, p.xst, wpb));
    sc->used.deep = static_cast<uint32_t>(wpb) | (kd.deep_static ? 16u : 0u);
    if (stats_deep_only) p.stats_waves = dgrid * static_cast<uint32_t>(wpb);
    return RT_OK;
}

// The sky kernel at the frame's last pass: the sky tiles' pixels, every sample of the frame;
// position i's sum to its sample-0 slot (which no pass of these groups uses), read by this
// pass's accumulation. A pass issued alone runs it on another stream, after the workspace is
// free, beside the main launch (which leaves it room) and the deep launch; beside other renders
// it follows the pass on its stream.
// A frame with moments (rt_options.sky_moments = 1): sky_moments_kernel at the call's
// last pass, the call's samples. A one-shot frame's sums go to the positions' sample-0 slots as
// above and {L_0, m1, m2} to their sample-1 slots (the workspace of a pass holds two rows at least:
// spp >= 2). A window's kernel reads and writes the session's planes, which until now only the
// caller's stream touched: it is ordered after everything that stream held when the call began
// (ev_enter: the previous step's sky kernel, accumulation and resolve), and the step's own
// accumulation and resolve follow it through ev_done or ev_sky like any pass's.
int launch_sky_tiles(const Frame &f, Pass &p, const rt::KParams &k)
{
    rt_scene *sc = f.sc;
    const uint32_t wb = p.wb;
    rt::KSkyMoments km{};
    rt::KSky &ks = km.sky;
    ks.fc = k.fc;
    ks.block_perm = k.block_perm;
    ks.pos0 = f.sky_pos0;
    ks.n_pix = k.n_pixels - f.sky_pos0;
    ks.sums = k.slots + 3u * static_cast<size_t>(f.sky_pos0);
    ks.segments = k.segments;
    const bool moments = f.d_var != nullptr, window = f.win_acc != nullptr;
    if (moments) {
        km.s_a = f.s_begin;
        km.s_b = f.s_end;
        km.natural = window ? 1u : 0u;
        km.acc = window ? f.win_acc : ks.sums;
        km.mom = window ? f.win_mom : ks.sums + 3u * static_cast<size_t>(k.n_pixels);
        ks.sums = nullptr;
        if (!window && sc->ws.slots[wb].bytes() < 2u * 12u * static_cast<uint64_t>(k.n_pixels))
            return fail(RT_ERR_CAPACITY, "rt_render_var_device: the last pass's workspace holds no second slot row");
    }
    auto launch = [&](hipStream_t s) -> int {
        if (moments && window && s != f.st) RT_HIP(hipStreamWaitEvent(s, sc->ev_enter.get(), 0));
        RT_HIP(moments ? rt::launch_sky_moments(km, s) : rt::launch_sky(ks, s));
        return RT_OK;
    };
    p.sky_aside = f.pipe() && !p.in_flight && !(sc->opt.diag & RT_DIAG_SKY_SERIAL);
    if (!p.sky_aside) return launch(p.xst);
    // the next render stream, not a stream of its own: HIP maps streams to hardware
    // queues round-robin in creation order, and a ninth stream shared a queue with one
    // of the render streams, behind whose main launch the sky kernel then waited (one
    // lone frame in three at 4 queues: 0.83 vs 0.69 ms on the 8-way share). Consecutive
    // render streams sit on different queues.
    hipStream_t sky_st = sc->xs[(wb % f.pl.streams + 1u) % f.pl.streams].get();
    if (sc->free_valid[wb]) RT_HIP(hipStreamWaitEvent(sky_st, sc->ev_free[wb].get(), 0));
    // (the counters it adds to are this pass's: zeroed on xst before the main launch)
    if (ks.segments) {
        if (!p.two_part) RT_HIP(record_main(sc, p));
        RT_HIP(hipStreamWaitEvent(sky_st, sc->ev_main[wb].get(), 0));
    }
    if (int rc = launch(sky_st); rc) return rc;
    RT_HIP(hipEventRecord(sc->ev_sky.get(), sky_st));
    return RT_OK;
}

// The pass's samples into the frame on the caller's stream, after the pass's stream (and the sky
// kernel's); then the workspace is free again.
int accumulate(const Frame &f, const Pass &p, const rt::KParams &k)
{
    rt_scene *sc = f.sc;
    const rt_params &P = f.P;
    const uint32_t wb = p.wb, s0 = p.s0, s1 = p.s1;
    const uint32_t full_blocks_end = P.spp & ~3u;  // samples [0, full_blocks_end) form blocks of 4
    rt::KAccum a{};
    a.slots = sc->ws.slots[wb].get();
    a.acc = f.win_acc ? f.win_acc : sc->ws.acc.get();
    a.out = f.d_rgb;
    a.out_u8 = nullptr;
    a.mom = f.win_mom ? f.win_mom : sc->ws.mom.get();
    a.var = f.d_var;
    a.n_pixels = k.n_pixels;
    a.n_samples = s1 - s0;
    a.n_blocks = (std::min(s1, full_blocks_end) - std::min(s0, full_blocks_end)) / 4u;
    a.paired = k.n_pair_items ? 1u : 0u;
    a.first = s0 == 0;
    a.last = s1 == P.spp && !f.win_acc;
    a.spp = P.spp;
    a.W = P.width;
    a.tiles_x = k.tiles_x;
    a.tiled_rows = k.tiled_rows;
    a.tile_lw = k.tile_lw;
    a.row_offset = k.row_offset;
    a.row_stride = k.row_stride;
    a.full_frame = k.full_frame;
    if (f.pipe() && f.d_segments) a.seg_from = seg_counters(sc, wb), a.seg_to = reinterpret_cast<unsigned long long *>(f.d_segments);
    a.queue_reset = k.queue_ctr;
    a.queue_words = 8 * rt::kQueueStride;
    a.block_perm = k.block_perm;
    a.sky_pos0 = f.sky_pos0;
    if (k.deep_depth) {
        a.deep_over = sc->deep_over_dev + wb;
        a.deep_key = f.deep_key;
        a.deep_rcap = k.deep.rcap;
    }
    if (p.two_part) {
        // a pass issued while no other render runs (a lone frame, the first of a stream):
        // the pixels without deep samples accumulate beside the deep launch, the others (and
        // the counters) after it. In a frame stream the other frames' work fills that time,
        // and the extra launch per pass measured ~1% slower there.
        rt::KAccum a1 = a;
        a1.seg_from = a1.seg_to = nullptr;
        a1.queue_reset = nullptr;
        a1.deep_over = nullptr;
        a1.deep_px = k.deep.px;
        a1.part = 1;
        RT_HIP(hipStreamWaitEvent(f.st, sc->ev_main[wb].get(), 0));
        RT_HIP(rt::launch_accumulate(a1, f.st));
        a.deep_px = k.deep.px;
        a.part = 2;
    } else if (k.deep_depth) {
        a.deep_px = k.deep.px;  // one part; clears the flags the main launch set
        a.part = 3;
    }
    if (f.pipe()) RT_HIP(hipStreamWaitEvent(f.st, sc->ev_done[wb].get(), 0));
    if (p.sky_aside) RT_HIP(hipStreamWaitEvent(f.st, sc->ev_sky.get(), 0));
    RT_HIP(rt::launch_accumulate(a, f.st));
    sc->ctr_dirty[wb] = false;
    if (f.pipe()) {
        RT_HIP(hipEventRecord(sc->ev_free[wb].get(), f.st));
        sc->free_valid[wb] = true;
    }
    return RT_OK;
}

// d_var (rt_render_var_device): the frame also yields the variance of each pixel's
// mean luminance. Its samples' colours must reach the accumulation one by one, so it is planned as
// under RT_DIAG_NO_PAIRS whatever the scene's options say, and as under RT_DIAG_NO_SKY unless
// rt_options.sky_moments = 1: then sky_moments_kernel renders the proven-sky tiles, folding each
// colour into the pixel's moments itself.
int render_device_impl(rt_scene *sc, const rt_camera *camera, const rt_params &P, float *d_rgb, hipStream_t st,
                       uint64_t *d_segments, float *d_var, const Window *win)
{
    // (a window: launch_accumulate takes the moments kernel where KAccum::var is set, and no pass of
    // a window writes through it or through d_rgb)
    if (win) d_var = win->mom;
    const bool moments = d_var != nullptr;
    rt::KParams k{};
    if (int rc = frame_params(sc, camera, P, k, "rt_render_device"); rc) return rc;
    if (k.n_pixels == 0) return RT_OK;
    // A window over a block list: from here on k.n_pixels counts the pass's positions, 64 per listed
    // block. Everything below that takes it (the plan, FrameConsts::n_pixels and its divisor, the
    // slots, the deep queue's pixel flags, KAccum::n_pixels, sky_pos0) means positions of the pass;
    // what places a pixel in the frame (W, tiles_x, tiled_rows, tile_lw, the row fields) stays the
    // frame's, and the running sums are indexed by the natural index the permutation yields.
    const WindowBlocks *blocks = win ? win->blocks : nullptr;
    if (blocks) {
        if (!blocks->d_perm || static_cast<uint64_t>(blocks->n_active) * 64u > k.n_pixels ||
            static_cast<uint64_t>(blocks->cls[0]) + blocks->cls[1] + blocks->cls[2] != blocks->n_active)
            return fail(RT_ERR_INVALID, "render_window: bad block list");
        k.n_pixels = 64u * blocks->n_active;
        if (k.n_pixels == 0) return RT_OK;
    }
    const rt_options &O = sc->opt;
    Frame f{sc, P, st, d_rgb, d_var, d_segments};
    f.blocks = blocks;
    const KernelChoice &c = f.c;
    const Plan &pl = f.pl;

    // the kernel, and whether this camera's passes are split (culled scenes only: with a handful
    // of spheres (the simple scene, brute force) a deep segment is cheap and the deep launch's
    // overhead outweighs the drain it saves; config 2: 0.98-1.00 vs 0.98-0.99 ms per frame)
    if (int rc = choose_kernel(sc, *camera, P, moments, k, f.c); rc) return rc;
    f.deep_key = camera_key(*camera, P.max_depth);
    f.deep_split = deep_split_for(sc, f.deep_key);
    const bool may_split = f.deep_split && !c.wave && c.cull_mode == 7 && f.deep_split < P.max_depth;
    if (int rc = pair_occupancy(sc, k, f.c); rc) return rc;

    // the cut of the call's samples (rt_plan.cpp; a window's: passes of a multiple of 4 from its
    // first sample, itself one), then its memory
    const uint32_t s_begin = win ? win->a : 0u, s_end = win ? win->b : P.spp;
    const PlanInput in{k.n_pixels, s_end - s_begin, c.wave ? 1u : render_streams_of(O),  // the wavefront variant: caller stream only
                       O.workspaces_per_stream, O.max_pass_bytes, O.max_workspace_bytes, O.ring_pass_bytes, O.wave_queue_rays,
                       c.wave, moments, c.pairs_ok, (O.diag & RT_DIAG_PAIRS) != 0u, may_split};
    if (int rc = plan_frame(in, f.pl); rc) return rc;
    WaveQueues wq;
    if (int rc = reserve(sc, pl, c, wq, win != nullptr); rc) return rc;

    // the frame's dealing order (not with sample pairs) and the sky kernel: the
    // tiles proven to send every primary ray to the sky are rendered by sky_kernel at the frame's
    // last pass (all samples, one thread per pixel, no slots), the passes deal the others
    // (a block list is its own order, whatever the scene and the flags: the identity's where they have none)
    if (c.order_ok && !pl.pairs && !blocks)
        if (int rc = pass_order(sc, *camera, k, st, &f.ord); rc) return rc;
    // (max_depth 0: every sample's colour is 0, main.cxx:74, not the sky's)
    // (a frame with moments: under rt_options.sky_moments = 1 alone, by sky_moments_kernel; a block
    // list is the order then, its sky blocks last)
    const uint32_t n_ordered = blocks ? blocks->n_active : f.ord && f.ord->d_perm ? f.ord->n_blocks : 0u;
    const uint32_t n_sky = blocks ? blocks->cls[2] : f.ord && f.ord->d_perm ? f.ord->t.n_sky : 0u;
    f.sky_kernel = n_sky && P.max_depth > 0 && !(O.diag & RT_DIAG_NO_SKY) && (!moments || O.sky_moments == 1u);
    f.sky_pos0 = f.sky_kernel ? static_cast<uint32_t>(64u * static_cast<uint64_t>(n_ordered - n_sky)) : k.n_pixels;
    // the ground tiles: the order's middle class is its tiled blocks of class 1,
    // in ascending order, then the untiled blocks (class 1 too, numbered after every tile)
    f.ground = false;
    f.ground_pos0 = f.ground_pos1 = f.sky_pos0;
#ifndef RT_NO_GROUND  // A/B build switch: every pass as before the ground kernel
    // (f.sky_kernel: a culled LDS kernel dealt by tile classes, single samples, no_sky unset; the ground
    // kernel stays out of frames with moments, whichever kernel renders their sky)
    if (f.sky_kernel && !moments && sc->dev.ground_ok && ground_pass_ok(O, P)) {
        const uint32_t n_ground = ground_blocks(f.ord->n_blocks, f.ord->t.n_lead, f.ord->t.n_sky, k.W, k.num_rows, k.tile_lw);
        f.ground = n_ground != 0u;
        f.ground_pos0 = 64u * f.ord->t.n_lead;
        f.ground_pos1 = f.ground_pos0 + 64u * n_ground;
    }
#endif
    f.ring = static_cast<uint32_t>(sc->calls % rt_scene::kRing);
    ++sc->calls;
    f.s_begin = s_begin, f.s_end = s_end;
    f.win_acc = win ? win->acc : nullptr, f.win_mom = win ? win->mom : nullptr;
    if (win && f.sky_kernel && f.pipe()) {
        RT_HIP(sc->ev_enter.make(hipEventDisableTiming));
        RT_HIP(hipEventRecord(sc->ev_enter.get(), st));
    }

    auto others_running = [&] { return f.pipe() && sc->last_ws >= 0 && hipEventQuery(sc->ev_done[sc->last_ws].get()) == hipErrorNotReady; };
    // a frame issued alone that fits one pass takes it whole (Plan::whole); otherwise ring passes
    const uint64_t first_pass =
        pl.whole && !others_running() && !(O.diag & RT_DIAG_IN_FLIGHT) ? pl.lone_samples : pl.ring_samples;
    for (uint32_t s0 = s_begin, s1 = s_begin; s0 < s_end; s0 = s1) {
        s1 = static_cast<uint32_t>(std::min<uint64_t>(s_end, s0 + (s0 == s_begin ? first_pass : pl.ring_samples)));
        Pass p{s0, s1};
        p.in_flight = others_running() || (f.pipe() && (O.diag & RT_DIAG_IN_FLIGHT));
        p.pass_pairs = pl.ring_pairs && p.in_flight;
        if (int rc = begin_pass(f, p, k); rc) return rc;
        deal_groups(f, p, k);
        if (int rc = bind_deep_queue(f, p, k); rc) return rc;
        if (O.diag & RT_DIAG_VERBOSE)
            std::fprintf(stderr, "[rt] variant=%d cull=%d shade_lds=%u lds=%zu B occ=%d WG/CU cus=%d grid=%u items=%u "
                                 "samples=[%u,%u) streams=%u workspaces=%u split=%u guided log2(beta)*1e6=%u\n",
                         c.variant, c.cull_mode, k.shade_lds, c.lds, c.occ, sc->cu_count, p.grid, k.n_items, s0, s1, pl.streams,
                         pl.n_ws, k.deep_depth, static_cast<uint32_t>(-k.guided_l2b * 1e6f));
        if (c.wave) {
            if (int rc = launch_wavefront(f, p, k, wq); rc) return rc;
        } else {
            rt::RedoList redo{};
            if (p.ground)
                if (int rc = launch_ground_tiles(f, p, k, redo); rc) return rc;
            if (int rc = launch_main(f, p, k); rc) return rc;
            if (p.ground)
                if (int rc = launch_redo(f, p, k, redo); rc) return rc;
            if (k.deep_depth)
                if (int rc = launch_deep(f, p, k); rc) return rc;
        }
        if (f.sky_kernel && s1 == s_end)
            if (int rc = launch_sky_tiles(f, p, k); rc) return rc;
        if (c.variant == rt::V_STATS_LDS) sc->dbg_waves = p.stats_waves;
        if (s1 == s_end) RT_HIP(hipEventRecord(sc->ev_end[f.ring].get(), p.xst));
        if (f.pipe()) {
            RT_HIP(hipEventRecord(sc->ev_done[p.wb].get(), p.xst));
            sc->last_ws = static_cast<int>(p.wb);
        }
        if (int rc = accumulate(f, p, k); rc) return rc;
    }
    // (every launch above that reads the order's permutation is ordered before st's tail)
    return order_used(sc, f.ord, st);
}

// The first window of an adaptive session: the dealing order the frame's own window would take
// (pass_order's for this camera and rows where the kernel choice deals by tile classes, else the
// identity), handed to the session, which enqueues its copy on `st`; the cached order is then marked
// as read up to st's tail, so its pool slot is not recycled under that copy.
int window_first_order(rt_scene *sc, const rt_camera *camera, const rt_params &P, hipStream_t st, WindowBlocks &blocks)
{
    rt::KParams k{};
    if (int rc = frame_params(sc, camera, P, k, "render_window"); rc) return rc;
    KernelChoice c{};
    if (int rc = choose_kernel(sc, *camera, P, true, k, c); rc) return rc;
    const Order *ord = nullptr;
    if (c.order_ok)
        if (int rc = pass_order(sc, *camera, k, st, &ord); rc) return rc;
    const bool ordered = ord && ord->d_perm;
    if (int rc = blocks.first(ordered ? ord->d_perm : nullptr, ordered ? ord->t.n_lead : 0u, ordered ? ord->t.n_sky : 0u); rc) return rc;
    blocks.first = nullptr;
    // the window's passes run on the render streams, which nothing else orders behind st's work
    RT_HIP(sc->ev_blocks.make(hipEventDisableTiming));
    RT_HIP(hipEventRecord(sc->ev_blocks.get(), st));
    for (const rthost::Stream &x : sc->xs)
        if (x) RT_HIP(hipStreamWaitEvent(x.get(), sc->ev_blocks.get(), 0));
    return order_used(sc, ord, st);
}

int render_compat(rt_scene *sc, const rt_camera *camera, const rt_params &P, float *d_rgb, hipStream_t st,
                  uint64_t *d_segments)
{
    rt::KCompat k{};
    for (int c = 0; c < 3; ++c) {
        k.org[c] = camera->origin[c];
        k.llc[c] = camera->lower_left_corner[c];
        k.hor[c] = camera->horizontal[c];
        k.ver[c] = camera->vertical[c];
    }
    k.W = P.width;
    k.H = P.height;
    k.spp = P.spp;
    k.max_depth = P.max_depth;
    k.row_offset = P.row_offset;
    k.row_stride = P.row_stride ? P.row_stride : 1;
    k.num_rows = rows_of(P);
    k.full_frame = (P.flags & RT_FLAG_FULL_FRAME) ? 1u : 0u;
    k.seed = static_cast<uint32_t>(P.seed);
    k.n_spheres = sc->dev.n_spheres;
    const uint64_t n_pixels = static_cast<uint64_t>(P.width) * k.num_rows;
    if (n_pixels == 0) return RT_OK;
    if (n_pixels >= (1ull << 31)) return fail(RT_ERR_INVALID, "rt_render_device: more than 2^31 pixels in one call");
    k.n_pixels = static_cast<uint32_t>(n_pixels);
    k.n_chunks = (k.n_pixels + 63u) / 64u;
    k.shade = reinterpret_cast<const float4 *>(sc->dev.blob[0].get()) + sc->dev.meta[0].shade_offset;
    k.out = d_rgb;
    k.ctr = sc->queue_ctr.get() + kCompatCtr;
    k.segments = reinterpret_cast<unsigned long long *>(d_segments);
    int occ = 0;
    RT_HIP(rt::occupancy_compat(&occ));
    const uint32_t grid = static_cast<uint32_t>(
        std::max<uint64_t>(1, std::min<uint64_t>(static_cast<uint64_t>(std::max(occ, 1)) * sc->cu_count, (n_pixels + 255u) / 256u)));
    const uint32_t ring = static_cast<uint32_t>(sc->calls % rt_scene::kRing);
    ++sc->calls;
    RT_HIP(hipMemsetAsync(k.ctr, 0, sizeof(uint32_t), st));
    RT_HIP(hipEventRecord(sc->ev_begin[ring].get(), st));
    RT_HIP(rt::launch_compat(k, grid, st));
    RT_HIP(hipEventRecord(sc->ev_end[ring].get(), st));
    return RT_OK;
}

// The first-hit feature buffers: one launch of aov_kernel on the caller's
// stream, the pass's blocks in its dealing order (pass_order) so that the blocks proven sky skip
// the closest-hit test. It reads the scene and the order's permutation and writes the caller's
// planes: no workspace, nothing that grows with the samples.
int render_aov_impl(rt_scene *sc, const rt_camera *camera, const rt_params &P, const rt_aov_buffers &A, hipStream_t st)
{
    rt::KParams k{};
    if (int rc = frame_params(sc, camera, P, k, "rt_render_aov_device"); rc) return rc;
    if (k.n_pixels == 0) return RT_OK;
    fill_frame_consts(k);
    const rt_options &O = sc->opt;
    const bool cull = !(P.flags & RT_FLAG_BRUTE_FORCE) && sc->dev.meta[1].n_clusters > 0;
    const int b = cull ? 1 : 0, cull_mode = cull ? 7 : 0;
    if (sc->static_lds_aov[b] == ~static_cast<size_t>(0)) RT_HIP(rt::static_lds_aov(cull_mode, &sc->static_lds_aov[b]));
    const size_t static_lds = sc->static_lds_aov[b];
    if (static_cast<size_t>(sc->dev.meta[b].shade_offset) * 16u + static_lds > sc->max_lds)
        return fail(RT_ERR_UNSUPPORTED, "rt_render_aov_device: scene too large for LDS");
    rt::KAov a{};
    a.fc = k.fc;
    a.samples = A.samples ? A.samples : P.spp;
    a.full_frame = k.full_frame;
    a.n_blocks = (k.n_pixels + 63u) / 64u;
    fill_traversal(a, sc->dev, b);
    a.use_root = (O.diag & RT_DIAG_NO_ROOT_BOX) ? 0u : 1u;
    a.transpose_max = O.transpose_max;
    a.fast_roots = sc->dev.in_fast_range && camera_in_fast_range(*camera) && !(O.diag & RT_DIAG_IEEE_ROOTS) ? 1u : 0u;
    // the shading records join the geometry in LDS by the render kernels' rule (place_shade)
    auto occ_for = [&](int in_lds, int *out) -> int {
        int &o = sc->occ.aov[b][in_lds];
        if (o < 0) {
            RT_HIP(rt::occupancy_aov(cull_mode, &o, static_cast<size_t>(in_lds ? sc->dev.meta[b].units : sc->dev.meta[b].shade_offset) * 16u));
            o = std::max(o, 1);
        }
        *out = o;
        return RT_OK;
    };
    const bool shade_fits = static_cast<size_t>(sc->dev.meta[b].units) * 16u + static_lds <= sc->max_lds;
    ShadePlace place{};
    if (int rc = place_shade(O.diag, shade_fits, false, occ_for, place); rc) return rc;
    a.shade_lds = place.in_lds;
    a.lds_units = a.shade_lds ? sc->dev.meta[b].units : sc->dev.meta[b].shade_offset;
    const int occ = place.occ;
    // the dealing order and its proven-sky blocks, under the beauty's conditions for sky_kernel
    const Order *ord = nullptr;
    if (sc->dev.has_geom && cull && !(O.diag & RT_DIAG_NATURAL_ORDER))
        if (int rc = pass_order(sc, *camera, k, st, &ord); rc) return rc;
    a.block_perm = ord ? ord->d_perm : nullptr;
    const bool sky = a.block_perm && ord->t.n_sky && !(O.diag & RT_DIAG_NO_SKY);
    a.sky_block0 = sky ? ord->n_blocks - ord->t.n_sky : a.n_blocks;
    a.albedo = A.albedo;
    a.normal = A.normal;
    a.depth = A.depth;
    a.alpha = A.alpha;
    a.sphere_id = A.sphere_id;
    const uint32_t grid = static_cast<uint32_t>(
        std::max<uint64_t>(1, std::min<uint64_t>(static_cast<uint64_t>(occ) * sc->cu_count, (a.n_blocks + 3u) / 4u)));
    if (O.diag & RT_DIAG_VERBOSE)
        std::fprintf(stderr, "[rt] aov cull=%d shade_lds=%u lds=%zu B occ=%d WG/CU cus=%d grid=%u blocks=%u sky_blocks=%u "
                             "ordered=%d samples=%u of %u\n",
                     cull_mode, a.shade_lds, static_cast<size_t>(a.lds_units) * 16u, occ, sc->cu_count, grid, a.n_blocks,
                     a.n_blocks - a.sky_block0, a.block_perm ? 1 : 0, a.samples, P.spp);
    RT_HIP(rt::launch_aov(cull_mode, a, grid, st));
    return order_used(sc, ord, st);
}
} // namespace

extern "C" {

int rt_render_aov_device(rt_scene *sc, const rt_camera *camera, const rt_params *params, const rt_aov_buffers *aov,
                         void *stream)
{
    if (int rc = check_aov(params, aov, "rt_render_aov_device"); rc != RT_OK) return rc;
    if (!sc || !camera) return fail(RT_ERR_INVALID, "rt_render_aov_device: null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    RT_HIP(hipSetDevice(sc->device));
    if (int rc = stream_enter(sc, st); rc != RT_OK) return rc;
    if (int rc = render_aov_impl(sc, camera, *params, *aov, st); rc != RT_OK) return rc;
    return stream_leave(sc, st);
}

int rt_epilogue_rgb8_device(const float *d_rgb, uint8_t *d_out, uint64_t n_pixels, void *stream)
{
    if (!d_rgb || !d_out) return fail(RT_ERR_INVALID, "rt_epilogue_rgb8_device: null argument");
    if (!n_pixels) return RT_OK;
    RT_HIP(rt::launch_epilogue(d_rgb, d_out, n_pixels * 3u, static_cast<hipStream_t>(stream)));
    return RT_OK;
}

} // extern "C"
