// rt_host_post.cpp — the post-process stages of the C-ABI (include/rt_api.h), which use nothing of
// a device scene: the à-trous denoiser, its variance-guided form, temporal accumulation and the
// guided upsample, each with its argument checks, defaults, level driver, stream-ordered *_device
// entry point and the synchronous host-plane call through the cached context (rt_host_sync.h
// SyncCall); and the preview session, which runs those stages after a scene's render calls, one
// frame per call, and the progressive session, which runs a frame's render in sample windows. The
// kernels are rt_denoise.hip, rt_temporal.hip, rt_upsample.hip, rt_preview.hip and rt_progressive.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>

#include "../../include/rt_api.h"
#include "rt_device.h"
#include "rt_hip_own.h"
#include "rt_host_build.h"
#include "rt_host_sync.h"

using namespace rthost;

namespace {

// ---- the à-trous denoiser (include/rt_api.h; kernels in rt_denoise.hip) ----------------------
// Levels with a step up to this take the tiled kernel: at 1280x720 with every guide it takes 0.77
// of the direct kernel's time at steps 1 and 2 and 1.03 at step 4, where its halo is as large as
// its tile (profiles/denoise/time_c3.txt). Its LDS image at step 2 is 37.5 KiB.
constexpr uint32_t kDenoiseTiledMaxStep = 2;
// The largest step the tiled kernel can take at all (rt_denoise_level_device's A/B): its LDS image
// with every guide is then 60 KiB, the most a launch gets without asking for more.
constexpr uint32_t kDenoiseTiledFits = 4;
constexpr uint32_t kDenoiseMaxSide = 65536;
// rt_denoise_var_params_default: the values scripts/denoise_var_sweep.py chose
constexpr uint32_t kDnVarLevels = 2;
constexpr float kDnVarSigmaColor = 32.0f, kDnVarSigmaNormal = 1.0f, kDnVarSigmaDepth = 4.0f, kDnVarSigmaAlbedo = 1.0f;
constexpr float kDnVarFloor = 1e-6f;

// The checks of a filter's params that read nothing but the record's own values, in two parts (the
// checks of the planes come between them). w: the message up to the field's name ("rt_denoise: ",
// or "rt_preview_create: denoise." for the session's sub-record).
struct Sigma { const char *name; float v; };
int check_denoise_ranges(const rt_denoise_params &p, const std::string &w)
{
    if (!p.width || p.width > kDenoiseMaxSide) return fail(RT_ERR_INVALID, w + "width must be 1..65536");
    if (!p.height || p.height > kDenoiseMaxSide) return fail(RT_ERR_INVALID, w + "height must be 1..65536");
    if (p.levels < 1u || p.levels > 6u) return fail(RT_ERR_INVALID, w + "levels must be 1..6");
    for (const Sigma &s : {Sigma{"sigma_color", p.sigma_color}, Sigma{"sigma_normal", p.sigma_normal},
                           Sigma{"sigma_depth", p.sigma_depth}, Sigma{"sigma_albedo", p.sigma_albedo}})
        if (!std::isfinite(s.v) || s.v < 0.f) return fail(RT_ERR_INVALID, w + s.name + " must be finite and not negative");
    return RT_OK;
}
int check_denoise_small(const rt_denoise_params &p, const std::string &w)
{
    if (p.sigma_color != 0.f) {
        const float s = p.sigma_color * std::ldexp(1.f, -static_cast<int>(p.levels - 1u));
        if (!std::isfinite(1.0f / (s * s))) return fail(RT_ERR_INVALID, w + "sigma_color is too small for this many levels");
    }
    for (const Sigma &s : {Sigma{"sigma_normal", p.sigma_normal}, Sigma{"sigma_depth", p.sigma_depth},
                           Sigma{"sigma_albedo", p.sigma_albedo}})
        if (s.v != 0.f && !std::isfinite(1.0f / (s.v * s.v))) return fail(RT_ERR_INVALID, w + s.name + " is too small");
    return RT_OK;
}

// Every argument check of the denoiser, before any HIP call (use_scratch: the call uses
// buffers.scratch). terms: the edge terms that are on.
int check_denoise(const rt_denoise_params *p, const rt_denoise_buffers *b, bool use_scratch, const char *who,
                  uint32_t *terms)
{
    const std::string w = std::string(who) + ": ";
    if (!p || !b) return fail(RT_ERR_INVALID, w + "null argument");
    if (p->size != sizeof(rt_denoise_params)) return fail(RT_ERR_INVALID, w + "params.size is not sizeof(rt_denoise_params)");
    if (b->size != sizeof(rt_denoise_buffers)) return fail(RT_ERR_INVALID, w + "buffers.size is not sizeof(rt_denoise_buffers)");
    if (int rc = check_denoise_ranges(*p, w); rc != RT_OK) return rc;
    if (p->flags & ~static_cast<uint32_t>(RT_DENOISE_DEMODULATE | RT_DENOISE_DIRECT))
        return fail(RT_ERR_INVALID, w + "unknown bits in flags");
    if (!b->beauty) return fail(RT_ERR_INVALID, w + "beauty is null");
    if (!b->out) return fail(RT_ERR_INVALID, w + "out is null");
    if (b->normal && p->sigma_normal == 0.f) return fail(RT_ERR_INVALID, w + "sigma_normal is 0 with a normal plane");
    if (b->depth && p->sigma_depth == 0.f) return fail(RT_ERR_INVALID, w + "sigma_depth is 0 with a depth plane");
    if ((p->flags & RT_DENOISE_DEMODULATE) && !b->albedo)
        return fail(RT_ERR_INVALID, w + "RT_DENOISE_DEMODULATE needs the albedo plane");
    if (int rc = check_denoise_small(*p, w); rc != RT_OK) return rc;
    const bool need_scratch = use_scratch && p->levels > 1u;
    if (need_scratch && !b->scratch) return fail(RT_ERR_INVALID, w + "scratch is null with levels > 1");
    const float *const scratch = use_scratch ? b->scratch : nullptr;
    for (const float *in : {b->beauty, b->albedo, b->normal, b->depth}) {
        if (in && in == b->out) return fail(RT_ERR_INVALID, w + "out is also an input plane");
        if (in && in == scratch) return fail(RT_ERR_INVALID, w + "scratch is also an input plane");
    }
    if (scratch && scratch == b->out) return fail(RT_ERR_INVALID, w + "scratch is also out");
    *terms = (p->sigma_color != 0.f ? 1u : 0u) | (b->normal ? 2u : 0u) | (b->depth ? 4u : 0u) |
             (b->albedo && p->sigma_albedo != 0.f ? 8u : 0u);
    return RT_OK;
}

float denoise_r(float sigma) { return 1.0f / (sigma * sigma); }

// The part of the kernel's record that is the same at every level of a run, of either filter: the
// guides, the image and the guides' weights (the albedo plane also where only demodulation reads it).
rt::KDenoise denoise_record(const rt_denoise_params &p, const rt_denoise_buffers &b, uint32_t terms)
{
    rt::KDenoise k{};
    k.albedo = (terms & 8u) || (p.flags & RT_DENOISE_DEMODULATE) ? b.albedo : nullptr;
    k.normal = b.normal;
    k.depth = b.depth;
    k.W = p.width;
    k.H = p.height;
    k.r_n = (terms & 2u) ? denoise_r(p.sigma_normal) : 0.f;
    k.r_z = (terms & 4u) ? denoise_r(p.sigma_depth) : 0.f;
    k.r_a = (terms & 8u) ? denoise_r(p.sigma_albedo) : 0.f;
    return k;
}

// Where level l of a run ending with level `last` writes: the last one b.out, those before it
// alternately b.scratch and b.out so that it does.
float *denoise_level_out(const rt_denoise_buffers &b, uint32_t l, uint32_t last)
{
    return ((last - l) & 1u) ? b.scratch : b.out;
}

// Enqueue levels [first, last] of the run `p` describes: level l reads `in` when l == first and
// the previous level's output otherwise (denoise_level_out). Steps up to tiled_max_step take the
// tiled kernel.
int denoise_levels(const rt_denoise_params &p, const rt_denoise_buffers &b, uint32_t terms, uint32_t first,
                   uint32_t last, uint32_t tiled_max_step, hipStream_t stream)
{
    const bool demod = (p.flags & RT_DENOISE_DEMODULATE) != 0u;
    rt::KDenoise k = denoise_record(p, b, terms);
    const float *in = b.beauty;
    for (uint32_t l = first; l <= last; ++l) {
        k.in = in;
        k.out = denoise_level_out(b, l, last);
        k.step = 1u << l;
        k.r_c = (terms & 1u) ? denoise_r(p.sigma_color * std::ldexp(1.f, -static_cast<int>(l))) : 0.f;
        k.demod_out = demod && l + 1u == p.levels;
        const bool tiled = !(p.flags & RT_DENOISE_DIRECT) && k.step <= tiled_max_step;
        RT_HIP(rt::launch_denoise(k, terms, demod && l == 0u, tiled, stream));
        in = k.out;
    }
    return RT_OK;
}

// The caller's record with the planes' addresses on the device: planes[0..3] the inputs, then out
// and scratch.
rt_denoise_buffers denoise_device_record(const Plane *planes, int out, int scratch)
{
    return {static_cast<uint32_t>(sizeof(rt_denoise_buffers)), planes[0].as<float>(), planes[1].as<float>(),
            planes[2].as<float>(), planes[3].as<float>(), planes[out].as<float>(), planes[scratch].as<float>()};
}

// A filter's or the accumulation's record: zeroed but for the two times.
void timed_stats(rt_stats &st, const SyncCall &call)
{
    st = rt_stats{};
    st.kernel_ms = call.kernel_ms;
    st.wall_ms = call.wall_ms();
}

// Synchronous denoise of host planes.
int denoise_host(const rt_denoise_params *params, const rt_denoise_buffers *buffers, rt_stats *stats)
{
    uint32_t terms = 0;
    if (int rc = check_denoise(params, buffers, false, "rt_denoise", &terms); rc != RT_OK) return rc;
    const rt_denoise_params &P = *params;
    const size_t n = static_cast<size_t>(P.width) * P.height;
    Plane planes[6] = {plane_in(buffers->beauty, 12), plane_in(buffers->albedo, 12), plane_in(buffers->normal, 12),
                       plane_in(buffers->depth, 4),   plane_out(buffers->out, 12),   plane_scratch(P.levels > 1u, 12)};
    SyncCall call;
    const int rc = call.run({"rt_denoise", planes, 6, n, {n, 1}}, [&] {
        return denoise_levels(P, denoise_device_record(planes, 4, 5), terms, 0, P.levels - 1u, kDenoiseTiledMaxStep, nullptr);
    });
    if (rc == RT_OK && stats) timed_stats(*stats, call);
    return rc;
}

// ---- the variance-guided filter (include/rt_api.h) ---------------------------
// Its checks: rt_denoise_device's, then the variance record's (use_scratch: a device call).
int check_denoise_var(const rt_denoise_params *p, const rt_denoise_buffers *b, const rt_denoise_var_buffers *v,
                      bool use_scratch, const char *who, uint32_t *terms)
{
    if (int rc = check_denoise(p, b, use_scratch, who, terms); rc != RT_OK) return rc;
    const std::string w = std::string(who) + ": ";
    if (p->flags & RT_DENOISE_DEMODULATE)
        return fail(RT_ERR_UNSUPPORTED, w + "RT_DENOISE_DEMODULATE is not supported (the variance is not demodulated)");
    if (!v) return fail(RT_ERR_INVALID, w + "null variance record");
    if (v->size != sizeof(rt_denoise_var_buffers))
        return fail(RT_ERR_INVALID, w + "var.size is not sizeof(rt_denoise_var_buffers)");
    if (!std::isfinite(v->var_floor) || !(v->var_floor > 0.f)) return fail(RT_ERR_INVALID, w + "var_floor must be finite and positive");
    if (!v->variance) return fail(RT_ERR_INVALID, w + "variance is null");
    const float *const var_scratch = use_scratch ? v->var_scratch : nullptr;
    if (use_scratch && !var_scratch) return fail(RT_ERR_INVALID, w + "var_scratch is null");
    const float *const scratch = use_scratch ? b->scratch : nullptr;
    for (const float *o : {b->beauty, b->albedo, b->normal, b->depth, static_cast<const float *>(b->out), scratch,
                           v->variance}) {
        if (o && o == v->variance_out) return fail(RT_ERR_INVALID, w + "variance_out is also another plane");
        if (o && o == var_scratch) return fail(RT_ERR_INVALID, w + "var_scratch is also another plane");
    }
    if (var_scratch && var_scratch == v->variance_out) return fail(RT_ERR_INVALID, w + "var_scratch is also variance_out");
    return RT_OK;
}

// Enqueue every level: the colours go where denoise_levels' do, the variances alternate between
// the halves of v.var_scratch; the last level's goes to v.variance_out, if given. c1, v1 (the
// preview session's feedback; both or neither): level 0 writes C_1 and V_1 there instead, and
// level 1 reads them there.
int denoise_var_levels(const rt_denoise_params &p, const rt_denoise_buffers &b, const rt_denoise_var_buffers &v,
                       uint32_t terms, hipStream_t stream, float *c1 = nullptr, float *v1 = nullptr)
{
    rt::KDenoiseVar kv{};
    rt::KDenoise &k = kv.d;
    k = denoise_record(p, b, terms);
    kv.sc2 = p.sigma_color * p.sigma_color;
    kv.var_floor = v.var_floor;
    const size_t n = static_cast<size_t>(p.width) * p.height;
    const float *in = b.beauty, *vin = v.variance;
    const uint32_t last = p.levels - 1u;
    for (uint32_t l = 0; l <= last; ++l) {
        k.in = in;
        k.out = denoise_level_out(b, l, last);
        k.step = 1u << l;
        kv.vin = vin;
        kv.vout = l == last ? v.variance_out : v.var_scratch + (l & 1u) * n;
        if (l == 0u && c1) k.out = c1, kv.vout = v1;
        RT_HIP(rt::launch_denoise_var(kv, terms, stream));
        in = k.out;
        vin = kv.vout;
    }
    return RT_OK;
}

// Synchronous variance-guided denoise of host planes.
int denoise_var_host(const rt_denoise_params *params, const rt_denoise_buffers *buffers, const rt_denoise_var_buffers *var,
                     rt_stats *stats)
{
    uint32_t terms = 0;
    if (int rc = check_denoise_var(params, buffers, var, false, "rt_denoise_var", &terms); rc != RT_OK) return rc;
    const rt_denoise_params &P = *params;
    const size_t n = static_cast<size_t>(P.width) * P.height;
    const bool more = P.levels > 1u;  // the colour scratch, and the two halves of the variance's
    Plane planes[9] = {plane_in(buffers->beauty, 12), plane_in(buffers->albedo, 12),   plane_in(buffers->normal, 12),
                       plane_in(buffers->depth, 4),   plane_in(var->variance, 4),      plane_out(buffers->out, 12),
                       plane_scratch(more, 12),       plane_out(var->variance_out, 4), plane_scratch(more, 8)};
    SyncCall call;
    const int rc = call.run({"rt_denoise_var", planes, 9, n, {n, 1}}, [&] {
        const rt_denoise_var_buffers dv{static_cast<uint32_t>(sizeof(rt_denoise_var_buffers)), var->var_floor,
                                        planes[4].as<float>(), planes[7].as<float>(), planes[8].as<float>()};
        return denoise_var_levels(P, denoise_device_record(planes, 5, 6), dv, terms, nullptr);
    });
    if (rc == RT_OK && stats) timed_stats(*stats, call);
    return rc;
}

// ---- temporal accumulation (include/rt_api.h; kernel in rt_temporal.hip) ------
// rt_temporal_params_default: the values scripts/temporal_sweep.py chose
constexpr float kTpAlphaMin = 0.4f, kTpMaxHistory = 32.0f, kTpNormalTol = 0.5f, kTpDepthTol = 0.1f;

// The checks of the params' own values (w: the message up to the field's name, as
// check_denoise_ranges takes it).
int check_temporal_ranges(const rt_temporal_params &p, const std::string &w)
{
    if (!p.width || p.width > kDenoiseMaxSide) return fail(RT_ERR_INVALID, w + "width must be 1..65536");
    if (!p.height || p.height > kDenoiseMaxSide) return fail(RT_ERR_INVALID, w + "height must be 1..65536");
    if (!std::isfinite(p.alpha_min) || !(p.alpha_min > 0.f) || p.alpha_min > 1.f)
        return fail(RT_ERR_INVALID, w + "alpha_min must be above 0 and at most 1");
    if (!std::isfinite(p.max_history) || p.max_history < 1.f) return fail(RT_ERR_INVALID, w + "max_history must be finite and at least 1");
    if (!std::isfinite(p.normal_tol) || p.normal_tol < 0.f) return fail(RT_ERR_INVALID, w + "normal_tol must be finite and not negative");
    if (!std::isfinite(p.depth_tol) || p.depth_tol < 0.f) return fail(RT_ERR_INVALID, w + "depth_tol must be finite and not negative");
    if (p.flags) return fail(RT_ERR_INVALID, w + "flags must be 0 (none is defined)");
    return RT_OK;
}

// Every argument check, before any HIP call; fills the kernel's record (the cameras as the
// contract's {a, hor, ver, o} and {A, B, G, o'}) from the caller's pointers.
int check_temporal(const rt_temporal_params *p, const rt_camera *cam, const rt_camera *prev_cam,
                   const rt_temporal_buffers *b, const char *who, rt::KTemporal *k)
{
    const std::string w = std::string(who) + ": ";
    if (!p || !b) return fail(RT_ERR_INVALID, w + "null argument");
    if (p->size != sizeof(rt_temporal_params)) return fail(RT_ERR_INVALID, w + "params.size is not sizeof(rt_temporal_params)");
    if (b->size != sizeof(rt_temporal_buffers)) return fail(RT_ERR_INVALID, w + "buffers.size is not sizeof(rt_temporal_buffers)");
    if (int rc = check_temporal_ranges(*p, w); rc != RT_OK) return rc;
    if (!cam) return fail(RT_ERR_INVALID, w + "camera is null");
    if (cam->mode > RT_CAMERA_CORRECTED) return fail(RT_ERR_INVALID, w + "camera has a bad mode");
    const struct { const char *name; const void *ptr; } cur[6] = {{"beauty", b->beauty}, {"variance", b->variance}, {"normal", b->normal},
                                                                 {"depth", b->depth},   {"alpha", b->alpha},       {"sphere_id", b->sphere_id}},
      prev[6] = {{"prev_color", b->prev_color},   {"prev_variance", b->prev_variance}, {"prev_history", b->prev_history},
                 {"prev_normal", b->prev_normal}, {"prev_depth", b->prev_depth},       {"prev_sphere_id", b->prev_sphere_id}},
      out[3] = {{"out_color", b->out_color}, {"out_variance", b->out_variance}, {"out_history", b->out_history}};
    for (const auto &c : cur)
        if (!c.ptr) return fail(RT_ERR_INVALID, w + c.name + " is null");
    for (const auto &o : out)
        if (!o.ptr) return fail(RT_ERR_INVALID, w + o.name + " is null");
    int given = 0;
    for (const auto &c : prev) given += c.ptr ? 1 : 0;
    if (given != 0 && given != 6)
        for (const auto &c : prev)
            if (!c.ptr) return fail(RT_ERR_INVALID, w + c.name + " is null while other planes of prev are given");
    for (int i = 0; i < 3; ++i) {
        for (const auto &c : cur)
            if (c.ptr == out[i].ptr) return fail(RT_ERR_INVALID, w + out[i].name + " is also the input plane " + c.name);
        for (const auto &c : prev)
            if (c.ptr == out[i].ptr) return fail(RT_ERR_INVALID, w + out[i].name + " is also the input plane " + c.name);
        for (int j = 0; j < i; ++j)
            if (out[j].ptr == out[i].ptr) return fail(RT_ERR_INVALID, w + out[i].name + " is also " + out[j].name);
    }
    rt::KTemporal t{};
    if (given) {
        if (!prev_cam) return fail(RT_ERR_INVALID, w + "prev_camera is null");
        if (rt_reproject_basis(prev_cam, t.basis) != RT_OK) return fail(RT_ERR_INVALID, w + g_error.substr(g_error.find(": ") + 2));
    }
    t.beauty = b->beauty, t.variance = b->variance, t.normal = b->normal, t.depth = b->depth, t.alpha = b->alpha;
    t.id = b->sphere_id;
    t.p_color = b->prev_color, t.p_variance = b->prev_variance, t.p_history = b->prev_history;
    t.p_normal = b->prev_normal, t.p_depth = b->prev_depth, t.p_id = b->prev_sphere_id;
    t.o_color = b->out_color, t.o_variance = b->out_variance, t.o_history = b->out_history;
    t.W = p->width, t.H = p->height;
    for (int c = 0; c < 3; ++c) {
        t.a[c] = cam->mode == RT_CAMERA_CORRECTED ? cam->lower_left_corner[c] - cam->origin[c] : cam->lower_left_corner[c];
        t.hor[c] = cam->horizontal[c], t.ver[c] = cam->vertical[c], t.o[c] = cam->origin[c];
    }
    t.alpha_min = p->alpha_min, t.max_history = p->max_history, t.normal_tol = p->normal_tol, t.depth_tol = p->depth_tol;
    *k = t;
    return RT_OK;
}

// The motion record's checks, after check_temporal's and before any HIP call; adds the tables to
// the kernel's record (null tables of a scene without spheres: a pointer that is never read,
// so that the launch still takes the motion kernel, in which every id is out of range).
int check_temporal_motion(const rt_temporal_motion_t *m, const rt_temporal_buffers *b, bool device_call, const char *who,
                          rt::KTemporal *k)
{
    const std::string w = std::string(who) + ": ";
    if (!m) return fail(RT_ERR_INVALID, w + "motion is null");
    if (m->size != sizeof(rt_temporal_motion_t)) return fail(RT_ERR_INVALID, w + "motion.size is not sizeof(rt_temporal_motion_t)");
    if (m->n_spheres && !m->centres) return fail(RT_ERR_INVALID, w + "motion.centres is null with n_spheres > 0");
    if (m->n_spheres && !m->prev_centres) return fail(RT_ERR_INVALID, w + "motion.prev_centres is null with n_spheres > 0");
    if (device_call && m->n_spheres && ((reinterpret_cast<uintptr_t>(m->centres) | reinterpret_cast<uintptr_t>(m->prev_centres)) & 15u))
        return fail(RT_ERR_INVALID, w + "motion.centres and motion.prev_centres must be 16-byte aligned");
    const struct { const char *name; const void *ptr; } out[3] = {{"out_color", b->out_color}, {"out_variance", b->out_variance},
                                                                 {"out_history", b->out_history}};
    for (const auto &o : out) {
        if (m->n_spheres && o.ptr == m->centres) return fail(RT_ERR_INVALID, w + "motion.centres is also the output plane " + o.name);
        if (m->n_spheres && o.ptr == m->prev_centres) return fail(RT_ERR_INVALID, w + "motion.prev_centres is also the output plane " + o.name);
    }
    k->centres = m->n_spheres ? m->centres : k->beauty;
    k->p_centres = m->n_spheres ? m->prev_centres : k->beauty;
    k->n_spheres = m->n_spheres;
    return RT_OK;
}

// rt_temporal_clip_default: the values scripts/clip_sweep.py chose
constexpr uint32_t kClipRadius = 1;
constexpr float kClipGamma = 0.5f;

// The clip record's checks, after every check of the underlying stage and before any HIP call; adds
// the window to the kernel's record (k null: the checks alone).
int check_temporal_clip(const rt_temporal_clip_t *c, const char *who, rt::KTemporal *k)
{
    const std::string w = std::string(who) + ": ";
    if (!c) return fail(RT_ERR_INVALID, w + "clip is null");
    if (c->size != sizeof(rt_temporal_clip_t)) return fail(RT_ERR_INVALID, w + "clip.size is not sizeof(rt_temporal_clip_t)");
    if (c->radius < 1u || c->radius > 3u) return fail(RT_ERR_INVALID, w + "clip.radius must be 1..3");
    if (!std::isfinite(c->gamma) || c->gamma < 0.f) return fail(RT_ERR_INVALID, w + "clip.gamma must be finite and not negative");
    if (c->flags) return fail(RT_ERR_INVALID, w + "clip.flags must be 0 (none is defined)");
    if (k) k->clip_radius = c->radius, k->clip_gamma = c->gamma;
    return RT_OK;
}

// Synchronous temporal accumulation of host planes: the current planes, the previous ones, the
// outputs, then the two sphere tables of the stage with object motion (motion null: the static one).
// with_clip: rt_temporal_clip (its motion is optional); the window reads planes staged anyway.
int temporal_host(const rt_temporal_params *params, const rt_camera *camera, const rt_camera *prev_camera,
                  const rt_temporal_buffers *buffers, const rt_temporal_motion_t *motion, bool with_motion, rt_stats *stats,
                  const rt_temporal_clip_t *clip = nullptr, bool with_clip = false)
{
    const char *const who = with_clip ? "rt_temporal_clip" : with_motion ? "rt_temporal_motion" : "rt_temporal";
    rt::KTemporal k{};
    if (int rc = check_temporal(params, camera, prev_camera, buffers, who, &k); rc != RT_OK) return rc;
    if (with_motion)
        if (int rc = check_temporal_motion(motion, buffers, false, who, &k); rc != RT_OK) return rc;
    if (with_clip)
        if (int rc = check_temporal_clip(clip, who, &k); rc != RT_OK) return rc;
    const size_t n = static_cast<size_t>(params->width) * params->height;
    const rt_temporal_buffers &b = *buffers;
    const uint32_t n_sph = with_motion ? motion->n_spheres : 0u;
    Plane planes[17] = {plane_in(b.beauty, 12),     plane_in(b.variance, 4),      plane_in(b.normal, 12),
                        plane_in(b.depth, 4),       plane_in(b.alpha, 4),         plane_in(b.sphere_id, 4),
                        plane_in(b.prev_color, 12), plane_in(b.prev_variance, 4), plane_in(b.prev_history, 4),
                        plane_in(b.prev_normal, 12), plane_in(b.prev_depth, 4),   plane_in(b.prev_sphere_id, 4),
                        plane_out(b.out_color, 12), plane_out(b.out_variance, 4), plane_out(b.out_history, 4),
                        plane_in(n_sph ? motion->centres : nullptr, 16), plane_in(n_sph ? motion->prev_centres : nullptr, 16)};
    planes[15].n_px = planes[16].n_px = n_sph;
    SyncCall call;
    const int rc = call.run({who, planes, 17, n, {n, 1}}, [&] {
        auto f = [&](int i) { return planes[i].as<float>(); };
        k.beauty = f(0), k.variance = f(1), k.normal = f(2), k.depth = f(3), k.alpha = f(4), k.id = planes[5].as<uint32_t>();
        k.p_color = f(6), k.p_variance = f(7), k.p_history = f(8), k.p_normal = f(9), k.p_depth = f(10);
        k.p_id = planes[11].as<uint32_t>();
        k.o_color = f(12), k.o_variance = f(13), k.o_history = f(14);
        if (with_motion) k.centres = n_sph ? f(15) : f(0), k.p_centres = n_sph ? f(16) : f(0);
        return hip_rc(rt::launch_temporal(k, nullptr), who);
    });
    if (rc == RT_OK && stats) timed_stats(*stats, call);
    return rc;
}

// ---- guided upsampling (include/rt_api.h; kernel in rt_upsample.hip) ----------
// rt_upsample_params_default: the values scripts/upscale_sweep.py chose
constexpr float kUpNormalTol = 0.01f, kUpDepthTol = 0.3f;

// The checks of the params' own values (w: the message up to the field's name).
int check_upsample_ranges(const rt_upsample_params &p, const std::string &w)
{
    if (!p.width || p.width > kDenoiseMaxSide) return fail(RT_ERR_INVALID, w + "width must be 1..65536");
    if (!p.height || p.height > kDenoiseMaxSide) return fail(RT_ERR_INVALID, w + "height must be 1..65536");
    if (!p.lo_width || p.lo_width > p.width) return fail(RT_ERR_INVALID, w + "lo_width must be 1..width");
    if (!p.lo_height || p.lo_height > p.height) return fail(RT_ERR_INVALID, w + "lo_height must be 1..height");
    if (!std::isfinite(p.normal_tol) || p.normal_tol < 0.f) return fail(RT_ERR_INVALID, w + "normal_tol must be finite and not negative");
    if (!std::isfinite(p.depth_tol) || p.depth_tol < 0.f) return fail(RT_ERR_INVALID, w + "depth_tol must be finite and not negative");
    if (p.flags) return fail(RT_ERR_INVALID, w + "flags must be 0 (none is defined)");
    return RT_OK;
}

// Every argument check, before any HIP call; fills the kernel's record from the caller's pointers.
int check_upsample(const rt_upsample_params *p, const rt_upsample_buffers *b, const char *who, rt::KUpsample *k)
{
    const std::string w = std::string(who) + ": ";
    if (!p || !b) return fail(RT_ERR_INVALID, w + "null argument");
    if (p->size != sizeof(rt_upsample_params)) return fail(RT_ERR_INVALID, w + "params.size is not sizeof(rt_upsample_params)");
    if (b->size != sizeof(rt_upsample_buffers)) return fail(RT_ERR_INVALID, w + "buffers.size is not sizeof(rt_upsample_buffers)");
    if (int rc = check_upsample_ranges(*p, w); rc != RT_OK) return rc;
    const struct { const char *name; const void *ptr; } in[9] = {
        {"lo_color", b->lo_color}, {"lo_normal", b->lo_normal}, {"lo_depth", b->lo_depth}, {"lo_sphere_id", b->lo_sphere_id},
        {"normal", b->normal},     {"depth", b->depth},         {"alpha", b->alpha},       {"sphere_id", b->sphere_id},
        {"lo_variance", b->lo_variance}};
    for (int i = 0; i < 8; ++i)
        if (!in[i].ptr) return fail(RT_ERR_INVALID, w + in[i].name + " is null");
    if (!b->out_color) return fail(RT_ERR_INVALID, w + "out_color is null");
    if (b->lo_variance && !b->out_variance) return fail(RT_ERR_INVALID, w + "lo_variance is given without out_variance");
    if (b->out_variance && !b->lo_variance) return fail(RT_ERR_INVALID, w + "out_variance is given without lo_variance");
    for (const auto &c : in) {
        if (c.ptr && c.ptr == b->out_color) return fail(RT_ERR_INVALID, w + "out_color is also the input plane " + c.name);
        if (c.ptr && c.ptr == b->out_variance) return fail(RT_ERR_INVALID, w + "out_variance is also the input plane " + c.name);
    }
    if (static_cast<const void *>(b->out_variance) == b->out_color) return fail(RT_ERR_INVALID, w + "out_variance is also out_color");
    *k = rt::KUpsample{b->lo_color, b->lo_variance, b->lo_normal, b->lo_depth, b->lo_sphere_id, b->normal, b->depth,
                       b->alpha,    b->sphere_id,   b->out_color, b->out_variance, p->width,    p->height, p->lo_width,
                       p->lo_height, p->normal_tol, p->depth_tol};
    return RT_OK;
}

// Synchronous upsample of host planes: the low-resolution planes (a pixel count of their own), the
// output-size guides, then the outputs.
int upsample_host(const rt_upsample_params *params, const rt_upsample_buffers *buffers, rt_stats *stats)
{
    rt::KUpsample k{};
    if (int rc = check_upsample(params, buffers, "rt_upsample", &k); rc != RT_OK) return rc;
    const size_t n = static_cast<size_t>(params->width) * params->height;
    const size_t n_lo = static_cast<size_t>(params->lo_width) * params->lo_height;
    const rt_upsample_buffers &b = *buffers;
    Plane planes[11] = {plane_in(b.lo_color, 12), plane_in(b.lo_variance, 4), plane_in(b.lo_normal, 12),
                        plane_in(b.lo_depth, 4),  plane_in(b.lo_sphere_id, 4), plane_in(b.normal, 12),
                        plane_in(b.depth, 4),     plane_in(b.alpha, 4),       plane_in(b.sphere_id, 4),
                        plane_out(b.out_color, 12), plane_out(b.out_variance, 4)};
    for (int i = 0; i < 5; ++i) planes[i].n_px = n_lo;
    SyncCall call;
    const int rc = call.run({"rt_upsample", planes, 11, n, {n, 1}}, [&] {
        auto f = [&](int i) { return planes[i].as<float>(); };
        k.l_color = f(0), k.l_variance = f(1), k.l_normal = f(2), k.l_depth = f(3), k.l_id = planes[4].as<uint32_t>();
        k.normal = f(5), k.depth = f(6), k.alpha = f(7), k.id = planes[8].as<uint32_t>();
        k.o_color = f(9), k.o_variance = f(10);
        return hip_rc(rt::launch_upsample(k, nullptr), "rt_upsample");
    });
    if (rc == RT_OK && stats) timed_stats(*stats, call);
    return rc;
}

} // namespace

// ---- the preview session (include/rt_api.h; kernels in rt_preview.hip) ---------
// Every plane is a piece of one device allocation, made by rt_preview_create; a plane that the
// session's flags and levels never touch is not there (its pointer stays null).
struct rt_preview {
    rt_scene *scene = nullptr;
    int device = 0;
    rt_preview_params p{};
    uint32_t terms = 0;            // the filter's edge terms (check_denoise)
    DevBuf<char> arena;
    uint64_t bytes = 0;
    // the frame's render, its guides that no later frame reads, and what DEMODULATE makes of it
    float *beauty = nullptr, *variance = nullptr, *albedo = nullptr, *alpha = nullptr;
    float *illum = nullptr, *illum_var = nullptr;
    // the guides the temporal stage compares, and what it reprojects: set `cur` is written by the
    // next frame, the other one is its prev_ (one set under NO_TEMPORAL, no history at all)
    struct Guides { float *normal = nullptr, *depth = nullptr; uint32_t *id = nullptr; } g[2];
    struct History { float *color = nullptr, *variance = nullptr, *history = nullptr; } h[2];
    // FEEDBACK: the temporal stage's outputs (h[cur] takes the first filter level's)
    float *acc_color = nullptr, *acc_variance = nullptr;
    // the filter's output and the levels' intermediate planes
    float *filtered = nullptr, *scratch = nullptr, *var_scratch = nullptr;
    // an upscaled session (rt_preview_create_upscaled; up.size is 0 otherwise): the guides of the
    // output size (the albedo under DEMODULATE only) and the upsampled image
    rt_preview_upscale up{};
    float *up_albedo = nullptr, *up_normal = nullptr, *up_depth = nullptr, *up_alpha = nullptr, *upsampled = nullptr;
    uint32_t *up_id = nullptr;
    bool up_written = false;       // a frame has written them
    uint32_t cur = 0;
    rt_camera prev_camera{};
    // rt_preview_set_clip's record (clip.size is 0: the temporal stage runs without the clamp)
    rt_temporal_clip_t clip{};
    // the scene's epochs at the session's last frame (rt_scene_motion)
    uint64_t geometry_epoch = 0, appearance_epoch = 0;
    rt_preview_planes_t last{};    // last.frames: frames since creation or the last reset
    // rt_preview_refine_device: the progressive session of the view at rest,
    // allocated on first use, and the refinement in progress (refining: no frame call since its start)
    rt_progressive *refine = nullptr;
    bool refining = false;
    rt_camera refine_camera{};
    uint64_t refine_seed = 0;
    uint64_t refine_geometry = 0, refine_appearance = 0;
};

namespace {

constexpr uint32_t kPreviewFlags = RT_PREVIEW_DEMODULATE | RT_PREVIEW_FEEDBACK | RT_PREVIEW_NO_TEMPORAL;
// rt_preview_params_default: max_depth as the reference's bounces_number; the flags
// scripts/preview_sweep.py chose
constexpr uint32_t kPvMaxDepth = 64;
constexpr uint32_t kPvFlags = RT_PREVIEW_DEMODULATE;

// Every check of a session's params, before its scene is looked at and before any HIP call. terms:
// the filter's edge terms (the session gives every guide).
int check_preview(const rt_preview_params *p, uint32_t *terms)
{
    const std::string w = "rt_preview_create: ";
    if (!p) return fail(RT_ERR_INVALID, w + "null params");
    if (p->size != sizeof(rt_preview_params)) return fail(RT_ERR_INVALID, w + "size is not sizeof(rt_preview_params)");
    if (!p->width || p->width > kDenoiseMaxSide) return fail(RT_ERR_INVALID, w + "width must be 1..65536");
    if (!p->height || p->height > kDenoiseMaxSide) return fail(RT_ERR_INVALID, w + "height must be 1..65536");
    if (static_cast<uint64_t>(p->width) * p->height >= (1ull << 31))
        return fail(RT_ERR_INVALID, w + "width * height must be below 2^31 (one render call)");
    if (p->spp < 2u) return fail(RT_ERR_INVALID, w + "spp must be at least 2 (a variance needs two samples)");
    if (!p->max_depth) return fail(RT_ERR_INVALID, w + "max_depth must be at least 1");
    if (p->flags & ~kPreviewFlags) return fail(RT_ERR_INVALID, w + "unknown bits in flags");
    if ((p->flags & RT_PREVIEW_FEEDBACK) && (p->flags & RT_PREVIEW_NO_TEMPORAL))
        return fail(RT_ERR_INVALID, w + "flags: RT_PREVIEW_FEEDBACK needs the temporal stage (RT_PREVIEW_NO_TEMPORAL is set)");
    if (!std::isfinite(p->var_floor) || !(p->var_floor > 0.f)) return fail(RT_ERR_INVALID, w + "var_floor must be finite and positive");
    const rt_temporal_params &t = p->temporal;
    if (t.size != sizeof(rt_temporal_params)) return fail(RT_ERR_INVALID, w + "temporal.size is not sizeof(rt_temporal_params)");
    if (t.width != p->width) return fail(RT_ERR_INVALID, w + "temporal.width is not the session's width");
    if (t.height != p->height) return fail(RT_ERR_INVALID, w + "temporal.height is not the session's height");
    if (int rc = check_temporal_ranges(t, w + "temporal."); rc != RT_OK) return rc;
    const rt_denoise_params &d = p->denoise;
    if (d.size != sizeof(rt_denoise_params)) return fail(RT_ERR_INVALID, w + "denoise.size is not sizeof(rt_denoise_params)");
    if (d.width != p->width) return fail(RT_ERR_INVALID, w + "denoise.width is not the session's width");
    if (d.height != p->height) return fail(RT_ERR_INVALID, w + "denoise.height is not the session's height");
    if (int rc = check_denoise_ranges(d, w + "denoise."); rc != RT_OK) return rc;
    if (d.flags & RT_DENOISE_DEMODULATE)
        return fail(RT_ERR_INVALID, w + "denoise.flags holds RT_DENOISE_DEMODULATE (the session demodulates with RT_PREVIEW_DEMODULATE)");
    if (d.flags & ~static_cast<uint32_t>(RT_DENOISE_DIRECT)) return fail(RT_ERR_INVALID, w + "unknown bits in denoise.flags");
    if (d.sigma_normal == 0.f) return fail(RT_ERR_INVALID, w + "denoise.sigma_normal is 0 with a normal plane");
    if (d.sigma_depth == 0.f) return fail(RT_ERR_INVALID, w + "denoise.sigma_depth is 0 with a depth plane");
    if (int rc = check_denoise_small(d, w + "denoise."); rc != RT_OK) return rc;
    *terms = (d.sigma_color != 0.f ? 1u : 0u) | 2u | 4u | (d.sigma_albedo != 0.f ? 8u : 0u);
    return RT_OK;
}

// The session's planes, each a multiple of 256 bytes from the arena's start: the first pass
// (base null) sizes the arena, the second hands the addresses out.
size_t preview_carve(rt_preview &pv, char *base)
{
    const rt_preview_params &p = pv.p;
    const size_t n = static_cast<size_t>(p.width) * p.height;
    const bool temporal = !(p.flags & RT_PREVIEW_NO_TEMPORAL), feedback = (p.flags & RT_PREVIEW_FEEDBACK) != 0u;
    const bool demod = (p.flags & RT_PREVIEW_DEMODULATE) != 0u;
    // the levels between the first (whose output the feedback keeps) and the last use the scratch planes
    const bool between = p.denoise.levels > (feedback ? 2u : 1u);
    size_t at = 0;
    auto take = [&](auto *&plane, size_t words, bool wanted = true) {
        if (!wanted) return;
        if (base) plane = reinterpret_cast<std::remove_reference_t<decltype(plane)>>(base + at);
        at += (words * n * sizeof(float) + 255u) / 256u * 256u;
    };
    take(pv.beauty, 3), take(pv.variance, 1), take(pv.albedo, 3), take(pv.alpha, 1);
    take(pv.illum, 3, demod), take(pv.illum_var, 1, demod);
    for (int s = 0; s < (temporal ? 2 : 1); ++s) take(pv.g[s].normal, 3), take(pv.g[s].depth, 1), take(pv.g[s].id, 1);
    for (int s = 0; s < 2; ++s)
        take(pv.h[s].color, 3, temporal), take(pv.h[s].variance, 1, temporal), take(pv.h[s].history, 1, temporal);
    take(pv.acc_color, 3, feedback), take(pv.acc_variance, 1, feedback);
    take(pv.filtered, 3), take(pv.scratch, 3, between), take(pv.var_scratch, 2, between);
    if (pv.up.size) {
        const size_t n_out = static_cast<size_t>(pv.up.out_width) * pv.up.out_height;
        auto take_out = [&](auto *&plane, size_t words, bool wanted = true) {
            if (!wanted) return;
            if (base) plane = reinterpret_cast<std::remove_reference_t<decltype(plane)>>(base + at);
            at += (words * n_out * sizeof(float) + 255u) / 256u * 256u;
        };
        take_out(pv.up_albedo, 3, demod), take_out(pv.up_normal, 3), take_out(pv.up_depth, 1), take_out(pv.up_alpha, 1);
        take_out(pv.up_id, 1), take_out(pv.upsampled, 3);
    }
    return at;
}

// One frame of the loop, enqueued on `st`. The session's history moves on only when every stage
// was enqueued.
int preview_frame(rt_preview &pv, const rt_camera *camera, uint64_t seed, float *d_rgb, uint8_t *d_rgb8, hipStream_t st)
{
    const char *const who = "rt_preview_frame_device";
    const rt_preview_params &P = pv.p;
    const bool temporal = !(P.flags & RT_PREVIEW_NO_TEMPORAL), feedback = (P.flags & RT_PREVIEW_FEEDBACK) != 0u;
    const bool demod = (P.flags & RT_PREVIEW_DEMODULATE) != 0u;
    const uint32_t c = pv.cur, o = c ^ 1u;
    const rt_preview::Guides &g = pv.g[c];
    // The scene since the session's last frame (rt_scene_update): other colours, or more than one
    // step of the geometry, and the frame has no history, as after rt_preview_reset; one step of the
    // geometry and the temporal stage takes the scene's two tables.
    rt_scene_motion_t sm{};
    if (int rc = rt_scene_motion(pv.scene, &sm); rc != RT_OK) return rc;
    const bool restart = pv.last.frames != 0u && (sm.appearance_epoch != pv.appearance_epoch ||
                                                 sm.geometry_epoch - pv.geometry_epoch > 1u);
    const bool moved = !restart && pv.last.frames != 0u && sm.geometry_epoch != pv.geometry_epoch;
    // 1 render
    const rt_params rp{P.width, P.height, P.spp, P.max_depth, seed, 0u, 1u, 0u, 0u};
    if (int rc = rt_render_var_device(pv.scene, camera, &rp, pv.beauty, pv.variance, st, nullptr); rc != RT_OK) return rc;
    const rt_aov_buffers aov{static_cast<uint32_t>(sizeof(rt_aov_buffers)), 0u, pv.albedo, g.normal, g.depth, pv.alpha, g.id};
    if (int rc = rt_render_aov_device(pv.scene, camera, &rp, &aov, st); rc != RT_OK) return rc;
    // 2 split
    const float *color = pv.beauty, *variance = pv.variance;
    if (demod) {
        RT_HIP(rt::launch_preview_split({pv.beauty, pv.variance, pv.albedo, pv.illum, pv.illum_var, P.width, P.height}, st));
        color = pv.illum, variance = pv.illum_var;
    }
    // 3 temporal
    if (temporal) {
        const bool prev = pv.last.frames != 0u && !restart;
        const rt_preview::History &hp = pv.h[o];
        const rt_preview::Guides &gp = pv.g[o];
        float *const out_c = feedback ? pv.acc_color : pv.h[c].color, *const out_v = feedback ? pv.acc_variance : pv.h[c].variance;
        const rt_temporal_buffers tb{static_cast<uint32_t>(sizeof(rt_temporal_buffers)),
                                     color, variance, g.normal, g.depth, pv.alpha, g.id,
                                     prev ? hp.color : nullptr, prev ? hp.variance : nullptr, prev ? hp.history : nullptr,
                                     prev ? gp.normal : nullptr, prev ? gp.depth : nullptr, prev ? gp.id : nullptr,
                                     out_c, out_v, pv.h[c].history};
        rt::KTemporal k{};
        if (int rc = check_temporal(&P.temporal, camera, prev ? &pv.prev_camera : nullptr, &tb, who, &k); rc != RT_OK) return rc;
        if (moved) {
            const rt_temporal_motion_t tm{static_cast<uint32_t>(sizeof(rt_temporal_motion_t)), sm.n_spheres, sm.centres,
                                          sm.prev_centres};
            if (int rc = check_temporal_motion(&tm, &tb, true, who, &k); rc != RT_OK) return rc;
        }
        if (pv.clip.size)
            if (int rc = check_temporal_clip(&pv.clip, who, &k); rc != RT_OK) return rc;
        RT_HIP(rt::launch_temporal(k, st));
        color = out_c, variance = out_v;
    }
    // 4 filter
    const rt_denoise_buffers db{static_cast<uint32_t>(sizeof(rt_denoise_buffers)), color, pv.albedo, g.normal, g.depth,
                                pv.filtered, pv.scratch};
    const rt_denoise_var_buffers vb{static_cast<uint32_t>(sizeof(rt_denoise_var_buffers)), P.var_floor, variance, nullptr,
                                    pv.var_scratch};
    float *const c1 = feedback ? pv.h[c].color : nullptr, *const v1 = feedback ? pv.h[c].variance : nullptr;
    if (int rc = denoise_var_levels(P.denoise, db, vb, pv.terms, st, c1, v1); rc != RT_OK) return rc;
    // 5 merge
    const float *const filtered = feedback && P.denoise.levels == 1u ? c1 : pv.filtered;
    if (!pv.up.size) {
        RT_HIP(rt::launch_preview_merge({filtered, demod ? pv.albedo : nullptr, d_rgb, d_rgb8, P.width, P.height}, st));
    } else {
        // an upscaled session: the guides of the output size, the upsample, the merge at that size
        const rt_preview_upscale &U = pv.up;
        const rt_params gp{U.out_width, U.out_height, P.spp, P.max_depth, seed, 0u, 1u, 0u, 0u};
        const rt_aov_buffers ga{static_cast<uint32_t>(sizeof(rt_aov_buffers)), U.guide_samples, pv.up_albedo, pv.up_normal,
                                pv.up_depth, pv.up_alpha, pv.up_id};
        if (int rc = rt_render_aov_device(pv.scene, camera, &gp, &ga, st); rc != RT_OK) return rc;
        const rt_upsample_params upar{static_cast<uint32_t>(sizeof(rt_upsample_params)), U.out_width, U.out_height, P.width,
                                      P.height, U.normal_tol, U.depth_tol, 0u};
        const rt_upsample_buffers ub{static_cast<uint32_t>(sizeof(rt_upsample_buffers)), filtered, nullptr, g.normal, g.depth,
                                     g.id, pv.up_normal, pv.up_depth, pv.up_alpha, pv.up_id, pv.upsampled, nullptr};
        rt::KUpsample ku{};
        if (int rc = check_upsample(&upar, &ub, who, &ku); rc != RT_OK) return rc;
        RT_HIP(rt::launch_upsample(ku, st));
        RT_HIP(rt::launch_preview_merge({pv.upsampled, demod ? pv.up_albedo : nullptr, d_rgb, d_rgb8, U.out_width, U.out_height}, st));
        pv.up_written = true;
    }
    // what the frame wrote, and what the next one reprojects
    rt_preview_planes_t &l = pv.last;
    l.frames = restart ? 1u : l.frames + 1u;
    pv.geometry_epoch = sm.geometry_epoch, pv.appearance_epoch = sm.appearance_epoch;
    l.out_color = color, l.out_variance = variance, l.out_history = temporal ? pv.h[c].history : nullptr;
    l.albedo = pv.albedo, l.normal = g.normal, l.depth = g.depth, l.alpha = pv.alpha, l.sphere_id = g.id;
    if (temporal) {
        l.prev_color = pv.h[c].color, l.prev_variance = pv.h[c].variance, l.prev_history = pv.h[c].history;
        l.prev_normal = g.normal, l.prev_depth = g.depth, l.prev_sphere_id = g.id;
        pv.cur = o;
        pv.prev_camera = *camera;
    }
    return RT_OK;
}

int check_preview_side(uint32_t width, uint32_t height, const std::string &w)
{
    if (!width || width > kDenoiseMaxSide) return fail(RT_ERR_INVALID, w + "width must be 1..65536");
    if (!height || height > kDenoiseMaxSide) return fail(RT_ERR_INVALID, w + "height must be 1..65536");
    return RT_OK;
}

// Every check of an upscaled session's second record, after check_preview has passed `p`.
int check_preview_upscale(const rt_preview_params &p, const rt_preview_upscale *u)
{
    const std::string w = "rt_preview_create_upscaled: ";
    if (!u) return fail(RT_ERR_INVALID, w + "null upscale record");
    if (u->size != sizeof(rt_preview_upscale)) return fail(RT_ERR_INVALID, w + "upscale.size is not sizeof(rt_preview_upscale)");
    if (u->out_width < p.width || u->out_width > kDenoiseMaxSide)
        return fail(RT_ERR_INVALID, w + "out_width must be the session's width..65536");
    if (u->out_height < p.height || u->out_height > kDenoiseMaxSide)
        return fail(RT_ERR_INVALID, w + "out_height must be the session's height..65536");
    if (static_cast<uint64_t>(u->out_width) * u->out_height >= (1ull << 31))
        return fail(RT_ERR_INVALID, w + "out_width * out_height must be below 2^31 (one render call)");
    if (u->guide_samples > p.spp) return fail(RT_ERR_INVALID, w + "guide_samples must be at most spp");
    if (!std::isfinite(u->normal_tol) || u->normal_tol < 0.f) return fail(RT_ERR_INVALID, w + "normal_tol must be finite and not negative");
    if (!std::isfinite(u->depth_tol) || u->depth_tol < 0.f) return fail(RT_ERR_INVALID, w + "depth_tol must be finite and not negative");
    return RT_OK;
}

// A session of either kind (u null: an ordinary one): its params checked, its planes allocated.
int preview_create(rt_scene *scene, const rt_preview_params *p, const rt_preview_upscale *u, const char *who,
                   rt_preview **out)
{
    uint32_t terms = 0;
    if (int rc = check_preview(p, &terms); rc != RT_OK) return rc;
    if (!scene) return fail(RT_ERR_INVALID, std::string(who) + ": scene is null");
    if (!out) return fail(RT_ERR_INVALID, std::string(who) + ": out is null");
    rt_preview *pv = new rt_preview;
    pv->scene = scene;
    pv->device = scene_device(scene);
    pv->p = *p;
    if (u) pv->up = *u;
    pv->terms = terms;
    pv->last.size = static_cast<uint32_t>(sizeof(rt_preview_planes_t));
    pv->bytes = preview_carve(*pv, nullptr);
    hipError_t e = hipSetDevice(pv->device);
    if (e == hipSuccess) e = pv->arena.alloc(pv->bytes);
    if (e != hipSuccess) {
        delete pv;
        return fail(RT_ERR_DEVICE, std::string(who) + ": the session's planes: " + hipGetErrorString(e));
    }
    preview_carve(*pv, pv->arena.get());
    *out = pv;
    return RT_OK;
}

} // namespace

extern "C" {

int rt_preview_params_default(uint32_t width, uint32_t height, uint32_t spp, rt_preview_params *out)
{
    if (!out) return fail(RT_ERR_INVALID, "rt_preview_params_default: null argument");
    if (!width || !height) return fail(RT_ERR_INVALID, "rt_preview_params_default: zero width or height");
    if (spp < 2u) return fail(RT_ERR_INVALID, "rt_preview_params_default: spp must be at least 2 (a variance needs two samples)");
    rt_preview_params p{};
    rt_denoise_var_buffers v{};
    if (int rc = rt_temporal_params_default(width, height, &p.temporal); rc != RT_OK) return rc;
    if (int rc = rt_denoise_var_params_default(width, height, &p.denoise, &v); rc != RT_OK) return rc;
    p.size = static_cast<uint32_t>(sizeof(rt_preview_params));
    p.width = width, p.height = height, p.spp = spp, p.max_depth = kPvMaxDepth;
    p.flags = kPvFlags;
    p.var_floor = v.var_floor;
    *out = p;
    return RT_OK;
}

int rt_preview_upscale_default(const rt_preview_params *p, uint32_t out_width, uint32_t out_height, rt_preview_upscale *out)
{
    if (!p || !out) return fail(RT_ERR_INVALID, "rt_preview_upscale_default: null argument");
    if (out_width < p->width || out_height < p->height || !out_width || !out_height)
        return fail(RT_ERR_INVALID, "rt_preview_upscale_default: the output is smaller than the session's frame");
    rt_upsample_params up{};
    if (int rc = rt_upsample_params_default(out_width, out_height, p->width, p->height, &up); rc != RT_OK) return rc;
    *out = rt_preview_upscale{static_cast<uint32_t>(sizeof(rt_preview_upscale)), out_width, out_height, 0u, up.normal_tol,
                              up.depth_tol};
    return RT_OK;
}

int rt_preview_create(rt_scene *scene, const rt_preview_params *p, rt_preview **out)
{
    return preview_create(scene, p, nullptr, "rt_preview_create", out);
}

int rt_preview_create_upscaled(rt_scene *scene, const rt_preview_params *p, const rt_preview_upscale *u, rt_preview **out)
{
    uint32_t terms = 0;
    if (int rc = check_preview(p, &terms); rc != RT_OK) return rc;
    if (int rc = check_preview_upscale(*p, u); rc != RT_OK) return rc;
    return preview_create(scene, p, u, "rt_preview_create_upscaled", out);
}

int rt_preview_output(rt_preview *pv, rt_preview_output_t *out)
{
    if (!pv || !out) return fail(RT_ERR_INVALID, "rt_preview_output: null argument");
    if (!pv->up.size) return fail(RT_ERR_INVALID, "rt_preview_output: the session is not an upscaled one (rt_preview_create made it)");
    rt_preview_output_t o{};
    o.size = static_cast<uint32_t>(sizeof(rt_preview_output_t));
    o.width = pv->up.out_width, o.height = pv->up.out_height;
    if (pv->up_written) {
        o.upsampled = pv->upsampled, o.albedo = pv->up_albedo, o.normal = pv->up_normal, o.depth = pv->up_depth;
        o.alpha = pv->up_alpha, o.sphere_id = pv->up_id;
    }
    *out = o;
    return RT_OK;
}

int rt_preview_frame_device(rt_preview *pv, const rt_camera *camera, uint64_t seed, float *d_rgb, uint8_t *d_rgb8,
                            void *stream)
{
    if (!pv) return fail(RT_ERR_INVALID, "rt_preview_frame_device: null session");
    if (!camera) return fail(RT_ERR_INVALID, "rt_preview_frame_device: camera is null");
    if (!d_rgb && !d_rgb8) return fail(RT_ERR_INVALID, "rt_preview_frame_device: d_rgb and d_rgb8 are both null");
    pv->refining = false;  // (a refinement restarts after a frame call)
    return preview_frame(*pv, camera, seed, d_rgb, d_rgb8, static_cast<hipStream_t>(stream));
}

int rt_preview_reset(rt_preview *pv)
{
    if (!pv) return fail(RT_ERR_INVALID, "rt_preview_reset: null session");
    pv->last.frames = 0u;
    return RT_OK;
}

int rt_preview_set_clip(rt_preview *pv, const rt_temporal_clip_t *clip)
{
    if (!pv) return fail(RT_ERR_INVALID, "rt_preview_set_clip: null session");
    if (pv->p.flags & RT_PREVIEW_NO_TEMPORAL)
        return fail(RT_ERR_INVALID, "rt_preview_set_clip: the session has no temporal stage (RT_PREVIEW_NO_TEMPORAL is set)");
    if (!clip) {
        pv->clip = rt_temporal_clip_t{};
        return RT_OK;
    }
    if (int rc = check_temporal_clip(clip, "rt_preview_set_clip", nullptr); rc != RT_OK) return rc;
    pv->clip = *clip;
    return RT_OK;
}

int rt_preview_planes(rt_preview *pv, rt_preview_planes_t *out)
{
    if (!pv || !out) return fail(RT_ERR_INVALID, "rt_preview_planes: null argument");
    *out = pv->last;
    return RT_OK;
}

int rt_preview_usage(const rt_preview *pv, uint64_t *bytes)
{
    if (!pv || !bytes) return fail(RT_ERR_INVALID, "rt_preview_usage: null argument");
    *bytes = pv->bytes;
    if (pv->refine) {
        rt_progressive_info_t info{};
        if (int rc = rt_progressive_info(pv->refine, &info); rc != RT_OK) return rc;
        *bytes += info.device_bytes;
    }
    return RT_OK;
}

void rt_preview_destroy(rt_preview *pv)
{
    if (!pv) return;
    // (the frames enqueued may still run: hipFree waits for the device)
    if (pv->refine) (void)rt_progressive_destroy(pv->refine);
    (void)hipSetDevice(pv->device);
    delete pv;
}

int rt_preview_split_device(uint32_t width, uint32_t height, const float *beauty, const float *variance,
                            const float *albedo, float *illumination, float *variance_out, void *stream)
{
    const std::string w = "rt_preview_split_device: ";
    if (int rc = check_preview_side(width, height, w); rc != RT_OK) return rc;
    const struct { const char *name; const void *ptr; } planes[5] = {
        {"beauty", beauty}, {"variance", variance}, {"albedo", albedo}, {"illumination", illumination}, {"variance_out", variance_out}};
    for (const auto &pl : planes)
        if (!pl.ptr) return fail(RT_ERR_INVALID, w + pl.name + " is null");
    RT_HIP(rt::launch_preview_split({beauty, variance, albedo, illumination, variance_out, width, height},
                                    static_cast<hipStream_t>(stream)));
    return RT_OK;
}

int rt_preview_merge_device(uint32_t width, uint32_t height, const float *filtered, const float *albedo, float *d_rgb,
                            uint8_t *d_rgb8, void *stream)
{
    const std::string w = "rt_preview_merge_device: ";
    if (int rc = check_preview_side(width, height, w); rc != RT_OK) return rc;
    if (!filtered) return fail(RT_ERR_INVALID, w + "filtered is null");
    if (!d_rgb && !d_rgb8) return fail(RT_ERR_INVALID, w + "d_rgb and d_rgb8 are both null");
    RT_HIP(rt::launch_preview_merge({filtered, albedo, d_rgb, d_rgb8, width, height}, static_cast<hipStream_t>(stream)));
    return RT_OK;
}

} // extern "C"

// ---- the progressive session (include/rt_api.h; kernel in rt_progressive.hip) -----
// The carried planes are one device allocation made by rt_progressive_create: acc, then mom, each
// n_pixels x 3 floats. ev_tail follows the last step's work (save and load wait for it).
struct rt_progressive {
    rt_scene *scene = nullptr;
    int device = 0;
    rt_params p{};
    rt_camera camera{};
    PixelLayout layout{};
    uint32_t done = 0;
    DevBuf<float> planes;
    float *acc = nullptr, *mom = nullptr;
    Event ev_tail;
    bool tail_valid = false;
    uint64_t geometry_epoch = 0, appearance_epoch = 0;
};

// The Step rule: m = min(n, spp - done); a window that stops before the frame's end holds whole blocks of 4.
// (rt_host_sync.h: the adaptive session, rt_host_adaptive.cpp, takes its windows by the same rule)
int rthost::progressive_window(const std::string &w, uint32_t spp, uint32_t done, uint32_t n, uint32_t *m)
{
    if (spp < 2u) return fail(RT_ERR_INVALID, w + "spp must be at least 2");
    if (done > spp || (done != spp && (done & 3u))) return fail(RT_ERR_INVALID, w + "done must be a multiple of 4 or spp");
    const uint32_t left = spp - done;
    if ((n & 3u) && n < left)
        return fail(RT_ERR_INVALID, w + "n_samples must be a multiple of 4 before the frame's end (passes start on multiples of 4)");
    *m = n < left ? n : left;
    return RT_OK;
}

namespace {

// The head of a checkpoint (rt_progressive_save); the planes follow it.
struct ProgressiveHeader {
    uint64_t magic;
    uint32_t version, layout;
    rt_params params;
    rt_camera camera;
    uint64_t n_pixels;
    uint32_t done, reserved;
};
constexpr uint64_t kProgressiveMagic = 0x31474f5250545152ull;  // "RQTPROG1"
// acc[n_pixels][3] then mom[n_pixels][3] = {L_0, m1, m2}, floats, in the natural enumeration of 8 x 8 tiles
constexpr uint32_t kProgressiveLayout = 0x33383301u;

uint64_t progressive_plane_bytes(uint64_t n_pixels) { return n_pixels * 3u * sizeof(float); }
uint64_t progressive_state_bytes(uint64_t n_pixels) { return sizeof(ProgressiveHeader) + 2u * progressive_plane_bytes(n_pixels); }

// load's check: the blob against the params and camera of a session.
int progressive_blob_check(const std::string &w, const void *host, uint64_t bytes, const rt_params &P, const rt_camera &cam,
                           rt_progressive_info_t *info)
{
    if (!host) return fail(RT_ERR_INVALID, w + "host is null");
    if (bytes < sizeof(ProgressiveHeader)) return fail(RT_ERR_CAPACITY, w + "bytes is smaller than a checkpoint's header");
    ProgressiveHeader h;
    std::memcpy(&h, host, sizeof h);
    if (h.magic != kProgressiveMagic) return fail(RT_ERR_INVALID, w + "magic: not a checkpoint of rt_progressive_save");
    if (h.version != RT_API_VERSION) return fail(RT_ERR_INVALID, w + "version: the checkpoint is of another RT_API_VERSION");
    if (h.layout != kProgressiveLayout) return fail(RT_ERR_INVALID, w + "layout: the checkpoint's planes are laid out otherwise");
    const struct { const char *name; uint64_t blob, own; } fields[] = {
        {"width", h.params.width, P.width}, {"height", h.params.height, P.height}, {"spp", h.params.spp, P.spp},
        {"max_depth", h.params.max_depth, P.max_depth}, {"seed", h.params.seed, P.seed},
        {"row_offset", h.params.row_offset, P.row_offset}, {"row_stride", h.params.row_stride, P.row_stride},
        {"num_rows", h.params.num_rows, P.num_rows}, {"flags", h.params.flags, P.flags}};
    for (const auto &f : fields)
        if (f.blob != f.own)
            return fail(RT_ERR_INVALID, w + "params." + f.name + " of the checkpoint (" + std::to_string(f.blob) +
                                            ") is not the session's (" + std::to_string(f.own) + ")");
    if (std::memcmp(&h.camera, &cam, sizeof(rt_camera)) != 0) return fail(RT_ERR_INVALID, w + "camera of the checkpoint is not the session's");
    const uint64_t n_pixels = pixel_layout(P).n_pixels;
    if (h.n_pixels != n_pixels) return fail(RT_ERR_INVALID, w + "n_pixels of the checkpoint is not the session's");
    if (h.done > P.spp || (h.done != P.spp && (h.done & 3u)))
        return fail(RT_ERR_INVALID, w + "done of the checkpoint is not a multiple of 4 or spp");
    if (bytes < progressive_state_bytes(n_pixels)) return fail(RT_ERR_CAPACITY, w + "bytes is smaller than the checkpoint (truncated)");
    if (info)
        *info = rt_progressive_info_t{static_cast<uint32_t>(sizeof(rt_progressive_info_t)), h.done, P.spp, 0u, n_pixels,
                                      progressive_state_bytes(n_pixels), 2u * progressive_plane_bytes(n_pixels)};
    return RT_OK;
}

// The outputs record of a step, before the session is looked at.
int check_progressive_outputs(const rt_progressive_outputs *o, const std::string &w)
{
    if (!o) return RT_OK;
    if (o->size != sizeof(rt_progressive_outputs)) return fail(RT_ERR_INVALID, w + "out.size is not sizeof(rt_progressive_outputs)");
    const struct { const char *name; const void *ptr; } planes[4] = {
        {"rgb", o->rgb}, {"variance", o->variance}, {"rgb8", o->rgb8}, {"noisy", o->noisy}};
    bool any = false;
    for (int i = 0; i < 4; ++i) {
        any = any || planes[i].ptr;
        for (int j = 0; j < i; ++j)
            if (planes[i].ptr && planes[i].ptr == planes[j].ptr)
                return fail(RT_ERR_INVALID, w + "out." + planes[i].name + " is also out." + planes[j].name);
    }
    if (!any) return fail(RT_ERR_INVALID, w + "out: rgb, variance, rgb8 and noisy are all null");
    if (o->noisy && (!std::isfinite(o->noise_tau) || o->noise_tau < 0.f))
        return fail(RT_ERR_INVALID, w + "out.noise_tau must be finite and not negative");
    return RT_OK;
}

int progressive_epochs(rt_progressive &pg)
{
    rt_scene_motion_t sm{};
    if (int rc = rt_scene_motion(pg.scene, &sm); rc != RT_OK) return rc;
    pg.geometry_epoch = sm.geometry_epoch, pg.appearance_epoch = sm.appearance_epoch;
    return RT_OK;
}

// save and load: the session's enqueued work has finished
int progressive_wait(rt_progressive &pg)
{
    RT_HIP(hipSetDevice(pg.device));
    if (pg.tail_valid) RT_HIP(hipEventSynchronize(pg.ev_tail.get()));
    return RT_OK;
}

} // namespace

extern "C" {

int rt_progressive_window(uint32_t spp, uint32_t done, uint32_t n_samples, uint32_t *m)
{
    if (!m) return fail(RT_ERR_INVALID, "rt_progressive_window: m is null");
    return progressive_window("rt_progressive_window: ", spp, done, n_samples, m);
}

int rt_progressive_create(rt_scene *scene, const rt_camera *camera, const rt_params *params, rt_progressive **out)
{
    const std::string w = "rt_progressive_create: ";
    if (int rc = check_var_params(params, "rt_progressive_create"); rc != RT_OK) return rc;
    const PixelLayout l = pixel_layout(*params);
    if (l.n_pixels >= (1ull << 31)) return fail(RT_ERR_INVALID, w + "params: more than 2^31 pixels in one call");
    if (!l.n_pixels) return fail(RT_ERR_INVALID, w + "params: no rows to render");
    if (!camera) return fail(RT_ERR_INVALID, w + "camera is null");
    if (!scene) return fail(RT_ERR_INVALID, w + "scene is null");
    if (!out) return fail(RT_ERR_INVALID, w + "out is null");
    rt_progressive *pg = new rt_progressive;
    pg->scene = scene;
    pg->device = scene_device(scene);
    pg->p = *params;
    pg->camera = *camera;
    pg->layout = l;
    hipError_t e = hipSetDevice(pg->device);
    if (e == hipSuccess) e = pg->planes.alloc(2u * progressive_plane_bytes(l.n_pixels));
    if (e == hipSuccess) e = pg->ev_tail.make(hipEventDisableTiming);
    if (e != hipSuccess) {
        delete pg;
        return fail(RT_ERR_DEVICE, w + "the session's planes: " + hipGetErrorString(e));
    }
    pg->acc = pg->planes.get();
    pg->mom = pg->acc + 3u * l.n_pixels;
    if (int rc = progressive_epochs(*pg); rc != RT_OK) {
        (void)rt_progressive_destroy(pg);
        return rc;
    }
    *out = pg;
    return RT_OK;
}

int rt_progressive_step_device(rt_progressive *pg, uint32_t n_samples, const rt_progressive_outputs *out, void *stream,
                               uint64_t *d_segments)
{
    const std::string w = "rt_progressive_step_device: ";
    if (int rc = check_progressive_outputs(out, w); rc != RT_OK) return rc;
    if (!pg) return fail(RT_ERR_INVALID, w + "null session");
    uint32_t m = 0;
    if (int rc = progressive_window(w, pg->p.spp, pg->done, n_samples, &m); rc != RT_OK) return rc;
    if (out && pg->done + m < 2u) return fail(RT_ERR_INVALID, w + "out is given but no sample is done (a resolve needs done >= 2)");
    rt_scene_motion_t sm{};
    if (int rc = rt_scene_motion(pg->scene, &sm); rc != RT_OK) return rc;
    if (sm.geometry_epoch != pg->geometry_epoch || sm.appearance_epoch != pg->appearance_epoch)
        return fail(RT_ERR_INVALID, w + "the scene was updated since the session's first step (rt_progressive_reset starts the frame again)");
    if (!m && !out) return RT_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t a = pg->done, b = pg->done + m;
    const PixelLayout &l = pg->layout;
    auto resolve = [&]() -> int {
        if (!out) return RT_OK;
        if (out->noisy) RT_HIP(hipMemsetAsync(out->noisy, 0, sizeof(uint32_t), st));
        rt::KResolve k{};
        k.acc = pg->acc, k.mom = pg->mom;
        k.out = out->rgb, k.var = out->variance, k.out_u8 = out->rgb8, k.noisy = out->noisy;
        k.t2 = out->noisy ? out->noise_tau * out->noise_tau : 0.f;
        k.done = b;
        k.n_pixels = static_cast<uint32_t>(l.n_pixels);
        k.W = l.W, k.tiles_x = l.tiles_x, k.tiled_rows = l.tiled_rows, k.tile_lw = l.tile_lw;
        k.row_offset = l.row_offset, k.row_stride = l.row_stride, k.full_frame = l.full_frame;
        RT_HIP(rt::launch_progressive_resolve(k, st));
        return RT_OK;
    };
    if (int rc = render_window(pg->scene, &pg->camera, pg->p, a, b, pg->acc, pg->mom, st, d_segments, resolve); rc != RT_OK) {
        // (a failure part of the way leaves the planes undefined: the frame starts again)
        if (m) pg->done = 0;
        return rc;
    }
    pg->done = b;
    RT_HIP(hipEventRecord(pg->ev_tail.get(), st));
    pg->tail_valid = true;
    return RT_OK;
}

int rt_progressive_info(const rt_progressive *pg, rt_progressive_info_t *info)
{
    if (!pg) return fail(RT_ERR_INVALID, "rt_progressive_info: null session");
    if (!info) return fail(RT_ERR_INVALID, "rt_progressive_info: info is null");
    const uint64_t n = pg->layout.n_pixels;
    *info = rt_progressive_info_t{static_cast<uint32_t>(sizeof(rt_progressive_info_t)), pg->done, pg->p.spp, 0u, n,
                                  progressive_state_bytes(n), 2u * progressive_plane_bytes(n)};
    return RT_OK;
}

int rt_progressive_reset(rt_progressive *pg, const rt_camera *camera, const uint64_t *seed)
{
    if (!pg) return fail(RT_ERR_INVALID, "rt_progressive_reset: null session");
    if (int rc = progressive_epochs(*pg); rc != RT_OK) return rc;
    if (camera) pg->camera = *camera;
    if (seed) pg->p.seed = *seed;
    pg->done = 0;
    return RT_OK;
}

int rt_progressive_save(rt_progressive *pg, void *host, uint64_t cap)
{
    const std::string w = "rt_progressive_save: ";
    if (!pg) return fail(RT_ERR_INVALID, w + "null session");
    if (!host) return fail(RT_ERR_INVALID, w + "host is null");
    const uint64_t n = pg->layout.n_pixels, plane = progressive_plane_bytes(n);
    if (cap < progressive_state_bytes(n)) return fail(RT_ERR_CAPACITY, w + "cap is smaller than state_bytes (rt_progressive_info)");
    if (int rc = progressive_wait(*pg); rc != RT_OK) return rc;
    const ProgressiveHeader h{kProgressiveMagic, RT_API_VERSION, kProgressiveLayout, pg->p, pg->camera, n, pg->done, 0u};
    std::memcpy(host, &h, sizeof h);
    // (acc and mom are adjacent: one copy)
    RT_HIP(hipMemcpy(static_cast<char *>(host) + sizeof h, pg->acc, 2u * plane, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_progressive_load(rt_progressive *pg, const void *host, uint64_t bytes)
{
    const std::string w = "rt_progressive_load: ";
    if (!pg) return fail(RT_ERR_INVALID, w + "null session");
    rt_progressive_info_t info{};
    if (int rc = progressive_blob_check(w, host, bytes, pg->p, pg->camera, &info); rc != RT_OK) return rc;
    if (int rc = progressive_wait(*pg); rc != RT_OK) return rc;
    RT_HIP(hipMemcpy(pg->acc, static_cast<const char *>(host) + sizeof(ProgressiveHeader), info.device_bytes, hipMemcpyHostToDevice));
    RT_HIP(hipDeviceSynchronize());  // (the planes are in place before a step on any stream)
    if (int rc = progressive_epochs(*pg); rc != RT_OK) return rc;
    pg->done = info.done;
    return RT_OK;
}

int rt_progressive_blob_check(const void *host, uint64_t bytes, const rt_params *params, const rt_camera *camera,
                              rt_progressive_info_t *info)
{
    const std::string w = "rt_progressive_blob_check: ";
    if (int rc = check_var_params(params, "rt_progressive_blob_check"); rc != RT_OK) return rc;
    if (!camera) return fail(RT_ERR_INVALID, w + "camera is null");
    return progressive_blob_check(w, host, bytes, *params, *camera, info);
}

int rt_progressive_destroy(rt_progressive *pg)
{
    if (!pg) return fail(RT_ERR_INVALID, "rt_progressive_destroy: null session");
    // (the steps enqueued may still run: hipFree waits for the device)
    (void)hipSetDevice(pg->device);
    delete pg;
    return RT_OK;
}

// The preview session at rest (include/rt_api.h): the session's own progressive session steps the
// frame of total_spp samples into beauty / variance; until the frame is complete every call filters
// the estimate with its carried variance (no temporal stage), then it stores the frame itself.
int rt_preview_refine_device(rt_preview *pv, const rt_camera *camera, uint64_t seed, uint32_t total_spp, uint32_t n_samples,
                             float *d_rgb, uint8_t *d_rgb8, void *stream)
{
    const std::string w = "rt_preview_refine_device: ";
    if (!pv) return fail(RT_ERR_INVALID, w + "null session");
    if (!camera) return fail(RT_ERR_INVALID, w + "camera is null");
    if (!d_rgb && !d_rgb8) return fail(RT_ERR_INVALID, w + "d_rgb and d_rgb8 are both null");
    if (total_spp < 2u) return fail(RT_ERR_INVALID, w + "total_spp must be at least 2 (a variance needs two samples)");
    if (pv->up.size) return fail(RT_ERR_UNSUPPORTED, w + "an upscaled session does not refine (rt_preview_create_upscaled made it)");
    const rt_preview_params &P = pv->p;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const rt_params rp{P.width, P.height, total_spp, P.max_depth, seed, 0u, 1u, 0u, 0u};
    rt_scene_motion_t sm{};
    if (int rc = rt_scene_motion(pv->scene, &sm); rc != RT_OK) return rc;
    const bool restart = !pv->refining || !pv->refine || pv->refine->p.spp != total_spp || pv->refine_seed != seed ||
                         std::memcmp(&pv->refine_camera, camera, sizeof(rt_camera)) != 0 ||
                         sm.geometry_epoch != pv->refine_geometry || sm.appearance_epoch != pv->refine_appearance;
    // the Step rule before anything is enqueued or started
    uint32_t m = 0;
    if (int rc = progressive_window(w, total_spp, restart ? 0u : pv->refine->done, n_samples, &m); rc != RT_OK) return rc;
    if ((restart ? 0u : pv->refine->done) + m < 2u)
        return fail(RT_ERR_INVALID, w + "n_samples: the first call of a refinement must render at least 2 samples");
    const rt_preview::Guides &g = pv->g[pv->cur];
    if (restart) {
        if (!pv->refine) {
            if (int rc = rt_progressive_create(pv->scene, camera, &rp, &pv->refine); rc != RT_OK) return rc;
        } else {
            if (int rc = rt_progressive_reset(pv->refine, camera, &seed); rc != RT_OK) return rc;
            pv->refine->p.spp = total_spp;  // (the planes do not depend on the sample count)
        }
        pv->refining = false;
        pv->last.frames = 0u;  // the next frame call has no history, as after rt_preview_reset
        // the guides, once per refinement
        const rt_aov_buffers aov{static_cast<uint32_t>(sizeof(rt_aov_buffers)), total_spp < P.spp ? total_spp : P.spp,
                                 pv->albedo, g.normal, g.depth, pv->alpha, g.id};
        if (int rc = rt_render_aov_device(pv->scene, camera, &rp, &aov, st); rc != RT_OK) return rc;
        pv->refine_camera = *camera, pv->refine_seed = seed;
        pv->refine_geometry = sm.geometry_epoch, pv->refine_appearance = sm.appearance_epoch;
    }
    const rt_progressive_outputs po{static_cast<uint32_t>(sizeof(rt_progressive_outputs)), 0.f, pv->beauty, pv->variance, nullptr,
                                    nullptr};
    if (int rc = rt_progressive_step_device(pv->refine, n_samples, &po, st, nullptr); rc != RT_OK) return rc;
    pv->refining = true;
    if (pv->refine->done == total_spp) {
        // the frame itself, unfiltered: the resolve's bits and their texels
        RT_HIP(rt::launch_preview_merge({pv->beauty, nullptr, d_rgb, d_rgb8, P.width, P.height}, st));
        return RT_OK;
    }
    const bool demod = (P.flags & RT_PREVIEW_DEMODULATE) != 0u;
    const float *color = pv->beauty, *variance = pv->variance;
    if (demod) {
        RT_HIP(rt::launch_preview_split({pv->beauty, pv->variance, pv->albedo, pv->illum, pv->illum_var, P.width, P.height}, st));
        color = pv->illum, variance = pv->illum_var;
    }
    const rt_denoise_buffers db{static_cast<uint32_t>(sizeof(rt_denoise_buffers)), color, pv->albedo, g.normal, g.depth,
                                pv->filtered, pv->scratch};
    const rt_denoise_var_buffers vb{static_cast<uint32_t>(sizeof(rt_denoise_var_buffers)), P.var_floor, variance, nullptr,
                                    pv->var_scratch};
    // (a FEEDBACK session's levels use the planes a frame's do: the first level's output goes to the
    // history planes, which the next frame call does not read: it has no history)
    const bool feedback = (P.flags & RT_PREVIEW_FEEDBACK) != 0u;
    float *const c1 = feedback ? pv->h[pv->cur].color : nullptr, *const v1 = feedback ? pv->h[pv->cur].variance : nullptr;
    if (int rc = denoise_var_levels(P.denoise, db, vb, pv->terms, st, c1, v1); rc != RT_OK) return rc;
    const float *const filtered = feedback && P.denoise.levels == 1u ? c1 : pv->filtered;
    RT_HIP(rt::launch_preview_merge({filtered, demod ? pv->albedo : nullptr, d_rgb, d_rgb8, P.width, P.height}, st));
    return RT_OK;
}

int rt_preview_refine_info(const rt_preview *pv, uint32_t *done, uint32_t *total)
{
    if (!pv || !done || !total) return fail(RT_ERR_INVALID, "rt_preview_refine_info: null argument");
    *done = pv->refining ? pv->refine->done : 0u;
    *total = pv->refining ? pv->refine->p.spp : 0u;
    return RT_OK;
}

int rt_temporal_params_default(uint32_t width, uint32_t height, rt_temporal_params *out)
{
    if (!out) return fail(RT_ERR_INVALID, "rt_temporal_params_default: null argument");
    if (!width || !height) return fail(RT_ERR_INVALID, "rt_temporal_params_default: zero width or height");
    *out = rt_temporal_params{static_cast<uint32_t>(sizeof(rt_temporal_params)), width, height, kTpAlphaMin, kTpMaxHistory,
                              kTpNormalTol, kTpDepthTol, 0u};
    return RT_OK;
}

int rt_temporal_device(const rt_temporal_params *params, const rt_camera *camera, const rt_camera *prev_camera,
                       const rt_temporal_buffers *buffers, void *stream)
{
    rt::KTemporal k{};
    if (int rc = check_temporal(params, camera, prev_camera, buffers, "rt_temporal_device", &k); rc != RT_OK) return rc;
    RT_HIP(rt::launch_temporal(k, static_cast<hipStream_t>(stream)));
    return RT_OK;
}

int rt_temporal(const rt_temporal_params *params, const rt_camera *camera, const rt_camera *prev_camera,
                const rt_temporal_buffers *buffers, rt_stats *stats)
{
    return temporal_host(params, camera, prev_camera, buffers, nullptr, false, stats);
}

int rt_temporal_motion_device(const rt_temporal_params *params, const rt_camera *camera, const rt_camera *prev_camera,
                              const rt_temporal_buffers *buffers, const rt_temporal_motion_t *motion, void *stream)
{
    rt::KTemporal k{};
    if (int rc = check_temporal(params, camera, prev_camera, buffers, "rt_temporal_motion_device", &k); rc != RT_OK) return rc;
    if (int rc = check_temporal_motion(motion, buffers, true, "rt_temporal_motion_device", &k); rc != RT_OK) return rc;
    RT_HIP(rt::launch_temporal(k, static_cast<hipStream_t>(stream)));
    return RT_OK;
}

int rt_temporal_motion(const rt_temporal_params *params, const rt_camera *camera, const rt_camera *prev_camera,
                       const rt_temporal_buffers *buffers, const rt_temporal_motion_t *motion, rt_stats *stats)
{
    return temporal_host(params, camera, prev_camera, buffers, motion, true, stats);
}

int rt_temporal_clip_default(rt_temporal_clip_t *out)
{
    if (!out) return fail(RT_ERR_INVALID, "rt_temporal_clip_default: null argument");
    *out = rt_temporal_clip_t{static_cast<uint32_t>(sizeof(rt_temporal_clip_t)), kClipRadius, kClipGamma, 0u};
    return RT_OK;
}

int rt_temporal_clip_device(const rt_temporal_params *params, const rt_camera *camera, const rt_camera *prev_camera,
                            const rt_temporal_buffers *buffers, const rt_temporal_motion_t *motion,
                            const rt_temporal_clip_t *clip, void *stream)
{
    const char *const who = "rt_temporal_clip_device";
    rt::KTemporal k{};
    if (int rc = check_temporal(params, camera, prev_camera, buffers, who, &k); rc != RT_OK) return rc;
    if (motion)
        if (int rc = check_temporal_motion(motion, buffers, true, who, &k); rc != RT_OK) return rc;
    if (int rc = check_temporal_clip(clip, who, &k); rc != RT_OK) return rc;
    RT_HIP(rt::launch_temporal(k, static_cast<hipStream_t>(stream)));
    return RT_OK;
}

int rt_temporal_clip(const rt_temporal_params *params, const rt_camera *camera, const rt_camera *prev_camera,
                     const rt_temporal_buffers *buffers, const rt_temporal_motion_t *motion, const rt_temporal_clip_t *clip,
                     rt_stats *stats)
{
    return temporal_host(params, camera, prev_camera, buffers, motion, motion != nullptr, stats, clip, true);
}

int rt_upsample_params_default(uint32_t width, uint32_t height, uint32_t lo_width, uint32_t lo_height, rt_upsample_params *out)
{
    if (!out) return fail(RT_ERR_INVALID, "rt_upsample_params_default: null argument");
    if (!width || !height || !lo_width || !lo_height) return fail(RT_ERR_INVALID, "rt_upsample_params_default: a zero side");
    *out = rt_upsample_params{static_cast<uint32_t>(sizeof(rt_upsample_params)), width, height, lo_width, lo_height,
                              kUpNormalTol, kUpDepthTol, 0u};
    return RT_OK;
}

int rt_upsample_device(const rt_upsample_params *params, const rt_upsample_buffers *buffers, void *stream)
{
    rt::KUpsample k{};
    if (int rc = check_upsample(params, buffers, "rt_upsample_device", &k); rc != RT_OK) return rc;
    RT_HIP(rt::launch_upsample(k, static_cast<hipStream_t>(stream)));
    return RT_OK;
}

int rt_upsample(const rt_upsample_params *params, const rt_upsample_buffers *buffers, rt_stats *stats)
{
    return upsample_host(params, buffers, stats);
}

int rt_denoise_var_params_default(uint32_t width, uint32_t height, rt_denoise_params *params, rt_denoise_var_buffers *var)
{
    if (!params && !var) return fail(RT_ERR_INVALID, "rt_denoise_var_params_default: null argument");
    if (!width || !height) return fail(RT_ERR_INVALID, "rt_denoise_var_params_default: zero width or height");
    // chosen by the CPU sweep of DESIGN.md §4.10 (scripts/denoise_var_sweep.py)
    if (params)
        *params = rt_denoise_params{static_cast<uint32_t>(sizeof(rt_denoise_params)), width, height, kDnVarLevels,
                                    kDnVarSigmaColor, kDnVarSigmaNormal, kDnVarSigmaDepth, kDnVarSigmaAlbedo, 0u};
    if (var)
        *var = rt_denoise_var_buffers{static_cast<uint32_t>(sizeof(rt_denoise_var_buffers)), kDnVarFloor, nullptr, nullptr,
                                      nullptr};
    return RT_OK;
}

int rt_denoise_var_device(const rt_denoise_params *params, const rt_denoise_buffers *buffers,
                          const rt_denoise_var_buffers *var, void *stream)
{
    uint32_t terms = 0;
    if (int rc = check_denoise_var(params, buffers, var, true, "rt_denoise_var_device", &terms); rc != RT_OK) return rc;
    return denoise_var_levels(*params, *buffers, *var, terms, static_cast<hipStream_t>(stream));
}

int rt_denoise_var(const rt_denoise_params *params, const rt_denoise_buffers *buffers, const rt_denoise_var_buffers *var,
                   rt_stats *stats)
{
    return denoise_var_host(params, buffers, var, stats);
}

int rt_denoise_params_default(uint32_t width, uint32_t height, rt_denoise_params *out)
{
    if (!out) return fail(RT_ERR_INVALID, "rt_denoise_params_default: null argument");
    if (!width || !height) return fail(RT_ERR_INVALID, "rt_denoise_params_default: zero width or height");
    // chosen by the CPU sweep of DESIGN.md §4.9
    *out = rt_denoise_params{static_cast<uint32_t>(sizeof(rt_denoise_params)), width, height, 2u, 4.0f, 2.0f, 1.0f, 1.0f, 0u};
    return RT_OK;
}

int rt_denoise_device(const rt_denoise_params *params, const rt_denoise_buffers *buffers, void *stream)
{
    uint32_t terms = 0;
    if (int rc = check_denoise(params, buffers, true, "rt_denoise_device", &terms); rc != RT_OK) return rc;
    return denoise_levels(*params, *buffers, terms, 0, params->levels - 1u, kDenoiseTiledMaxStep,
                          static_cast<hipStream_t>(stream));
}

int rt_denoise_level_device(const rt_denoise_params *params, const rt_denoise_buffers *buffers, uint32_t level,
                            void *stream)
{
    uint32_t terms = 0;
    if (int rc = check_denoise(params, buffers, false, "rt_denoise_level_device", &terms); rc != RT_OK) return rc;
    if (level >= params->levels) return fail(RT_ERR_INVALID, "rt_denoise_level_device: level is not below levels");
    return denoise_levels(*params, *buffers, terms, level, level, kDenoiseTiledFits, static_cast<hipStream_t>(stream));
}

int rt_denoise(const rt_denoise_params *params, const rt_denoise_buffers *buffers, rt_stats *stats)
{
    return denoise_host(params, buffers, stats);
}

} // extern "C"
