// rt_host_synccall.cpp — the synchronous host-buffer calls (include/rt_api.h rt_render_f32 / rgb8 /
// var / aov, rt_render_cuda_impl: the entry points that replace `cuda_impl`, src/main.cxx:18,
// src/CUDA/cuda_impl.cu:384) and the cached per-device context they share: the device scene kept
// between calls, the arena of device planes, and the one path every such call takes through it
// (rt_host_sync.h SyncCall, which rt_host_post.cpp's synchronous filters take too).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rt_api.h"
#include "rt_hip_own.h"
#include "rt_host_build.h"
#include "rt_host_sync.h"
#include "rt_scene.h"

using namespace rthost;

namespace {

// The synchronous calls' per-device context, kept between calls: the reference's entry point
// (cuda_impl, src/CUDA/cuda_impl.cu:384-453) is called once per frame with the same scene, and
// building the scene (clusters, shortcut words, streams, events), its workspaces and the frame
// buffers on every call cost more than the frame itself. The context is keyed by the scene's
// records and the options its scene would be created with (rt_get_default_options at the call):
// another scene or other options rebuild it. rt_release_cached frees it.
struct SyncContext {
    std::vector<unsigned char> key;
    rt_scene *sc = nullptr;
    // The device planes of every synchronous call, grow-only: each call lays its planes out from
    // offset 0 (rthost::plane_layout), so the arena holds the largest call's need, not the sum.
    // Nothing in it outlives a call: every input plane is uploaded by the call that reads it, and
    // every plane a call copies back is first written in full by its kernels (the rendered rows,
    // each filter level's output and scratch, the temporal outputs) or cleared (render_host's
    // full frame); the full-frame feature and variance renders copy back only the rows they wrote.
    DevBuf<char> arena;
    DevBuf<uint64_t> d_seg;  // the work counters of a render with stats (24 bytes)
    Event e0, e1;
};
std::mutex g_sync_mu;  // one synchronous call at a time per process (the reference's entry is not re-entrant)
// (never destroyed: a context that rt_release_cached did not free stays allocated at exit, as it
// always has; its owners must not call into HIP while the process is being torn down)
std::map<int, SyncContext> &g_sync = *new std::map<int, SyncContext>;

void sync_release(int dev, SyncContext &c)
{
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(dev);
    if (c.sc) rt_scene_destroy(c.sc);
    c = SyncContext{};  // (what it owned frees itself)
    (void)hipSetDevice(prev);
}

// The device's context holds this scene under the current process-default options: kept if it
// does already, rebuilt otherwise (g_sync_mu held).
int sync_scene(int dev, SyncContext &cx, const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials,
               uint32_t n_materials)
{
    rt_options opt;
    if (int rc = rt_get_default_options(&opt); rc) return rc;
    std::vector<unsigned char> key(sizeof(rt_sphere) * n_spheres + sizeof(rt_material) * n_materials + sizeof(opt));
    unsigned char *k = key.data();
    if (n_spheres) std::memcpy(k, spheres, sizeof(rt_sphere) * n_spheres);
    k += sizeof(rt_sphere) * n_spheres;
    std::memcpy(k, materials, sizeof(rt_material) * n_materials);
    k += sizeof(rt_material) * n_materials;
    std::memcpy(k, &opt, sizeof(opt));
    if (!cx.sc || key != cx.key) {
        sync_release(dev, cx);
        if (int rc = rt_scene_create(spheres, n_spheres, materials, n_materials, dev, &cx.sc); rc) return rc;
        cx.key.swap(key);
    }
    return RT_OK;
}

} // namespace

namespace rthost {

SyncCall::SyncCall() : t0_(std::chrono::steady_clock::now()), lock_(g_sync_mu) {}

int SyncCall::run(const SyncSpec &s, const std::function<int()> &enqueue, const std::function<int()> &after)
{
    int dev = 0;
    RT_HIP(hipGetDevice(&dev));
    SyncContext &cx = g_sync[dev];
    if (s.scene) {
        if (int rc = sync_scene(dev, cx, s.scene->spheres, s.scene->n_spheres, s.scene->materials, s.scene->n_materials); rc)
            return rc;
        scene = cx.sc;
    }
    const size_t total = plane_layout(s.planes, s.n_planes, s.n_px);
    int rc = RT_OK;
    auto chk = [&](hipError_t e, const char *what) {
        if (rc == RT_OK) rc = hip_rc(e, what);
        return rc == RT_OK;
    };
    rc = cx.arena.ensure(total);  // (its wait finds the device idle: every call ends synchronised)
    if (rc == RT_OK && s.counters && !cx.d_seg) chk(cx.d_seg.alloc(24), "hipMalloc");
    if (rc == RT_OK) chk(cx.e0.make(hipEventDefault), "hipEventCreate");
    if (rc == RT_OK) chk(cx.e1.make(hipEventDefault), "hipEventCreate");
    if (rc == RT_OK && !s.skip) {
        Plane *const end = s.planes + s.n_planes;
        for (Plane *pl = s.planes; pl != end; ++pl) {
            if (pl->kind == Plane::Absent) continue;
            pl->dev = cx.arena.get() + pl->at;
            if (rc == RT_OK && pl->kind == Plane::In)
                chk(hipMemcpy(pl->dev, pl->host, pl->pixels(s.n_px) * pl->px_bytes, hipMemcpyHostToDevice), "hipMemcpy");
            if (rc == RT_OK && pl->clear) chk(hipMemsetAsync(pl->dev, 0, pl->pixels(s.n_px) * pl->px_bytes, nullptr), "hipMemset");
        }
        // the work counters (rt_stats) come from the counting instantiation of the kernels, slower than
        // the product's: only when the caller asks for them (rt::render_impl does not, as cuda_impl)
        if (rc == RT_OK && s.counters) {
            chk(hipMemsetAsync(cx.d_seg.get(), 0, 24, nullptr), "hipMemset");
            d_counters = cx.d_seg.get();
        }
        if (rc == RT_OK) chk(hipEventRecord(cx.e0.get(), nullptr), "hipEventRecord");
        if (rc == RT_OK) rc = enqueue();
        if (rc == RT_OK) chk(hipEventRecord(cx.e1.get(), nullptr), "hipEventRecord");
        if (rc == RT_OK && after) rc = after();
        // the copies on the null stream follow the work; the last one returns when all is done
        const SyncRows &r = s.rows;
        for (const Plane *pl = s.planes; pl != end; ++pl) {
            if (rc != RT_OK || pl->kind != Plane::Out) continue;
            const size_t row_bytes = r.width * pl->px_bytes;
            if (!r.stride) {
                chk(hipMemcpy(pl->host, pl->dev, r.rows * row_bytes, hipMemcpyDeviceToHost), "hipMemcpy");
            } else {
                const size_t first = r.offset * row_bytes;
                chk(hipMemcpy2D(static_cast<char *>(pl->host) + first, r.stride * row_bytes,
                                static_cast<const char *>(pl->dev) + first, r.stride * row_bytes, row_bytes, r.rows,
                                hipMemcpyDeviceToHost),
                    "hipMemcpy2D");
            }
        }
        if (rc == RT_OK && s.counters) chk(hipMemcpy(counters, cx.d_seg.get(), 24, hipMemcpyDeviceToHost), "hipMemcpy");
        if (rc == RT_OK) chk(hipDeviceSynchronize(), s.who);
        if (rc == RT_OK) chk(hipEventElapsedTime(&kernel_ms, cx.e0.get(), cx.e1.get()), "hipEventElapsedTime");
    }
    if (rc != RT_OK) {
        // a failed call leaves no state behind: the next one starts from a new context
        const std::string msg = g_error;
        sync_release(dev, cx);
        g_error = msg;
    }
    return rc;
}

} // namespace rthost

namespace {

// The rows a render's outputs come back as: the rendered rows one after the other, or, of a full
// frame, those rows only, each to its place in the caller's frame.
SyncRows rendered_rows(const rt_params &P)
{
    if (!(P.flags & RT_FLAG_FULL_FRAME)) return {P.width, rows_of(P)};
    return {P.width, rows_of(P), P.row_offset, P.row_stride ? P.row_stride : 1u};
}

// The six fields a counted render sets of the caller's record (the others stay as they are).
void render_stats(rt_stats &st, const SyncCall &call, uint64_t primaries)
{
    st.primaries = primaries;
    st.segments = call.counters[0];
    st.sphere_tests = call.counters[1];
    st.box_tests = call.counters[2];
    st.kernel_ms = call.kernel_ms;
    st.wall_ms = call.wall_ms();
}

// Synchronous host-buffer render on the current device (the cuda_impl replacement). The frame is
// rendered as floats also where only the 8-bit image is wanted; a full frame comes back whole,
// cleared where no row was rendered.
int render_host(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials, uint32_t n_materials,
                const rt_camera *camera, const rt_params *params, float *rgb_out, uint8_t *u8_out, rt_stats *stats)
{
    if (!camera || (!rgb_out && !u8_out)) return fail(RT_ERR_INVALID, "render: null argument");
    if (int rc = check_params(params); rc != RT_OK) return rc;
    if ((n_spheres && !spheres) || !materials || !n_materials) return fail(RT_ERR_INVALID, "render: null scene");
    const rt_params &P = *params;
    const bool full = (P.flags & RT_FLAG_FULL_FRAME) != 0u;
    const size_t rows = full ? P.height : rows_of(P), n_px = rows * P.width;
    Plane planes[2] = {rgb_out ? plane_out(rgb_out, 12) : plane_scratch(true, 12), plane_out(u8_out, 3)};
    planes[0].clear = full;
    const SyncScene scene{spheres, n_spheres, materials, n_materials};
    SyncCall call;
    const int rc = call.run(
        {"render", planes, 2, n_px, {P.width, rows}, &scene, stats != nullptr},
        [&] { return rt_render_device(call.scene, camera, params, planes[0].as<float>(), nullptr, call.d_counters); },
        [&] { return u8_out ? rt_epilogue_rgb8_device(planes[0].as<float>(), planes[1].as<uint8_t>(), n_px, nullptr) : RT_OK; });
    if (rc == RT_OK && stats) render_stats(*stats, call, static_cast<uint64_t>(P.width) * rows_of(P) * P.spp);
    return rc;
}

// Synchronous feature buffers into host planes (full frame: the rendered rows only).
int render_aov_host(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials, uint32_t n_materials,
                    const rt_camera *camera, const rt_params *params, const rt_aov_buffers *aov, rt_stats *stats)
{
    if (int rc = check_aov(params, aov, "rt_render_aov"); rc != RT_OK) return rc;
    if (!camera) return fail(RT_ERR_INVALID, "rt_render_aov: null camera");
    if ((n_spheres && !spheres) || !materials || !n_materials) return fail(RT_ERR_INVALID, "rt_render_aov: null scene");
    const rt_params &P = *params;
    const SyncRows rows = rendered_rows(P);
    const size_t rows_out = (P.flags & RT_FLAG_FULL_FRAME) ? P.height : rows.rows;
    const uint32_t samples = aov->samples ? aov->samples : P.spp;
    Plane planes[5] = {plane_out(aov->albedo, 12), plane_out(aov->normal, 12), plane_out(aov->depth, 4),
                       plane_out(aov->alpha, 4), plane_out(aov->sphere_id, 4)};
    const SyncScene scene{spheres, n_spheres, materials, n_materials};
    SyncCall call;
    const int rc = call.run({"rt_render_aov", planes, 5, rows_out * P.width, rows, &scene, false, rows.rows == 0}, [&] {
        const rt_aov_buffers d{static_cast<uint32_t>(sizeof(rt_aov_buffers)), samples, planes[0].as<float>(),
                               planes[1].as<float>(), planes[2].as<float>(), planes[3].as<float>(), planes[4].as<uint32_t>()};
        return rt_render_aov_device(call.scene, camera, params, &d, nullptr);
    });
    if (rc == RT_OK && stats) {
        *stats = rt_stats{};
        stats->primaries = stats->segments = static_cast<uint64_t>(P.width) * rows.rows * samples;
        stats->kernel_ms = call.kernel_ms;
        stats->wall_ms = call.wall_ms();
    }
    return rc;
}

// Synchronous render with the variance plane into host buffers (full frame: the rendered rows
// only, of both outputs).
int render_var_host(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials, uint32_t n_materials,
                    const rt_camera *camera, const rt_params *params, float *rgb_out, float *var_out, rt_stats *stats)
{
    if (!camera) return fail(RT_ERR_INVALID, "rt_render_var: null camera");
    if (!rgb_out) return fail(RT_ERR_INVALID, "rt_render_var: null rgb_out");
    if (!var_out) return fail(RT_ERR_INVALID, "rt_render_var: null var_out");
    if (var_out == rgb_out) return fail(RT_ERR_INVALID, "rt_render_var: var_out is also rgb_out");
    if (int rc = check_var_params(params, "rt_render_var"); rc != RT_OK) return rc;
    if ((n_spheres && !spheres) || !materials || !n_materials) return fail(RT_ERR_INVALID, "rt_render_var: null scene");
    const rt_params &P = *params;
    const SyncRows rows = rendered_rows(P);
    const size_t rows_out = (P.flags & RT_FLAG_FULL_FRAME) ? P.height : rows.rows;
    Plane planes[2] = {plane_out(rgb_out, 12), plane_out(var_out, 4)};
    const SyncScene scene{spheres, n_spheres, materials, n_materials};
    SyncCall call;
    const int rc = call.run({"rt_render_var", planes, 2, rows_out * P.width, rows, &scene, stats != nullptr, rows.rows == 0}, [&] {
        return rt_render_var_device(call.scene, camera, params, planes[0].as<float>(), planes[1].as<float>(), nullptr,
                                    call.d_counters);
    });
    if (rc == RT_OK && stats) render_stats(*stats, call, static_cast<uint64_t>(P.width) * rows.rows * P.spp);
    return rc;
}

} // namespace

extern "C" {

int rt_render_cuda_impl(uint32_t width, uint32_t height, uint8_t *rgb_out)
{
    if (!rgb_out) return fail(RT_ERR_INVALID, "rt_render_cuda_impl: null output");
    rt_sphere s[8];
    rt_material m[8];
    uint32_t ns = 0, nm = 0;
    if (int rc = rt_scene_cuda(s, 8, &ns, m, 8, &nm); rc) return rc;
    rt_camera cam;
    if (int rc = rt_camera_cuda(width, height, &cam); rc) return rc;
    rt_params p{width, height, 48, 32, 0, 0, 1, 0, RT_FLAG_CUDA_COMPAT};  // cuda_impl.cu:62-63
    return rt_render_rgb8(s, ns, m, nm, &cam, &p, rgb_out, nullptr);
}

int rt_render_var(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials, uint32_t n_materials,
                  const rt_camera *camera, const rt_params *params, float *rgb_out, float *var_out, rt_stats *stats)
{
    return render_var_host(spheres, n_spheres, materials, n_materials, camera, params, rgb_out, var_out, stats);
}

int rt_render_aov(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials, uint32_t n_materials,
                  const rt_camera *camera, const rt_params *params, const rt_aov_buffers *aov, rt_stats *stats)
{
    return render_aov_host(spheres, n_spheres, materials, n_materials, camera, params, aov, stats);
}

int rt_release_cached(void)
{
    std::lock_guard<std::mutex> lock(g_sync_mu);
    for (auto &kv : g_sync) sync_release(kv.first, kv.second);
    g_sync.clear();
    return RT_OK;
}

int rt_render_f32(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials, uint32_t n_materials,
                  const rt_camera *camera, const rt_params *params, float *rgb_out, rt_stats *stats)
{
    if (!rgb_out) return fail(RT_ERR_INVALID, "rt_render_f32: null output");
    return render_host(spheres, n_spheres, materials, n_materials, camera, params, rgb_out, nullptr, stats);
}

int rt_render_rgb8(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials, uint32_t n_materials,
                   const rt_camera *camera, const rt_params *params, uint8_t *rgb_out, rt_stats *stats)
{
    if (!rgb_out) return fail(RT_ERR_INVALID, "rt_render_rgb8: null output");
    return render_host(spheres, n_spheres, materials, n_materials, camera, params, nullptr, rgb_out, stats);
}

} // extern "C"
