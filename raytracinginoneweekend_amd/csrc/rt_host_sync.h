// rt_host_sync.h — what the device half's files share (the four around the scene record, rt_scene.h:
// rt_host_scene.cpp, rt_host_order.cpp, rt_host.cpp, rt_host_synccall.cpp; rt_host_post.cpp: the
// filters, temporal accumulation and sessions; rt_host_adaptive.cpp: the adaptive session; rt_host_multi.cpp: the multi-GPU context): the
// kernels' launchers, the HIP error forms, the params checks, a scene's device and sample windows
// for those that do not see the record, and the one path every synchronous host-buffer entry point
// takes through the cached per-device context (SyncCall, implemented in rt_host_synccall.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <functional>
#include <mutex>
#include <string>

#include "../../include/rt_api.h"
#include "rt_device.h"
#include "rt_host_build.h"
#include "rt_tiles.h"

namespace rt {
// rt_kernel.hip
hipError_t launch_render(int variant, int cull, const KParams &p, uint32_t grid, hipStream_t stream, int wpb = 4);
hipError_t deep_occupancy(int variant, int wpb, size_t lds, int *blocks_per_cu, size_t *static_lds);
hipError_t occupancy_render(int variant, int cull, int *blocks_per_cu, size_t lds, bool pairs = false);
hipError_t static_lds_render(int variant, int cull, size_t *bytes, bool pairs = false);
hipError_t launch_render_list(int variant, const KList &k, uint32_t grid, hipStream_t stream);
// rt_sky.hip
hipError_t launch_sky(const KSky &k, hipStream_t stream);
hipError_t launch_sky_moments(const KSkyMoments &k, hipStream_t stream);
// rt_ground.hip
hipError_t launch_ground(int variant, const KGround &k, hipStream_t stream);
// rt_accum.hip
hipError_t launch_accumulate(const KAccum &k, hipStream_t stream);
hipError_t launch_epilogue(const float *in, uint8_t *out, uint64_t n, hipStream_t stream);
// rt_compat.hip
hipError_t launch_compat(const KCompat &k, uint32_t grid, hipStream_t stream);
hipError_t occupancy_compat(int *blocks_per_cu);
// rt_wavefront.hip
hipError_t launch_wave_gen(const KWave &w, hipStream_t stream);
hipError_t launch_wave_bounce(int cull, const KWave &w, uint32_t grid, hipStream_t stream);
hipError_t occupancy_wave_bounce(int cull, int *blocks_per_cu, size_t lds);
// rt_aov.hip
hipError_t launch_aov(int cull, const KAov &k, uint32_t grid, hipStream_t stream);
hipError_t occupancy_aov(int cull, int *blocks_per_cu, size_t lds);
hipError_t static_lds_aov(int cull, size_t *bytes);
// rt_denoise.hip
hipError_t launch_denoise(const KDenoise &k, uint32_t terms, bool demod_in, bool tiled, hipStream_t stream);
hipError_t launch_denoise_var(const KDenoiseVar &k, uint32_t terms, hipStream_t stream);
size_t denoise_tiled_lds(uint32_t terms, uint32_t step);
// rt_temporal.hip
hipError_t launch_temporal(const KTemporal &k, hipStream_t stream);
// rt_upsample.hip
hipError_t launch_upsample(const KUpsample &k, hipStream_t stream);
// rt_preview.hip
hipError_t launch_preview_split(const KPreviewSplit &k, hipStream_t stream);
hipError_t launch_preview_merge(const KPreviewMerge &k, hipStream_t stream);
// rt_progressive.hip
hipError_t launch_progressive_resolve(const KResolve &k, hipStream_t stream);
// rt_adaptive.hip
hipError_t launch_adaptive_resolve(const KAdaptive &k, hipStream_t stream);
hipError_t launch_compact_blocks(const KCompact &k, hipStream_t stream);
// rt_tiles.hip
hipError_t launch_classify_tiles(const rttile::KTiles &k, hipStream_t stream);
hipError_t launch_order_blocks(const uint8_t *cls, uint32_t n_blocks, uint32_t *perm, uint32_t *counts, hipStream_t stream);
} // namespace rt

#define RT_HIP(call)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(RT_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace rthost {

// RT_OK, or the failure "<what>: <HIP's message>"
inline int hip_rc(hipError_t e, const char *what)
{
    return e == hipSuccess ? RT_OK : fail(RT_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

// The device a scene was created on (rt_scene is rt_scene.h's record, which rt_host_post.cpp and
// rt_host_multi.cpp do not include; rt_host_scene.cpp).
int scene_device(const rt_scene *sc);

// The params of a render call, decided before any HIP call (rt_host.cpp).
int check_params(const rt_params *p);
// ... and of a variance render or a progressive session: spp >= 2, the exact kernel only.
int check_var_params(const rt_params *p, const char *who);

// The rows a call renders and how its pixels are enumerated (the natural enumeration: 64-pixel
// tiles of 2^tile_lw x 64/2^tile_lw over the tiled rows, then the other rows pixel by pixel), which
// indexes the running sums and places the outputs (accumulate_pixels, progressive_resolve).
struct PixelLayout {
    uint32_t W, num_rows, row_offset, row_stride, full_frame, tile_lw, tiles_x, tiled_rows;
    uint64_t n_pixels;
};
PixelLayout pixel_layout(const rt_params &P);

// Samples [a, b) of the P.spp-sample frame (a a multiple of 4, b one or P.spp; a == b: nothing)
// folded into acc / mom, [n_pixels][3] floats each, by the passes of a variance render that never
// reaches its last pass; then `after` on `st`; one call on the scene's stream order (rt_host.cpp).
// `blocks` (an adaptive session's step): the window renders the pixels of these
// 64-pixel blocks alone. A pass over them is a pass whose position count is 64 n_active and whose
// block permutation is d_perm; the frame's width, tiles and rows stay the frame's.
struct WindowBlocks {
    const uint32_t *d_perm;  // the blocks' natural numbers in dealing order (device), n_active entries
    uint32_t n_active;
    uint32_t cls[3];         // its lead / other / sky blocks (their sum is n_active)
    // The session's first window: called inside the call's stream order, before the render, with the
    // frame's own dealing order (frame_perm null: the identity, every block in the middle class), of
    // which it enqueues its copy on `st` and fills the fields above. Null: they are filled already.
    std::function<int(const uint32_t *frame_perm, uint32_t n_lead, uint32_t n_sky)> first;
};
int render_window(rt_scene *sc, const rt_camera *camera, const rt_params &P, uint32_t a, uint32_t b, float *acc, float *mom,
                  hipStream_t st, uint64_t *d_segments, const std::function<int()> &after, WindowBlocks *blocks = nullptr);

// The Step rule of a progressive or adaptive session (rt_host_post.cpp): *m = min(n, spp - done);
// a window that stops before the frame's end holds whole blocks of 4. `w` starts the message.
int progressive_window(const std::string &w, uint32_t spp, uint32_t done, uint32_t n, uint32_t *m);

// The scene of a synchronous render: the context keeps its device scene between calls.
struct SyncScene {
    const rt_sphere *spheres;
    uint32_t n_spheres;
    const rt_material *materials;
    uint32_t n_materials;
};

// What the Out planes are copied back as: `rows` rows of `width` pixels, from the plane's start
// one after the other (stride 0), or rows offset, offset + stride, ... of a frame that wide, each
// to the same place in the caller's frame (one hipMemcpy2D per plane).
struct SyncRows {
    size_t width, rows, offset = 0, stride = 0;
};

struct SyncSpec {
    const char *who;  // names the call where its last synchronise fails
    Plane *planes;    // in upload and download order
    size_t n_planes;
    size_t n_px;      // pixels of every plane on the device that has no count of its own (Plane::n_px)
    SyncRows rows;
    const SyncScene *scene = nullptr;  // a render: the context holds this scene before the work
    bool counters = false;  // zero the device's work counters before the work, read them after it
    bool skip = false;      // nothing to do on the device (no rows): the outputs stay as they are
};

// One synchronous host-buffer call on the current device's cached context, g_sync_mu held from
// construction to destruction. run(): the context's scene (renders), the planes laid out in its
// arena, the inputs uploaded, the cleared planes and the counters zeroed, then between the two
// timing events `enqueue` (the one device entry, on the null stream), then `after` (more work
// that is not timed), the outputs and counters copied back, and the device synchronised. Any
// failure releases the device's whole context, its scene included; the first failure's message
// stays. The wrapper's own argument checks come before the object, so before any HIP call.
class SyncCall {
public:
    SyncCall();
    int run(const SyncSpec &spec, const std::function<int()> &enqueue, const std::function<int()> &after = {});
    double wall_ms() const
    {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0_).count();
    }
    rt_scene *scene = nullptr;       // spec.scene's device scene, for `enqueue`
    uint64_t *d_counters = nullptr;  // spec.counters: the device's three counters, for `enqueue`
    uint64_t counters[3] = {0, 0, 0};  // ... and their values: segments, sphere tests, box tests
    float kernel_ms = 0.f;           // between the events around `enqueue`

private:
    std::chrono::steady_clock::time_point t0_;
    std::unique_lock<std::mutex> lock_;
};

} // namespace rthost
