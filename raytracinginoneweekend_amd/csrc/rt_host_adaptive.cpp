// rt_host_adaptive.cpp — the adaptive session of the C-ABI (include/rt_api.h): a
// progressive session whose windows render the pixels of the blocks still active, and the stage call
// of its compaction kernel. It shares the progressive session's machinery: render_window (rt_host.cpp)
// with a block list, the Step rule, the moments accumulation. Its two kernels are rt_adaptive.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/rt_api.h"
#include "rt_device.h"
#include "rt_hip_own.h"
#include "rt_host_build.h"
#include "rt_host_sync.h"

using namespace rthost;

// One device allocation for the planes (acc, then mom, n_pixels x 3 floats each) and one for the
// block words: d_b[B], active[B], perm[0][B], perm[1][B], then the four count words. h_counts is
// their pinned copy, written by the copy that follows every compaction; ev_counts follows that copy.
struct rt_adaptive {
    rt_scene *scene = nullptr;
    int device = 0;
    rt_params p{};
    rt_adaptive_params ap{};
    rt_camera camera{};
    PixelLayout layout{};
    uint32_t n_blocks = 0;
    uint32_t done = 0;
    DevBuf<float> planes;
    float *acc = nullptr, *mom = nullptr;
    DevBuf<uint32_t> words;
    uint32_t *d_b = nullptr, *active = nullptr, *perm[2] = {nullptr, nullptr}, *d_counts = nullptr;
    PinnedBuf<uint32_t> h_counts;
    Event ev_counts;
    // the host's view of A: the list in perm[cur], its size and class counts; pending: the last step's
    // compaction has not been read back yet (adaptive_wait), perm[cur ^ 1] and h_counts then hold A
    uint32_t cur = 0, n_active = 0, cls[3] = {0, 0, 0};
    bool pending = false;
    uint64_t samples_rendered = 0;
    uint64_t geometry_epoch = 0, appearance_epoch = 0;
};

namespace {

uint64_t adaptive_plane_bytes(uint64_t n_pixels) { return n_pixels * 3u * sizeof(float); }
uint64_t adaptive_word_bytes(uint64_t n_blocks) { return (4u * n_blocks + 4u) * sizeof(uint32_t); }

int check_adaptive_params(const rt_adaptive_params *a, const std::string &w)
{
    if (!a) return fail(RT_ERR_INVALID, w + "adaptive is null");
    if (a->size != sizeof(rt_adaptive_params)) return fail(RT_ERR_INVALID, w + "adaptive.size is not sizeof(rt_adaptive_params)");
    if (!std::isfinite(a->noise_tau) || a->noise_tau < 0.f)
        return fail(RT_ERR_INVALID, w + "adaptive.noise_tau must be finite and not negative");
    if (a->max_noisy > 63u) return fail(RT_ERR_INVALID, w + "adaptive.max_noisy must be in 0..63");
    if (a->min_samples < 4u || (a->min_samples & 3u))
        return fail(RT_ERR_INVALID, w + "adaptive.min_samples must be a multiple of 4 and at least 4");
    return RT_OK;
}

// The outputs record of a step, before the session is looked at (no plane given is allowed).
int check_adaptive_outputs(const rt_adaptive_outputs *o, const std::string &w)
{
    if (!o) return RT_OK;
    if (o->size != sizeof(rt_adaptive_outputs)) return fail(RT_ERR_INVALID, w + "out.size is not sizeof(rt_adaptive_outputs)");
    const struct { const char *name; const void *ptr; } planes[5] = {
        {"rgb", o->rgb}, {"variance", o->variance}, {"rgb8", o->rgb8}, {"samples", o->samples}, {"noisy", o->noisy}};
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < i; ++j)
            if (planes[i].ptr && planes[i].ptr == planes[j].ptr)
                return fail(RT_ERR_INVALID, w + "out." + planes[i].name + " is also out." + planes[j].name);
    return RT_OK;
}

int adaptive_epochs(rt_adaptive &ad)
{
    rt_scene_motion_t sm{};
    if (int rc = rt_scene_motion(ad.scene, &sm); rc != RT_OK) return rc;
    ad.geometry_epoch = sm.geometry_epoch, ad.appearance_epoch = sm.appearance_epoch;
    return RT_OK;
}

// The host wait: the previous step's counts have arrived; A is then the list in the other buffer.
int adaptive_wait(rt_adaptive &ad, const std::string &w)
{
    if (!ad.pending) return RT_OK;
    RT_HIP(hipSetDevice(ad.device));
    RT_HIP(hipEventSynchronize(ad.ev_counts.get()));
    const uint32_t *h = ad.h_counts.get();
    ad.pending = false;
    if (h[0] > ad.n_active || static_cast<uint64_t>(h[1]) + h[2] + h[3] != h[0] || h[1] > ad.cls[0] || h[2] > ad.cls[1] ||
        h[3] > ad.cls[2])
        return fail(RT_ERR_DEVICE, w + "bad block counts from the device");
    ad.cur ^= 1u;
    ad.n_active = h[0];
    ad.cls[0] = h[1], ad.cls[1] = h[2], ad.cls[2] = h[3];
    return RT_OK;
}

void adaptive_restart(rt_adaptive &ad)
{
    ad.done = 0;
    ad.cur = 0;
    ad.n_active = ad.n_blocks;
    ad.cls[0] = ad.cls[2] = 0, ad.cls[1] = ad.n_blocks;  // (the first step takes the frame's own)
    ad.pending = false;
    ad.samples_rendered = 0;
}

} // namespace

extern "C" {

int rt_adaptive_create(rt_scene *scene, const rt_camera *camera, const rt_params *params, const rt_adaptive_params *adaptive,
                       rt_adaptive **out)
{
    const std::string w = "rt_adaptive_create: ";
    if (int rc = check_adaptive_params(adaptive, w); rc != RT_OK) return rc;
    if (int rc = check_var_params(params, "rt_adaptive_create"); rc != RT_OK) return rc;
    const PixelLayout l = pixel_layout(*params);
    if (l.n_pixels >= (1ull << 31)) return fail(RT_ERR_INVALID, w + "params: more than 2^31 pixels in one call");
    if (!l.n_pixels) return fail(RT_ERR_INVALID, w + "params: no rows to render");
    if (l.n_pixels % 64u)
        return fail(RT_ERR_UNSUPPORTED, w + "params: the pixel count " + std::to_string(l.n_pixels) +
                                            " is not a multiple of 64 (the session retires whole 64-pixel blocks)");
    if (!camera) return fail(RT_ERR_INVALID, w + "camera is null");
    if (!scene) return fail(RT_ERR_INVALID, w + "scene is null");
    if (!out) return fail(RT_ERR_INVALID, w + "out is null");
    rt_adaptive *ad = new rt_adaptive;
    ad->scene = scene;
    ad->device = scene_device(scene);
    ad->p = *params;
    ad->ap = *adaptive;
    ad->camera = *camera;
    ad->layout = l;
    const uint32_t B = ad->n_blocks = static_cast<uint32_t>(l.n_pixels / 64u);
    hipError_t e = hipSetDevice(ad->device);
    if (e == hipSuccess) e = ad->planes.alloc(2u * adaptive_plane_bytes(l.n_pixels));
    if (e == hipSuccess) e = ad->words.alloc(adaptive_word_bytes(B));
    if (e == hipSuccess) e = ad->h_counts.alloc(4 * sizeof(uint32_t), hipHostMallocDefault);
    if (e == hipSuccess) e = ad->ev_counts.make(hipEventDisableTiming);
    if (e != hipSuccess) {
        delete ad;
        return fail(RT_ERR_DEVICE, w + "the session's planes: " + hipGetErrorString(e));
    }
    ad->acc = ad->planes.get();
    ad->mom = ad->acc + 3u * l.n_pixels;
    ad->d_b = ad->words.get();
    ad->active = ad->d_b + B;
    ad->perm[0] = ad->active + B;
    ad->perm[1] = ad->perm[0] + B;
    ad->d_counts = ad->perm[1] + B;
    adaptive_restart(*ad);
    if (int rc = adaptive_epochs(*ad); rc != RT_OK) {
        (void)rt_adaptive_destroy(ad);
        return rc;
    }
    *out = ad;
    return RT_OK;
}

int rt_adaptive_step_device(rt_adaptive *ad, uint32_t n_samples, const rt_adaptive_outputs *out, void *stream,
                            uint64_t *d_segments)
{
    const std::string w = "rt_adaptive_step_device: ";
    if (int rc = check_adaptive_outputs(out, w); rc != RT_OK) return rc;
    if (!ad) return fail(RT_ERR_INVALID, w + "null session");
    uint32_t m = 0;
    if (int rc = progressive_window(w, ad->p.spp, ad->done, n_samples, &m); rc != RT_OK) return rc;
    // (done + m < 2 means done == 0, where A is every block: the rule's m is the step's)
    if (out && ad->done + m < 2u) return fail(RT_ERR_INVALID, w + "out is given but no sample is done (a resolve needs done >= 2)");
    rt_scene_motion_t sm{};
    if (int rc = rt_scene_motion(ad->scene, &sm); rc != RT_OK) return rc;
    if (sm.geometry_epoch != ad->geometry_epoch || sm.appearance_epoch != ad->appearance_epoch)
        return fail(RT_ERR_INVALID, w + "the scene was updated since the session's first step (rt_adaptive_reset starts the frame again)");
    // the host wait: this step's launches are sized by the previous step's counts
    if (int rc = adaptive_wait(*ad, w); rc != RT_OK) return rc;
    if (!ad->n_active) m = 0;  // A is empty: nothing is rendered, done stays
    const uint32_t a = ad->done, b = ad->done + m;
    if (b < 2u) return RT_OK;  // (a step of no samples on a fresh session)
    hipStream_t st = static_cast<hipStream_t>(stream);
    const PixelLayout &l = ad->layout;
    const uint32_t B = ad->n_blocks;

    WindowBlocks wb{ad->perm[ad->cur], ad->n_active, {ad->cls[0], ad->cls[1], ad->cls[2]}, nullptr};
    if (a == 0u) {
        // the session's first window: every block active with no sample, and the frame's own dealing
        // order copied into the session (the compaction kernel with every block kept)
        wb.first = [&](const uint32_t *frame_perm, uint32_t n_lead, uint32_t n_sky) -> int {
            if (static_cast<uint64_t>(n_lead) + n_sky > B) return fail(RT_ERR_DEVICE, w + "bad class counts of the frame's order");
            RT_HIP(hipMemsetAsync(ad->d_b, 0, B * sizeof(uint32_t), st));
            RT_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ad->active), 1, B, st));
            rt::KCompact kc{frame_perm, nullptr, ad->perm[0], ad->d_counts, B, B, n_lead, B - n_lead - n_sky};
            RT_HIP(rt::launch_compact_blocks(kc, st));
            ad->cur = 0;
            ad->n_active = B;
            ad->cls[0] = n_lead, ad->cls[1] = B - n_lead - n_sky, ad->cls[2] = n_sky;
            wb.d_perm = ad->perm[0];
            wb.n_active = B;
            wb.cls[0] = ad->cls[0], wb.cls[1] = ad->cls[1], wb.cls[2] = ad->cls[2];
            return RT_OK;
        };
    }
    auto after = [&]() -> int {
        if (out && out->noisy) RT_HIP(hipMemsetAsync(out->noisy, 0, sizeof(uint32_t), st));
        rt::KAdaptive k{};
        k.acc = ad->acc, k.mom = ad->mom;
        if (out) k.out = out->rgb, k.var = out->variance, k.out_u8 = out->rgb8, k.samples = out->samples, k.noisy = out->noisy;
        k.d_b = ad->d_b, k.active = ad->active;
        k.t2 = ad->ap.noise_tau * ad->ap.noise_tau;
        k.done = b;
        k.n_blocks = B;
        k.min_samples = ad->ap.min_samples, k.max_noisy = ad->ap.max_noisy;
        k.W = l.W, k.tiles_x = l.tiles_x, k.tiled_rows = l.tiled_rows, k.tile_lw = l.tile_lw;
        k.row_offset = l.row_offset, k.row_stride = l.row_stride, k.full_frame = l.full_frame;
        RT_HIP(rt::launch_adaptive_resolve(k, st));
        if (!ad->n_active) return RT_OK;  // (no block is left to retire)
        // the next step's list into the other buffer: a pass in flight reads this one
        rt::KCompact kc{ad->perm[ad->cur], ad->active, ad->perm[ad->cur ^ 1u], ad->d_counts, ad->n_active, B, ad->cls[0], ad->cls[1]};
        RT_HIP(rt::launch_compact_blocks(kc, st));
        RT_HIP(hipMemcpyAsync(ad->h_counts.get(), ad->d_counts, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        RT_HIP(hipEventRecord(ad->ev_counts.get(), st));
        ad->pending = true;
        return RT_OK;
    };
    if (int rc = render_window(ad->scene, &ad->camera, ad->p, a, b, ad->acc, ad->mom, st, d_segments, after, &wb); rc != RT_OK) {
        // (a failure part of the way leaves the planes undefined: the frame starts again)
        adaptive_restart(*ad);
        return rc;
    }
    ad->done = b;
    ad->samples_rendered += 64ull * ad->n_active * m;
    return RT_OK;
}

int rt_adaptive_info(rt_adaptive *ad, rt_adaptive_info_t *info)
{
    const std::string w = "rt_adaptive_info: ";
    if (!ad) return fail(RT_ERR_INVALID, w + "null session");
    if (!info) return fail(RT_ERR_INVALID, w + "info is null");
    if (int rc = adaptive_wait(*ad, w); rc != RT_OK) return rc;
    const uint64_t n = ad->layout.n_pixels;
    *info = rt_adaptive_info_t{static_cast<uint32_t>(sizeof(rt_adaptive_info_t)), ad->done, ad->p.spp, ad->n_blocks, ad->n_active,
                               (ad->done == ad->p.spp || !ad->n_active) ? 1u : 0u, n, ad->samples_rendered,
                               2u * adaptive_plane_bytes(n) + adaptive_word_bytes(ad->n_blocks)};
    return RT_OK;
}

int rt_adaptive_blocks(rt_adaptive *ad, uint32_t *host, uint32_t cap)
{
    const std::string w = "rt_adaptive_blocks: ";
    if (!ad) return fail(RT_ERR_INVALID, w + "null session");
    if (!host) return fail(RT_ERR_INVALID, w + "host is null");
    if (cap < ad->n_blocks) return fail(RT_ERR_CAPACITY, w + "cap is smaller than n_blocks (rt_adaptive_info)");
    if (!ad->done) {  // (nothing enqueued since creation or reset: the device words are not yet written)
        std::memset(host, 0, ad->n_blocks * sizeof(uint32_t));
        return RT_OK;
    }
    RT_HIP(hipSetDevice(ad->device));
    RT_HIP(hipDeviceSynchronize());
    RT_HIP(hipMemcpy(host, ad->d_b, ad->n_blocks * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_adaptive_reset(rt_adaptive *ad, const rt_camera *camera, const uint64_t *seed)
{
    if (!ad) return fail(RT_ERR_INVALID, "rt_adaptive_reset: null session");
    if (int rc = adaptive_epochs(*ad); rc != RT_OK) return rc;
    if (camera) ad->camera = *camera;
    if (seed) ad->p.seed = *seed;
    adaptive_restart(*ad);
    return RT_OK;
}

int rt_adaptive_destroy(rt_adaptive *ad)
{
    if (!ad) return fail(RT_ERR_INVALID, "rt_adaptive_destroy: null session");
    // (the steps enqueued may still run: the copy into the pinned words ends before they are freed)
    if (hipSetDevice(ad->device) == hipSuccess) (void)hipDeviceSynchronize();
    delete ad;
    return RT_OK;
}

int rt_block_compact_device(const uint32_t *d_src_perm, uint32_t n_blocks, const uint32_t class_counts[3],
                            const uint32_t *d_active, uint32_t *d_out_perm, uint32_t *d_counts, void *stream)
{
    const std::string w = "rt_block_compact_device: ";
    if (!d_src_perm) return fail(RT_ERR_INVALID, w + "d_src_perm is null");
    if (!class_counts) return fail(RT_ERR_INVALID, w + "class_counts is null");
    if (!d_active) return fail(RT_ERR_INVALID, w + "d_active is null");
    if (!d_out_perm) return fail(RT_ERR_INVALID, w + "d_out_perm is null");
    if (!d_counts) return fail(RT_ERR_INVALID, w + "d_counts is null");
    if (!n_blocks || n_blocks > (1u << 26)) return fail(RT_ERR_INVALID, w + "n_blocks must be in 1..2^26");
    if (static_cast<uint64_t>(class_counts[0]) + class_counts[1] + class_counts[2] != n_blocks)
        return fail(RT_ERR_INVALID, w + "class_counts do not sum to n_blocks");
    if (d_out_perm == d_src_perm) return fail(RT_ERR_INVALID, w + "d_out_perm is also d_src_perm");
    const rt::KCompact k{d_src_perm, d_active, d_out_perm, d_counts, n_blocks, n_blocks, class_counts[0], class_counts[1]};
    RT_HIP(rt::launch_compact_blocks(k, static_cast<hipStream_t>(stream)));
    return RT_OK;
}

} // extern "C"
