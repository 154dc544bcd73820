// rt_host.cpp — the device half of the C-ABI's host side (include/rt_api.h): device scene upload,
// the stages of a render under the scene's options (kernel choice, the frame's plan from
// rt_plan.cpp, workspaces, the launches of every pass), frames in flight, the render entry points
// that replace `cuda_impl` (src/main.cxx:18, src/CUDA/cuda_impl.cu:384), and the cached context of
// the synchronous host-buffer calls with the one path they all take through it (rt_host_sync.h
// SyncCall). The multi-GPU context is rt_host_multi.cpp; the filters and temporal accumulation are
// rt_host_post.cpp; the host-only half is rt_host_build.cpp (camera and scene constructors,
// cluster builder, options, PPM writer, the synchronous calls' plane layout) and rt_plan.cpp (the
// pass planner).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <random>
#include <string>
#include <vector>

#include "../../include/rt_api.h"
#include "rt_device.h"
#include "rt_host_build.h"
#include "rt_host_sync.h"
#include "rt_plan.h"

using namespace rthost;

#ifndef RT_LONE_DEEP_TMAX
#define RT_LONE_DEEP_TMAX 4u  // the lone deep launch's transposition threshold (below)
#endif

namespace {

// counters: [kMaxWs][8 queues x kQueueStride], then [kMaxWs][4] u64 segment counters, then
// the compat kernel's counter
constexpr size_t kSegWords = kMaxWs * 8 * rt::kQueueStride;
constexpr size_t kCompatCtr = kSegWords + kMaxWs * 8 + 16;
constexpr size_t kCtrWords = kCompatCtr + rt::kQueueStride;

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

} // namespace

struct rt_scene {
    int device = 0;
    rt_options opt{};  // fixed at creation (rt_scene_create_ex)
    uint32_t n_spheres = 0, n_materials = 0;
    // scene blobs: [0] every sphere in index order (brute force), [1] big
    // spheres always tested + spatial clusters
    float *blob[2] = {nullptr, nullptr};
    uint32_t blob_units[2] = {0, 0}, n_geo[2] = {0, 0}, n_always[2] = {0, 0}, n_clusters[2] = {0, 0},
             clus_offset[2] = {0, 0};
    float clus_pad[2] = {0.f, 0.f};
    uint32_t n_supers[2] = {0, 0}, supers_offset[2] = {0, 0};
    uint32_t shade_offset[2] = {0, 0};
    // trap windows (rt_host_build.cpp trap_windows): {cos_lo, cos_hi} per sphere, then as many
    // empty windows (for renders deeper than rt::kTrapDepth); all empty under RT_DIAG_NO_TRAP_END
    float *trap = nullptr;
    bool in_fast_range = false;  // every sphere within 2^19 of the origin, radii >= 2^-40 (short exact forms)
    // workspaces: consecutive render passes (of one frame or of consecutive frames) rotate over
    // internal streams xs[b] and workspaces slots[b], so a pass renders while the caller stream
    // still accumulates the previous ones
    float *slots[kMaxWs] = {};
    size_t slots_bytes[kMaxWs] = {};
    float *acc = nullptr;
    size_t acc_bytes = 0;
    // rt_render_var_device: {L_0, m1, m2} per pixel between the passes of a frame, beside acc
    // (allocated by the first multi-pass variance render)
    float *mom = nullptr;
    size_t mom_bytes = 0;
    // deep-path split: per workspace, the pixel flags (a byte per pixel, at the front) and then
    // the deep queue (rt::DeepQueue); deep_clean = leading bytes known to be zero (every pass's
    // accumulation clears the flags it set, so only a larger pixel count needs a memset)
    void *deep[kMaxWs] = {};
    size_t deep_bytes[kMaxWs] = {}, deep_clean[kMaxWs] = {};
    // where the pair-arrival words of the queue of workspace w lay in its last layout (the
    // arrays' offsets follow the pixel count and the region capacity): zeroed again when moved
    size_t deep_meet_at[kMaxWs] = {};
    // deep-queue overflow reports (pinned host memory written by accumulate_kernel, one word per
    // workspace) and the camera keys they named, with the call that last reported each: renders
    // with such a camera are not split for kDeepOffCalls calls; at most kDeepOffKeys keys (LRU)
    unsigned long long *deep_over = nullptr, *deep_over_dev = nullptr;
    static constexpr size_t kDeepOffKeys = 8;
    static constexpr uint64_t kDeepOffCalls = 256;
    std::vector<std::pair<unsigned long long, uint64_t>> deep_off;
    void *wq = nullptr;  // RT_FLAG_WAVEFRONT: two ray queues and their counters
    size_t wq_bytes = 0;
    int occ_wave[2] = {-1, -1};  // wave_bounce_kernel blocks per CU [culled], -1 = unknown
    uint32_t *queue_ctr = nullptr;  // kCtrWords: queue and segment counters (layout at kCtrWords)
    hipStream_t xs[kMaxBufs] = {};
    hipEvent_t ev_done[kMaxWs] = {}, ev_free[kMaxWs] = {};
    hipEvent_t ev_main[kMaxWs] = {};  // split passes: after the main launch (created on first use)
    // the sky kernel of a pass issued alone runs beside the pass's main and deep launches, on the
    // next render stream (idle: nothing else runs); ev_sky after it
    hipEvent_t ev_sky = nullptr;
    bool free_valid[kMaxWs] = {};
    // queue/segment counters of workspace b not known to be zero (set while a render using
    // them is enqueued, cleared once the accumulation that resets them is enqueued after it)
    bool ctr_dirty[kMaxWs];
    rt_scene() { std::fill(std::begin(ctr_dirty), std::end(ctr_dirty), true); }
    uint32_t next_buf = 0;  // workspace of the next render pass
    int last_ws = -1;       // workspace of the last render pass issued (its ev_done), -1 = none
    // the caller stream of the previous call and an event after the last work enqueued on it:
    // a call on another stream first waits for it, so the shared accumulation buffer, the
    // compat counter and (render_streams = 1) the workspaces are never used by two streams at once
    hipStream_t last_stream = nullptr;
    hipEvent_t ev_tail = nullptr;
    bool tail_valid = false;
    int cu_count = 0;
    int occ[4][2][2];  // [variant][culled][shade records in LDS] blocks per CU, -1 = unknown
    int occ_pairs[4][2];  // the culled kernel's sample-pair instantiation, [variant][shade records in LDS]
    // [variant] blocks per CU of the 8-wave deep kernel with the whole blob in LDS, -1 = unknown,
    // 0 = it does not fit or holds no more waves than 4-wave groups (the lone deep launch)
    int occ_deep_wide[4] = {-1, -1, -1, -1};
    unsigned long long *dbg = nullptr;  // diagnostic counters (RT_DIAG_STATS)
    uint32_t dbg_waves = 0;             // waves of the last instrumented launch
    size_t max_lds = 0;
    // static LDS of the render kernel per traversal, [0] brute force, [1] culled (per-wave
    // transposed-test records and per-lane arrays; hipFuncGetAttributes)
    size_t static_lds[2] = {0, 0};
    size_t static_lds_pairs = 0;  // the culled kernel's sample-pair instantiation (its parked colours)
    // aov_kernel (rt_render_aov_device), on first use: static LDS per traversal (~0 = unknown) and
    // blocks per CU [culled][shade records in LDS] (-1 = unknown)
    size_t static_lds_aov[2] = {~static_cast<size_t>(0), ~static_cast<size_t>(0)};
    int occ_aov[2][2] = {{-1, -1}, {-1, -1}};
    // the last render's cut (rt_scene_usage_get)
    uint32_t used_streams = 0, used_ws = 0, used_pass = 0, used_deep = 0, used_pairs = 0, used_split = 0;
    uint32_t used_lead = 0, used_sky = 0;  // the last pass's tile classes
    // The ground kernel. ground_ok: the culled scene has a root box and 1 to 8
    // always-tested spheres, all lambert. Per workspace the pass's redo list (4 B per ground
    // sample; beside the planner's cut, like the orders' buffers). redo_stat: the samples redone per
    // call, by the call's ring slot; ground_samples / ground_ring: the last frame's ground samples
    // and its slot (rt_scene_ground_counts). ev_gpre / ev_ground: before and after the ground
    // kernel of a pass issued alone, which runs on another stream.
    bool ground_ok = false;
    uint32_t *redo[kMaxWs] = {};
    size_t redo_bytes[kMaxWs] = {};
    uint32_t *redo_stat = nullptr;
    uint64_t ground_samples = 0;
    uint32_t ground_ring = 0;
    uint64_t ground_call = 0;  // sc->calls of the frame ground_samples and ground_ring belong to
    hipEvent_t ev_gpre = nullptr, ev_ground = nullptr;
    // the culled scene's geometry for the tile classes of a pass, and the
    // dealing orders computed from it, per camera and rows (a pure function of those and the
    // scene, kept for the kOrders most recently used), each with its block permutation on the device
    rthost::scene_geom geom;
    bool has_geom = false;
    struct Order {
        std::vector<unsigned char> key;
        rthost::tile_order t;   // (an order computed on the device: the counts alone, perm stays empty)
        uint32_t n_blocks = 0;  // blocks of the permutation (0: the pass keeps its natural order)
        uint32_t *d_perm = nullptr;
        int slot = -1;  // >= 0: d_perm is perm_pool[slot]'s buffer, not the order's own
        uint64_t used = 0;
    };
    static constexpr size_t kOrders = 8;
    std::vector<Order> orders;
    uint64_t order_tick = 0;  // the orders' LRU clock
    uint64_t host_orders = 0, device_orders = 0, order_hits = 0;  // rt_scene_order_counts
    // Dealing orders computed on the device (rt_options.tile_classes = 1, rt_tile_order_device;
    // DESIGN.md §4.13). The geometry classify_tiles_kernel reads, uploaded at creation (KTiles::geom);
    // then, made by the first such order: a stream of the scene's own for the two kernels (the
    // caller's and the render streams hold the frames in flight) with the event the host waits
    // on, the class bytes, the counts on the device and in pinned host memory. A cached order's
    // permutation sits in a slot of perm_pool; a slot carries an event recorded after the last
    // call that read it, which the classification stream waits on before the slot is written again.
    float *d_geom = nullptr;
    uint32_t geom_boxes = 0, geom_always = 0;
    bool geom_root = false;
    float geom_pad = 0.f;
    hipStream_t tile_st = nullptr;
    hipEvent_t ev_tiles = nullptr;
    uint8_t *d_cls = nullptr;
    uint32_t cls_cap = 0;
    uint32_t *d_counts = nullptr, *h_counts = nullptr;
    struct PermSlot {
        uint32_t *d = nullptr;
        uint32_t cap = 0;
        hipEvent_t ev_read = nullptr;
        bool read_valid = false;
    };
    PermSlot perm_pool[kOrders];
    // ring of (start, end) events bracketing the render kernels of each rt_render_device call
    static constexpr uint32_t kRing = 256;
    std::vector<hipEvent_t> ev_begin, ev_end;
    uint64_t calls = 0;
    // Moving spheres (rt_scene_update). The bytes allocated behind blob[], trap and
    // d_geom: an update whose clustering needs more grows them, one that needs less keeps them. The
    // records the scene was last derived from, as an update compares them: {cx, cy, cz, r} per sphere
    // and its flattened {kind, albedo, param}. The two device tables rt_scene_motion reports, [0] the
    // current records and [1] those before the most recent update, and the two epochs.
    size_t blob_cap[2] = {0, 0}, trap_cap = 0, geom_cap = 0;
    std::vector<float> cur_table, cur_flat;
    float *centres[2] = {nullptr, nullptr};
    uint64_t geometry_epoch = 0, appearance_epoch = 0;
};

extern "C" {


int rt_device_count(int *count)
{
    if (!count) return fail(RT_ERR_INVALID, "rt_device_count: null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *count = n;
    return RT_OK;
}



} // extern "C"

namespace {



uint32_t rows_of(const rt_params &p)
{
    if (p.num_rows) return p.num_rows;
    const uint32_t st = p.row_stride ? p.row_stride : 1;
    return p.row_offset >= p.height ? 0 : (p.height - p.row_offset + st - 1) / st;
}

} // namespace

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

// The arguments of the feature-buffer calls, decided before any HIP call.
int check_aov(const rt_params *p, const rt_aov_buffers *a, const char *who)
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
    static const struct { uint32_t bit; const char *name; } unsupported[] = {
        {RT_FLAG_FAST_MATH, "RT_FLAG_FAST_MATH"}, {RT_FLAG_SCALAR_SCENE, "RT_FLAG_SCALAR_SCENE"},
        {RT_FLAG_WAVEFRONT, "RT_FLAG_WAVEFRONT"}, {RT_FLAG_CUDA_COMPAT, "RT_FLAG_CUDA_COMPAT"}};
    for (const auto &u : unsupported)
        if (p->flags & u.bit) return fail(RT_ERR_UNSUPPORTED, w + ": " + u.name + " is not supported (the exact kernel only)");
    return RT_OK;
}


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

} // namespace

struct rt_scene;
namespace {

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


// *fresh (optional): set when the buffer was (re)allocated, whatever address it got back (the
// allocator may return the freed one; ADVICE r5: callers key their resets on this, not on the address)
int ensure(void **ptr, size_t *have, size_t want, bool *fresh = nullptr)
{
    if (fresh) *fresh = false;
    if (*have >= want && *ptr) return RT_OK;
    if (fresh) *fresh = true;
    if (*ptr) {
        RT_HIP(hipDeviceSynchronize());
        RT_HIP(hipFree(*ptr));
        *ptr = nullptr;
        *have = 0;
    }
    RT_HIP(hipMalloc(ptr, std::max<size_t>(want, 256)));
    *have = want;
    return RT_OK;
}

// frees every workspace of a scene (slots, deep queues, multi-pass sums, wavefront queues)
// after the device is idle: the next render re-cuts them under max_workspace_bytes
int free_workspaces(rt_scene *sc);

// ---- what a scene derives from its records (rt_scene_create_ex and rt_scene_update) -----------
// The checks of the records, before any HIP call (who: the entry point's name).
int check_records(const char *who, const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials,
                  uint32_t n_materials)
{
    const std::string w(who);
    for (uint32_t i = 0; i < n_spheres; ++i)
        if (spheres[i].material >= n_materials)
            return fail(RT_ERR_INVALID, w + ": sphere " + std::to_string(i) + " has material index " +
                                            std::to_string(spheres[i].material) + " >= " + std::to_string(n_materials));
    for (uint32_t i = 0; i < n_materials; ++i)
        if (materials[i].kind > RT_DIELECTRIC)
            return fail(RT_ERR_INVALID, w + ": material " + std::to_string(i) + " has unknown kind");
    return RT_OK;
}

// Everything derived from the records, on the host: the one derivation both entry points install.
struct SceneDerived {
    blob_t blobs[2];             // with the shading records, kinds, dielectric constants, shortcut words
    std::vector<float> trap;     // the windows, then the empty set
    scene_geom geom;             // the tile classes' geometry, and as classify_tiles_kernel reads it
    bool has_geom = false;
    bool ground_ok = false;      // a root box and 1 to 8 always-tested spheres, all lambert
    std::vector<float> geom_words;
    bool in_fast_range = true;
    std::vector<float> table;    // [n][4] {cx, cy, cz, r}
    std::vector<float> flat;     // [n][5] {kind bits, albedo, param}
};

void derive_scene(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials, const rt_options &opt,
                  SceneDerived &d)
{
    std::vector<float> hit(static_cast<size_t>(std::max(n_spheres, 1u)) * 12, 0.f);
    d.table.resize(4 * static_cast<size_t>(n_spheres));
    d.flat.resize(5 * static_cast<size_t>(n_spheres));
    for (uint32_t i = 0; i < n_spheres; ++i) {
        const rt_sphere &sp = spheres[i];
        const rt_material &mt = materials[sp.material];
        float *h = hit.data() + 12 * static_cast<size_t>(i);
        h[0] = sp.center[0]; h[1] = sp.center[1]; h[2] = sp.center[2]; h[3] = sp.radius;
        h[4] = mt.albedo[0]; h[5] = mt.albedo[1]; h[6] = mt.albedo[2]; h[7] = mt.param;
        std::memcpy(h + 8, &mt.kind, 4);
        std::memcpy(d.table.data() + 4 * static_cast<size_t>(i), h, 16);
        float *f = d.flat.data() + 5 * static_cast<size_t>(i);
        std::memcpy(f, &mt.kind, 4);
        std::memcpy(f + 1, h + 4, 16);
    }
    d.blobs[0] = build_blob(spheres, n_spheres, false, opt.cluster_size);
    d.blobs[1] = build_blob(spheres, n_spheres, true, opt.cluster_size);
    const std::vector<uint32_t> shortcut =
        shortcut_words(spheres, n_spheres, materials, d.blobs[1], (opt.diag & RT_DIAG_NO_NEIGHBOURS) != 0);
    // shading records join each blob (so they sit in LDS next to the geometry): per original
    // sphere index {c, r}, {albedo, param}, then the material kinds as bytes, 16-B padded
    for (blob_t &b : d.blobs) {
        b.shade_offset = static_cast<uint32_t>(b.data.size() / 4);
        for (uint32_t i = 0; i < n_spheres; ++i) b.data.insert(b.data.end(), hit.data() + 12 * static_cast<size_t>(i), hit.data() + 12 * static_cast<size_t>(i) + 8);
        std::vector<uint8_t> kinds((n_spheres + 15u) / 16u * 16u, 0);
        for (uint32_t i = 0; i < n_spheres; ++i) kinds[i] = static_cast<uint8_t>(materials[spheres[i].material].kind);
        const size_t at = b.data.size();
        b.data.resize(at + kinds.size() / 4);
        std::memcpy(b.data.data() + at, kinds.data(), kinds.size());
        // dielectric constants per sphere index (raytracer.hxx:166-174 and the Schlick ratio
        // :47): {1 / ior, (1 - ior) / (1 + ior), (1 - 1/ior) / (1 + 1/ior), shortcut}, the same
        // binary32 operations the kernel would run (this file is built with -ffp-contract=off);
        // and the sphere's walk-shortcut word (shortcut_words; as raw bits)
        for (uint32_t i = 0; i < n_spheres; ++i) {
            const rt_material &mt = materials[spheres[i].material];
            float dc[4] = {0.f, 0.f, 0.f, 0.f};
            if (mt.kind == RT_DIELECTRIC) {
                const float ior = mt.param, inv = 1.f / ior;
                dc[0] = inv;
                dc[1] = (1.f - ior) / (1.f + ior);
                dc[2] = (1.f - inv) / (1.f + inv);
                std::memcpy(&dc[3], &shortcut[i], 4);
            }
            b.data.insert(b.data.end(), dc, dc + 4);
        }
    }
    d.geom = scene_geometry(spheres, d.blobs[1]);
    d.has_geom = d.blobs[1].n_clusters != 0u;
    d.ground_ok = d.has_geom && ground_scene_ok(spheres, materials, d.blobs[1], d.geom);
    d.in_fast_range = true;
    for (uint32_t i = 0; i < n_spheres; ++i) {
        for (float v : {spheres[i].center[0], spheres[i].center[1], spheres[i].center[2], spheres[i].radius})
            if (!(std::fabs(v) <= 0x1p19f)) d.in_fast_range = false;
        // the hit normal's short division by r (rt_trace.h div3_short) needs |r| >= 2^-40
        if (!(std::fabs(spheres[i].radius) >= 0x1p-40f)) d.in_fast_range = false;
    }
    // the windows, then the empty set; a scene without spheres keeps one empty window
    d.trap = trap_windows(spheres, n_spheres, materials);
    const size_t nw = std::max<size_t>(n_spheres, 1u);
    d.trap.resize(4 * nw);
    for (size_t i = (opt.diag & RT_DIAG_NO_TRAP_END) ? 0 : nw; i < 2 * nw; ++i) {
        d.trap[2 * i] = 1.f;
        d.trap[2 * i + 1] = 0.f;
    }
    if (n_spheres == 0) { d.trap[0] = 1.f; d.trap[1] = 0.f; }
    // the culled scene's geometry as classify_tiles_kernel reads it (rt_tiles.h KTiles::geom)
    const scene_geom &g = d.geom;
    d.geom_words.assign(g.root, g.root + 6);
    d.geom_words.insert(d.geom_words.end(), g.boxes.begin(), g.boxes.end());
    static_assert(sizeof(rt_sphere) == 5 * sizeof(float), "rt_sphere records follow the boxes as words");
    const size_t at = d.geom_words.size();
    d.geom_words.resize(at + 5u * g.always.size());
    if (!g.always.empty()) std::memcpy(d.geom_words.data() + at, g.always.data(), g.always.size() * sizeof(rt_sphere));
}

// Puts a derivation on the device and into the scene's fields. Every buffer that is too small (all
// of them at creation) is allocated first, then everything is uploaded, then the scene's pointers
// and counts are swapped: an allocation that fails leaves the scene as it was. The device is idle
// (an update has waited for it; at creation nothing runs yet). `first`: the creation, which also
// makes the two sphere tables, both with the records; an update swaps them and writes the current one.
int install_scene(rt_scene *sc, SceneDerived &d, bool first)
{
    struct Buf { void **ptr; size_t *cap; const void *src; size_t bytes; void *fresh; };
    Buf bufs[4] = {{(void **)&sc->blob[0], &sc->blob_cap[0], d.blobs[0].data.data(), d.blobs[0].data.size() * 4, nullptr},
                   {(void **)&sc->blob[1], &sc->blob_cap[1], d.blobs[1].data.data(), d.blobs[1].data.size() * 4, nullptr},
                   {(void **)&sc->trap, &sc->trap_cap, d.trap.data(), d.trap.size() * sizeof(float), nullptr},
                   {(void **)&sc->d_geom, &sc->geom_cap, d.geom_words.data(), d.geom_words.size() * sizeof(float), nullptr}};
    const size_t table_bytes = d.table.size() * sizeof(float);
    void *tables[2] = {nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (Buf &b : bufs)
        if (e == hipSuccess && (!*b.ptr || *b.cap < b.bytes)) e = hipMalloc(&b.fresh, std::max<size_t>(b.bytes, 256));
    for (int t = 0; first && t < 2 && e == hipSuccess; ++t) e = hipMalloc(&tables[t], std::max<size_t>(table_bytes, 256));
    for (Buf &b : bufs)
        if (e == hipSuccess && b.bytes) e = hipMemcpy(b.fresh ? b.fresh : *b.ptr, b.src, b.bytes, hipMemcpyHostToDevice);
    // (the table an update writes is the older one: it becomes the current one below)
    float *const write_table = first ? static_cast<float *>(tables[0]) : sc->centres[1];
    if (e == hipSuccess && table_bytes) e = hipMemcpy(write_table, d.table.data(), table_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && first && table_bytes) e = hipMemcpy(tables[1], d.table.data(), table_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        for (Buf &b : bufs)
            if (b.fresh) (void)hipFree(b.fresh);
        for (void *t : tables)
            if (t) (void)hipFree(t);
        return fail(RT_ERR_DEVICE, std::string("scene upload: ") + hipGetErrorString(e));
    }
    for (Buf &b : bufs)
        if (b.fresh) {
            if (*b.ptr) (void)hipFree(*b.ptr);
            *b.ptr = b.fresh;
            *b.cap = std::max<size_t>(b.bytes, 256);
        }
    if (first) sc->centres[0] = static_cast<float *>(tables[0]), sc->centres[1] = static_cast<float *>(tables[1]);
    else std::swap(sc->centres[0], sc->centres[1]);
    for (int b = 0; b < 2; ++b) {
        const blob_t &bl = d.blobs[b];
        sc->blob_units[b] = static_cast<uint32_t>(bl.data.size() / 4);
        sc->n_geo[b] = bl.n_geo;
        sc->n_always[b] = bl.n_always;
        sc->n_clusters[b] = bl.n_clusters;
        sc->clus_offset[b] = bl.clus_offset;
        sc->clus_pad[b] = bl.clus_pad;
        sc->n_supers[b] = bl.n_supers;
        sc->supers_offset[b] = bl.supers_offset;
        sc->shade_offset[b] = bl.shade_offset;
    }
    sc->geom_boxes = static_cast<uint32_t>(d.geom.boxes.size() / 6u);
    sc->geom_always = static_cast<uint32_t>(d.geom.always.size());
    sc->geom_root = d.geom.has_root;
    sc->geom_pad = d.geom.clus_pad;
    sc->has_geom = d.has_geom;
    sc->ground_ok = d.ground_ok;
    sc->geom = d.has_geom ? std::move(d.geom) : scene_geom{};
    sc->in_fast_range = d.in_fast_range;
    sc->cur_table.swap(d.table);
    sc->cur_flat.swap(d.flat);
    return RT_OK;
}

// The caches keyed by a blob's size, as a fresh scene has them: unknown.
void reset_occupancy(rt_scene *sc)
{
    for (auto &r : sc->occ) for (auto &x : r) x[0] = x[1] = -1;
    for (auto &r : sc->occ_pairs) r[0] = r[1] = -1;
    for (int &x : sc->occ_deep_wide) x = -1;
    for (auto &r : sc->occ_aov) r[0] = r[1] = -1;
    sc->occ_wave[0] = sc->occ_wave[1] = -1;
}

} // namespace

extern "C" {


int rt_scene_destroy(rt_scene *sc)
{
    if (!sc) return RT_OK;
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(sc->device);
    for (auto e : sc->ev_begin) (void)hipEventDestroy(e);
    for (auto e : sc->ev_end) (void)hipEventDestroy(e);
    for (uint32_t b = 0; b < kMaxBufs; ++b) {
        if (sc->xs[b]) (void)hipStreamSynchronize(sc->xs[b]);
        if (sc->xs[b]) (void)hipStreamDestroy(sc->xs[b]);
    }
    for (uint32_t b = 0; b < kMaxWs; ++b) {
        if (sc->ev_done[b]) (void)hipEventDestroy(sc->ev_done[b]);
        if (sc->ev_free[b]) (void)hipEventDestroy(sc->ev_free[b]);
        if (sc->ev_main[b]) (void)hipEventDestroy(sc->ev_main[b]);
    }
    if (sc->ev_tail) (void)hipEventDestroy(sc->ev_tail);
    if (sc->ev_sky) (void)hipEventDestroy(sc->ev_sky);
    if (sc->ev_gpre) (void)hipEventDestroy(sc->ev_gpre);
    if (sc->ev_ground) (void)hipEventDestroy(sc->ev_ground);
    for (uint32_t *p : sc->redo)
        if (p) (void)hipFree(p);
    if (sc->redo_stat) (void)hipFree(sc->redo_stat);
    for (void *p : {(void *)sc->blob[0], (void *)sc->blob[1], (void *)sc->dbg, (void *)sc->acc, (void *)sc->mom, (void *)sc->queue_ctr, sc->wq, (void *)sc->trap,
                    (void *)sc->centres[0], (void *)sc->centres[1]})
        if (p) (void)hipFree(p);
    for (float *p : sc->slots)
        if (p) (void)hipFree(p);
    for (void *p : sc->deep)
        if (p) (void)hipFree(p);
    if (sc->deep_over) (void)hipHostFree(sc->deep_over);
    for (auto &o : sc->orders)
        if (o.d_perm && o.slot < 0) (void)hipFree(o.d_perm);
    if (sc->tile_st) {
        (void)hipStreamSynchronize(sc->tile_st);
        (void)hipStreamDestroy(sc->tile_st);
    }
    if (sc->ev_tiles) (void)hipEventDestroy(sc->ev_tiles);
    for (auto &s : sc->perm_pool) {
        if (s.ev_read) (void)hipEventDestroy(s.ev_read);
        if (s.d) (void)hipFree(s.d);
    }
    for (void *p : {(void *)sc->d_geom, (void *)sc->d_cls, (void *)sc->d_counts})
        if (p) (void)hipFree(p);
    if (sc->h_counts) (void)hipHostFree(sc->h_counts);
    (void)hipSetDevice(prev);
    delete sc;
    return RT_OK;
}

int rt_scene_create(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials,
                    uint32_t n_materials, int device, rt_scene **out)
{
    return rt_scene_create_ex(spheres, n_spheres, materials, n_materials, device, nullptr, out);
}

int rt_scene_create_ex(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials,
                       uint32_t n_materials, int device, const rt_options *options, rt_scene **out)
{
    if (!out || (n_spheres && !spheres) || !materials || !n_materials)
        return fail(RT_ERR_INVALID, "rt_scene_create: null argument or no materials");
    *out = nullptr;
    rt_options opt;
    if (options) {
        if (int rc = check_options(*options); rc) return rc;
        opt = *options;
    } else if (int rc = default_options(opt); rc) {
        return rc;
    }
    if (int rc = check_records("rt_scene_create", spheres, n_spheres, materials, n_materials); rc != RT_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RT_ERR_DEVICE, "rt_scene_create: no HIP device");
    if (device < 0 || device >= ndev) return fail(RT_ERR_INVALID, "rt_scene_create: bad device index");
    RT_HIP(hipSetDevice(device));

    SceneDerived derived;
    derive_scene(spheres, n_spheres, materials, opt, derived);
    rt_scene *sc = new rt_scene();
    sc->opt = opt;
    reset_occupancy(sc);
    sc->device = device;
    sc->n_spheres = n_spheres;
    sc->n_materials = n_materials;
    int rc = install_scene(sc, derived, true);
    if (rc == RT_OK) {
        hipError_t e = hipMalloc((void **)&sc->queue_ctr, kCtrWords * sizeof(uint32_t));
        if (e != hipSuccess) rc = fail(RT_ERR_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(e));
        if (rc == RT_OK &&
            (hipHostMalloc((void **)&sc->deep_over, kMaxWs * sizeof(unsigned long long), hipHostMallocMapped) != hipSuccess ||
             hipHostGetDevicePointer((void **)&sc->deep_over_dev, sc->deep_over, 0) != hipSuccess))
            rc = fail(RT_ERR_DEVICE, "rt_scene_create: pinned host allocation failed");
        if (rc == RT_OK) std::memset(sc->deep_over, 0, kMaxWs * sizeof(unsigned long long));
        for (uint32_t b = 0; b < kMaxWs && rc == RT_OK; ++b) {
            if ((b < kMaxBufs && hipStreamCreateWithFlags(&sc->xs[b], hipStreamNonBlocking) != hipSuccess) ||
                hipEventCreateWithFlags(&sc->ev_done[b], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&sc->ev_free[b], hipEventDisableTiming) != hipSuccess)
                rc = fail(RT_ERR_DEVICE, "rt_scene_create: stream/event creation failed");
        }
        if (rc == RT_OK && (hipEventCreateWithFlags(&sc->ev_tail, hipEventDisableTiming) != hipSuccess ||
                            hipEventCreateWithFlags(&sc->ev_sky, hipEventDisableTiming) != hipSuccess))
            rc = fail(RT_ERR_DEVICE, "rt_scene_create: event creation failed");
    }
    if (rc == RT_OK) {
        hipDeviceProp_t prop;
        hipError_t e = hipGetDeviceProperties(&prop, device);
        if (e != hipSuccess) rc = fail(RT_ERR_DEVICE, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
        else {
            sc->cu_count = prop.multiProcessorCount;
            sc->max_lds = prop.sharedMemPerBlock;
        }
    }
    if (rc == RT_OK) {
        hipError_t e = rt::static_lds_render(rt::V_EXACT_LDS, 0, &sc->static_lds[0]);
        if (e == hipSuccess) e = rt::static_lds_render(rt::V_EXACT_LDS, 7, &sc->static_lds[1]);
        if (e == hipSuccess) e = rt::static_lds_render(rt::V_EXACT_LDS, 7, &sc->static_lds_pairs, true);
        if (e != hipSuccess) rc = fail(RT_ERR_DEVICE, std::string("hipFuncGetAttributes: ") + hipGetErrorString(e));
    }
    for (uint32_t i = 0; rc == RT_OK && i < rt_scene::kRing; ++i) {
        hipEvent_t a = nullptr, b = nullptr;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
            if (a) (void)hipEventDestroy(a);
            rc = fail(RT_ERR_DEVICE, "hipEventCreate failed");
            break;
        }
        sc->ev_begin.push_back(a);
        sc->ev_end.push_back(b);
    }
    if (rc != RT_OK) {
        rt_scene_destroy(sc);
        return rc;
    }
    *out = sc;
    return RT_OK;
}

} // extern "C"

namespace {
// ---- dealing orders computed on the device --------------------------------
// order_blocks_kernel is one workgroup that walks the blocks 1024 at a time: passes above this
// many blocks (a 8192 x 8192 frame) have their order computed on the host under tile_classes = 1
constexpr uint32_t kDeviceOrderMaxBlocks = 1u << 20;

// The classification's stream, event, class bytes and counts, made on first use and grown to
// n_blocks class bytes (nothing of an earlier classification is in flight then: every one ends
// with the host waiting for it).
int tiles_ready(rt_scene *sc, uint32_t n_blocks)
{
    // (a stream of the default priority: one of the highest priority, and the kernels' waves at a
    // raised issue priority, were measured and did not help)
    if (!sc->tile_st) RT_HIP(hipStreamCreateWithFlags(&sc->tile_st, hipStreamNonBlocking));
    if (!sc->ev_tiles) RT_HIP(hipEventCreateWithFlags(&sc->ev_tiles, hipEventDisableTiming));
    if (!sc->d_counts) RT_HIP(hipMalloc((void **)&sc->d_counts, 2 * sizeof(uint32_t)));
    if (!sc->h_counts) RT_HIP(hipHostMalloc((void **)&sc->h_counts, 2 * sizeof(uint32_t), hipHostMallocDefault));
    if (sc->cls_cap < n_blocks) {
        if (sc->d_cls) RT_HIP(hipFree(sc->d_cls));
        sc->d_cls = nullptr;
        sc->cls_cap = 0;
        const uint32_t cap = (n_blocks + 4095u) & ~4095u;
        RT_HIP(hipMalloc((void **)&sc->d_cls, cap));
        sc->cls_cap = cap;
    }
    return RT_OK;
}

// The blocks of a pass as classify_tiles counts them (rt_host_build.cpp): n_blocks = 0 when the
// pass keeps its natural order, n_tiles = 0 when its width is not a multiple of the tile's.
void pass_tiles(uint32_t W, uint32_t H, uint32_t row_offset, uint32_t row_stride, uint32_t num_rows, uint32_t tile_lw,
                rttile::KTiles &k)
{
    k.n_blocks = k.n_tiles = 0;
    const uint64_t n_pixels = static_cast<uint64_t>(W) * num_rows;
    if (!W || !H || n_pixels == 0 || n_pixels % 64u || tile_lw > 6u) return;
    k.n_blocks = static_cast<uint32_t>(n_pixels / 64u);
    const uint32_t tw = 1u << tile_lw, th = 64u >> tile_lw;
    const bool tiled = W % tw == 0u;
    const uint32_t tiles_x = tiled ? W / tw : 1u, tiled_rows = tiled ? (num_rows / th) * th : 0u;
    k.n_tiles = tiled ? tiles_x * (tiled_rows / th) : 0u;
    k.pass = {W, H, row_offset, row_stride ? row_stride : 1u, tw, th, tiles_x};
}

// Enqueues the two kernels and the copy of the counts to sc->h_counts on `st`: the class bytes of
// the pass k describes, then d_perm (null: none) and the counts.
int enqueue_device_order(rt_scene *sc, const rt_camera &cam, rttile::KTiles &k, uint32_t *d_perm, hipStream_t st)
{
    k.cam = cam;
    k.geom = sc->d_geom;
    k.has_root = sc->geom_root ? 1u : 0u;
    k.n_boxes = sc->geom_boxes;
    k.n_always = sc->geom_always;
    k.clus_pad = sc->geom_pad;
    k.cls = sc->d_cls;
    RT_HIP(rt::launch_classify_tiles(k, st));
    RT_HIP(rt::launch_order_blocks(sc->d_cls, k.n_blocks, d_perm, sc->d_counts, st));
    RT_HIP(hipMemcpyAsync(sc->h_counts, sc->d_counts, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return RT_OK;
}

// The least recently used order leaves when kOrders are cached. One with a permutation of its own
// (computed on the host) is freed once the device is idle: renders in flight may still read it.
// One in a pool slot just leaves: the slot's event guards its next use.
int evict_order(rt_scene *sc)
{
    if (sc->orders.size() < rt_scene::kOrders) return RT_OK;
    auto lru = std::min_element(sc->orders.begin(), sc->orders.end(),
                                [](const rt_scene::Order &a, const rt_scene::Order &b) { return a.used < b.used; });
    if (lru->d_perm && lru->slot < 0) {
        RT_HIP(hipDeviceSynchronize());
        RT_HIP(hipFree(lru->d_perm));
    }
    sc->orders.erase(lru);
    return RT_OK;
}

// A miss under tile_classes = 1: the order of the pass in a free slot of the pool, by the two
// kernels on the scene's own stream. The host waits for that stream's event alone (it needs the
// counts to size the launches), and the caller's stream waits for it too.
int device_order(rt_scene *sc, const rt_camera &cam, rttile::KTiles &kt, hipStream_t st, rt_scene::Order &e)
{
    if (int rc = evict_order(sc); rc) return rc;
    int slot = -1;
    for (int i = 0; i < static_cast<int>(rt_scene::kOrders) && slot < 0; ++i) {
        bool taken = false;
        for (const auto &o : sc->orders) taken = taken || o.slot == i;
        if (!taken) slot = i;
    }
    if (slot < 0) return fail(RT_ERR_DEVICE, "pass_order: no free permutation slot");
    if (int rc = tiles_ready(sc, kt.n_blocks); rc) return rc;
    if (sc->perm_pool[slot].cap < kt.n_blocks) {
        // a larger pass than the pool was cut for: every slot no cached order holds grows to it
        // (the first order of a scene allocates them all), after the last call that read it
        for (int i = 0; i < static_cast<int>(rt_scene::kOrders); ++i) {
            rt_scene::PermSlot &p = sc->perm_pool[i];
            bool taken = false;
            for (const auto &o : sc->orders) taken = taken || o.slot == i;
            if (taken || p.cap >= kt.n_blocks) continue;
            if (!p.ev_read) RT_HIP(hipEventCreateWithFlags(&p.ev_read, hipEventDisableTiming));
            if (p.read_valid) RT_HIP(hipEventSynchronize(p.ev_read));
            p.read_valid = false;
            if (p.d) RT_HIP(hipFree(p.d));
            p.d = nullptr;
            p.cap = 0;
            RT_HIP(hipMalloc((void **)&p.d, static_cast<size_t>(kt.n_blocks) * sizeof(uint32_t)));
            p.cap = kt.n_blocks;
        }
    }
    rt_scene::PermSlot &p = sc->perm_pool[slot];
    if (p.read_valid) RT_HIP(hipStreamWaitEvent(sc->tile_st, p.ev_read, 0));
    if (int rc = enqueue_device_order(sc, cam, kt, p.d, sc->tile_st); rc) return rc;
    RT_HIP(hipEventRecord(sc->ev_tiles, sc->tile_st));
    RT_HIP(hipEventSynchronize(sc->ev_tiles));
    RT_HIP(hipStreamWaitEvent(st, sc->ev_tiles, 0));
    e.t.n_lead = sc->h_counts[0];
    e.t.n_sky = sc->h_counts[1];
    if (static_cast<uint64_t>(e.t.n_lead) + e.t.n_sky > kt.n_blocks) return fail(RT_ERR_DEVICE, "pass_order: bad class counts from the device");
    e.n_blocks = kt.n_blocks;
    e.d_perm = p.d;
    e.slot = slot;
    return RT_OK;
}

// The dealing order of a pass over these rows with this camera (rt_scene::orders; computed on a
// miss: classify_tiles on the host, the permutation uploaded once; or, under tile_classes = 1
// for a pass whose tiles are classified at all, on the device: device_order). `st`: the stream
// of the call, on which order_used is recorded once the call's last reader is enqueued.
int pass_order(rt_scene *sc, const rt_camera &cam, const rt::KParams &k, hipStream_t st, const rt_scene::Order **out)
{
    *out = nullptr;
    std::vector<unsigned char> key(sizeof(rt_camera) + 7 * sizeof(uint32_t));
    const uint32_t g[7] = {k.W, k.H, k.row_offset, k.row_stride, k.num_rows, k.tile_lw, 0u};
    std::memcpy(key.data(), &cam, sizeof(rt_camera));
    std::memcpy(key.data() + sizeof(rt_camera), g, sizeof(g));
    for (auto &o : sc->orders)
        if (o.key == key) {
            o.used = ++sc->order_tick;
            ++sc->order_hits;
            *out = &o;
            return RT_OK;
        }
    rt_scene::Order e;
    e.key.swap(key);
    if (sc->opt.tile_classes == 1u) {
        rttile::KTiles kt{};
        pass_tiles(k.W, k.H, k.row_offset, k.row_stride, k.num_rows, k.tile_lw, kt);
        if (kt.n_tiles && kt.n_blocks <= kDeviceOrderMaxBlocks) {
            if (int rc = device_order(sc, cam, kt, st, e); rc) return rc;
            ++sc->device_orders;
            e.used = ++sc->order_tick;
            sc->orders.push_back(std::move(e));
            *out = &sc->orders.back();
            return RT_OK;
        }
    }
    e.t = classify_tiles(cam, k.W, k.H, k.row_offset, k.row_stride, k.num_rows, k.tile_lw, sc->geom);
#ifdef RT_ORDER_IDENTITY  // A/B build switch: the class machinery over the natural order (one middle group)
    for (uint32_t i = 0; i < e.t.perm.size(); ++i) e.t.perm[i] = i;
    e.t.n_lead = e.t.n_sky = 0;
#endif
    e.n_blocks = static_cast<uint32_t>(e.t.perm.size());
    ++sc->host_orders;
    if (!e.t.perm.empty()) {
        RT_HIP(hipMalloc((void **)&e.d_perm, e.t.perm.size() * sizeof(uint32_t)));
        const hipError_t ce = hipMemcpy(e.d_perm, e.t.perm.data(), e.t.perm.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (ce != hipSuccess) {
            (void)hipFree(e.d_perm);
            return fail(RT_ERR_DEVICE, std::string("hipMemcpy: ") + hipGetErrorString(ce));
        }
    }
    if (int rc = evict_order(sc); rc) return rc;
    e.used = ++sc->order_tick;
    sc->orders.push_back(std::move(e));
    *out = &sc->orders.back();
    return RT_OK;
}

// After the last work of a call that reads the order's permutation is enqueued on (or ordered
// before the tail of) `st`: a permutation in a pool slot is not written again before that work.
int order_used(rt_scene *sc, const rt_scene::Order *ord, hipStream_t st)
{
    if (!ord || ord->slot < 0) return RT_OK;
    rt_scene::PermSlot &p = sc->perm_pool[ord->slot];
    RT_HIP(hipEventRecord(p.ev_read, st));
    p.read_valid = true;
    return RT_OK;
}

int free_workspaces(rt_scene *sc)
{
    RT_HIP(hipDeviceSynchronize());
    auto drop = [](void *&p, size_t &n) -> hipError_t {
        hipError_t e = hipSuccess;
        if (p) e = hipFree(p);
        p = nullptr;
        n = 0;
        return e;
    };
    for (uint32_t w = 0; w < kMaxWs; ++w) {
        void *sp = sc->slots[w];
        RT_HIP(drop(sp, sc->slots_bytes[w]));
        sc->slots[w] = nullptr;
        RT_HIP(drop(sc->deep[w], sc->deep_bytes[w]));
        void *rp = sc->redo[w];
        RT_HIP(drop(rp, sc->redo_bytes[w]));
        sc->redo[w] = nullptr;
        sc->deep_clean[w] = 0;
        sc->deep_meet_at[w] = 0;
    }
    void *ap = sc->acc;
    RT_HIP(drop(ap, sc->acc_bytes));
    sc->acc = nullptr;
    void *mp = sc->mom;
    RT_HIP(drop(mp, sc->mom_bytes));
    sc->mom = nullptr;
    RT_HIP(drop(sc->wq, sc->wq_bytes));
    return RT_OK;
}
} // namespace

namespace {
// Calls on one scene may come on different caller streams: order a call after everything the
// previous call enqueued on its stream (the accumulation buffer and counters are
// per scene), then remember this call's stream and its last work.
int stream_enter(rt_scene *sc, hipStream_t st)
{
    if (sc->tail_valid && st != sc->last_stream) RT_HIP(hipStreamWaitEvent(st, sc->ev_tail, 0));
    return RT_OK;
}
int stream_leave(rt_scene *sc, hipStream_t st)
{
    RT_HIP(hipEventRecord(sc->ev_tail, st));
    sc->last_stream = st;
    sc->tail_valid = true;
    return RT_OK;
}
// A sample window of a frame (a progressive session's step): samples [a, b) of
// the P.spp-sample frame, a a multiple of 4 and b a multiple of 4 or P.spp, folded into the caller's
// own planes (indexed like KAccum::acc / KAccum::mom) and never divided: no pass of a window is
// the frame's last.
struct Window {
    uint32_t a, b;
    float *acc, *mom;
};
int render_device_impl(rt_scene *sc, const rt_camera *camera, const rt_params &P, float *d_rgb, hipStream_t st,
                       uint64_t *d_segments, float *d_var = nullptr, const Window *win = nullptr);
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
    static const struct { uint32_t bit; const char *name; } unsupported[] = {
        {RT_FLAG_FAST_MATH, "RT_FLAG_FAST_MATH"}, {RT_FLAG_SCALAR_SCENE, "RT_FLAG_SCALAR_SCENE"},
        {RT_FLAG_WAVEFRONT, "RT_FLAG_WAVEFRONT"}, {RT_FLAG_CUDA_COMPAT, "RT_FLAG_CUDA_COMPAT"}};
    for (const auto &u : unsupported)
        if (p->flags & u.bit) return fail(RT_ERR_UNSUPPORTED, w + ": " + u.name + " is not supported (the exact kernel only)");
    return RT_OK;
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

// A progressive session's step (rt_host_post.cpp): samples [a, b) of the frame into the session's
// planes as one call on the scene (a == b: no render), then `after` (the resolve, which reads
// those planes) on the caller's stream, inside the call's stream order.
int rthost::render_window(rt_scene *sc, const rt_camera *camera, const rt_params &P, uint32_t a, uint32_t b, float *acc,
                          float *mom, hipStream_t st, uint64_t *d_segments, const std::function<int()> &after)
{
    RT_HIP(hipSetDevice(sc->device));
    if (int rc = stream_enter(sc, st); rc != RT_OK) return rc;
    const Window win{a, b, acc, mom};
    if (a < b)
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
    k.n_spheres = sc->n_spheres;
    k.n_materials = sc->n_materials;
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
    bool cull = !(P.flags & RT_FLAG_BRUTE_FORCE) && sc->n_clusters[1] > 0;
    const bool wave = (P.flags & RT_FLAG_WAVEFRONT) != 0u;
    if (wave && (P.flags & (RT_FLAG_FAST_MATH | RT_FLAG_SCALAR_SCENE)))
        return fail(RT_ERR_UNSUPPORTED, "rt_render_device: the wavefront variant is the exact kernel only");
    if (P.flags & RT_FLAG_SCALAR_SCENE) { variant = rt::V_EXACT_SCALAR; cull = false; }
    if (variant != rt::V_EXACT_SCALAR && static_cast<size_t>(sc->shade_offset[cull]) * 16u + sc->static_lds[cull] > sc->max_lds) {
        if (variant == rt::V_FAST_LDS || cull) return fail(RT_ERR_UNSUPPORTED, "rt_render_device: scene too large for LDS");
        variant = rt::V_EXACT_SCALAR;
    }
    if (wave && variant != rt::V_EXACT_LDS)
        return fail(RT_ERR_UNSUPPORTED, "rt_render_device: the wavefront variant needs the scene in LDS");
    if (variant == rt::V_EXACT_LDS && (O.diag & RT_DIAG_STATS) && !wave) {
        variant = rt::V_STATS_LDS;
        if (!sc->dbg) {
            RT_HIP(hipMalloc((void **)&sc->dbg, rt::kDbgWords * sizeof(unsigned long long)));
            RT_HIP(hipMemset(sc->dbg, 0, rt::kDbgWords * sizeof(unsigned long long)));
        }
        k.dbg = sc->dbg;
    }
    const int b = cull ? 1 : 0;
    const int cull_mode = cull ? 7 : 0;
    k.blob = reinterpret_cast<const float4 *>(sc->blob[b]);
    k.blob_units = sc->blob_units[b];
    k.n_geo = sc->n_geo[b];
    k.n_always = sc->n_always[b];
    k.n_clusters = sc->n_clusters[b];
    k.clus_offset = sc->clus_offset[b];
    k.clus_pad = sc->clus_pad[b];
    k.n_supers = sc->n_supers[b];
    k.supers_offset = sc->supers_offset[b];
    k.use_root = (O.diag & RT_DIAG_NO_ROOT_BOX) ? 0u : 1u;
    k.iso = (O.diag & RT_DIAG_NO_SHORTCUT) ? 0u : 1u;
    k.transpose_max = O.transpose_max;
    k.diag_unbounded_nb = (O.diag & RT_DIAG_UNBOUNDED_NB) ? 1u : 0u;
    k.fast_roots = sc->in_fast_range && camera_in_fast_range(camera) && !(O.diag & RT_DIAG_IEEE_ROOTS) ? 1u : 0u;
    k.shade_offset = sc->shade_offset[b];
    // the windows hold for paths of at most rt::kTrapDepth segments: deeper renders get the empty set
    k.trap = reinterpret_cast<const float2 *>(sc->trap) +
             (P.max_depth > rt::kTrapDepth ? std::max<size_t>(sc->n_spheres, 1u) : 0u);
    auto occ_for = [&](int in_lds, int *out) -> int {
        int &o = sc->occ[variant][b][in_lds];
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
    c.order_ok = sc->has_geom && cull_mode == 7 && !wave && variant != rt::V_EXACT_SCALAR && !(O.diag & RT_DIAG_NATURAL_ORDER);
    return RT_OK;
}

// the pair instantiation's own occupancy (its parked colours add static LDS): the
// grid of a paired pass is sized by it
int pair_occupancy(rt_scene *sc, const rt::KParams &k, KernelChoice &c)
{
    if (!c.pairs_ok) return RT_OK;
    int &o = sc->occ_pairs[c.variant][k.shade_lds ? 1 : 0];
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
        const unsigned long long v = __atomic_exchange_n(sc->deep_over + w, 0ull, __ATOMIC_ACQ_REL);
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
            after += used ? std::max<uint64_t>(sc->slots_bytes[w], pl.slot_bytes(w)) : sc->slots_bytes[w];
            after += used && in.may_split ? std::max<uint64_t>(sc->deep_bytes[w], pl.deep_bytes(w)) : sc->deep_bytes[w];
        }
        after += multi_pass ? std::max<uint64_t>(sc->acc_bytes, per_sample) : sc->acc_bytes;
        after += multi_pass && in.moments ? std::max<uint64_t>(sc->mom_bytes, per_sample) : sc->mom_bytes;
        after += in.wave ? std::max<uint64_t>(sc->wq_bytes, pl.wave_bytes()) : sc->wq_bytes;
        if (after > in.max_workspace_bytes)
            if (int rc = free_workspaces(sc); rc) return rc;
    }
    sc->used_streams = pl.streams;
    sc->used_ws = pl.n_ws + (pl.has_lone() ? 1u : 0u);
    sc->used_pass = static_cast<uint32_t>(pl.ring_samples);
    sc->used_deep = 0;
    sc->used_pairs = sc->used_split = sc->used_lead = sc->used_sky = 0;
    if (multi_pass)
        if (int rc = ensure((void **)&sc->acc, &sc->acc_bytes, per_sample); rc) return rc;
    if (multi_pass && in.moments)
        if (int rc = ensure((void **)&sc->mom, &sc->mom_bytes, per_sample); rc) return rc;
    for (uint32_t w = 0; w < pl.n_ws; ++w)
        if (int rc = ensure((void **)&sc->slots[w], &sc->slots_bytes[w], pl.slot_bytes(w)); rc) return rc;
    if (pl.has_lone())
        if (int rc = ensure((void **)&sc->slots[pl.lone_ws], &sc->slots_bytes[pl.lone_ws], pl.slot_bytes(pl.lone_ws)); rc) return rc;
    if (in.wave) {
        wq.cap = pl.wave_cap;
        const size_t qbytes = static_cast<size_t>(wq.cap) * 52u;
        if (int rc = ensure(&sc->wq, &sc->wq_bytes, 2 * qbytes + 512); rc) return rc;
        auto carve = [&](char *base, rt::RayQueue &q) {
            q.f = reinterpret_cast<float *>(base);
            q.rng = reinterpret_cast<uint64_t *>(base + static_cast<size_t>(wq.cap) * 36u);
            q.item = reinterpret_cast<uint32_t *>(base + static_cast<size_t>(wq.cap) * 44u);
            q.depth = reinterpret_cast<uint32_t *>(base + static_cast<size_t>(wq.cap) * 48u);
        };
        char *w0 = static_cast<char *>(sc->wq);
        carve(w0, wq.a);
        carve(w0 + qbytes, wq.b);
        wq.a.count = reinterpret_cast<uint32_t *>(w0 + 2 * qbytes);
        wq.b.count = reinterpret_cast<uint32_t *>(w0 + 2 * qbytes + 256);
        int &ow = sc->occ_wave[c.cull ? 1 : 0];
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
    const rt_scene::Order *ord;  // the frame's dealing order, if any
    bool sky_kernel;             // the proven-sky tiles are rendered by sky_kernel at the last pass
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
    return reinterpret_cast<unsigned long long *>(sc->queue_ctr + kSegWords) + 4u * wb;
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
    p.xst = f.pipe() ? sc->xs[wb % pl.streams] : f.st;
    k.slots = sc->slots[wb];
    k.queue_ctr = sc->queue_ctr + wb * 8u * rt::kQueueStride;
    unsigned long long *seg_b = seg_counters(sc, wb);
    k.segments = f.d_segments ? (f.pipe() ? seg_b : reinterpret_cast<unsigned long long *>(f.d_segments)) : nullptr;
    if (f.pipe() && sc->free_valid[wb]) RT_HIP(hipStreamWaitEvent(p.xst, sc->ev_free[wb], 0));
    if (sc->ctr_dirty[wb]) {
        RT_HIP(hipMemsetAsync(k.queue_ctr, 0, 8 * rt::kQueueStride * sizeof(uint32_t), p.xst));
        RT_HIP(hipMemsetAsync(seg_b, 0, 3 * sizeof(unsigned long long), p.xst));
    }
    sc->ctr_dirty[wb] = true;
    if (p.s0 == f.s_begin) RT_HIP(hipEventRecord(sc->ev_begin[f.ring], p.xst));
    k.sample_begin = p.s0;
    k.sample_end = p.s1;
    k.n_pair_items = static_cast<uint32_t>(((p.s1 - p.s0) - pl.slot_rows(p.s0, p.s1, p.pass_pairs)) * pl.in.n_pixels);
    if (k.n_pair_items) ++sc->used_pairs;
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
    const rt_scene::Order *ord = f.ord;
    const uint64_t n_pixels = k.n_pixels;
    const uint32_t s0 = p.s0, s1 = p.s1;
    p.ordered = ord && ord->d_perm && !k.n_pair_items;
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
    if (!p.in_flight && f.sky_kernel && p.ordered && s1 == f.P.spp && f.pipe() && !(sc->opt.diag & RT_DIAG_SKY_SERIAL)) {
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
        const rthost::tile_order &t = ord->t;
        const uint64_t S = s1 - s0;
        const uint64_t nbl[3] = {t.n_lead, ord->n_blocks - t.n_lead - t.n_sky, f.sky_kernel ? 0u : t.n_sky};
        k.block_perm = ord->d_perm;
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
        sc->used_lead = t.n_lead;
        sc->used_sky = f.sky_kernel ? t.n_sky : 0u;
    } else {
        sc->used_lead = sc->used_sky = 0;
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
    if (int rc = ensure(&sc->deep[wb], &sc->deep_bytes[wb], deep_queue_bytes(n_pixels, n_samples), &fresh); rc)
        return rc;
    if (fresh) {  // new memory: no flag set, no pair arrival counted
        sc->deep_clean[wb] = 0;
        RT_HIP(hipMemsetAsync(sc->deep[wb], 0, sc->deep_bytes[wb], p.xst));
    } else if (sc->deep_meet_at[wb] != px_bytes + static_cast<size_t>(cap) * 56u) {
        // another layout: its arrival words lie where other arrays were (every pass that
        // keeps the layout leaves them zero: the second arrival of a pair resets its word)
        RT_HIP(hipMemsetAsync(static_cast<char *>(sc->deep[wb]) + px_bytes + static_cast<size_t>(cap) * 56u, 0,
                              static_cast<size_t>(cap) * 4u, p.xst));
    }
    sc->deep_meet_at[wb] = px_bytes + static_cast<size_t>(cap) * 56u;
    if (sc->deep_clean[wb] < px_bytes)  // flags over bytes a queue may have used
        RT_HIP(hipMemsetAsync(sc->deep[wb], 0, px_bytes, p.xst));
    // every accumulation clears the flags its pass set, and the bytes past px_bytes are
    // this pass's queue storage: only the leading px_bytes are known to be zero after it
    sc->deep_clean[wb] = px_bytes;
    char *base = static_cast<char *>(sc->deep[wb]);
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

// The main launch on the pass's stream, and ev_main after it where the first part of the
// accumulation waits for it alone.
int launch_main(const Frame &f, Pass &p, const rt::KParams &k)
{
    rt_scene *sc = f.sc;
    RT_HIP(rt::launch_render(f.c.variant, f.c.cull_mode, k, p.grid, p.xst));
    p.stats_waves = p.grid * 4u;
    if (p.two_part && !p.ground) {  // (with a ground kernel: after the redo launch)
        if (!sc->ev_main[p.wb]) RT_HIP(hipEventCreateWithFlags(&sc->ev_main[p.wb], hipEventDisableTiming));
        RT_HIP(hipEventRecord(sc->ev_main[p.wb], p.xst));
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
    if (int rc = ensure((void **)&sc->redo[wb], &sc->redo_bytes[wb], n_samples * sizeof(uint32_t)); rc) return rc;
    if (!sc->redo_stat) {
        RT_HIP(hipMalloc((void **)&sc->redo_stat, rt_scene::kRing * sizeof(uint32_t)));
        RT_HIP(hipMemset(sc->redo_stat, 0, rt_scene::kRing * sizeof(uint32_t)));
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
        RT_HIP(hipMemsetAsync(sc->redo_stat + (sc->ground_ring + rt_scene::kRing / 2u) % rt_scene::kRing, 0, sizeof(uint32_t), p.xst));
    }
    sc->ground_samples += n_samples;
    redo = rt::RedoList{sc->redo[wb], k.queue_ctr, static_cast<uint32_t>(n_samples), sc->redo_stat + sc->ground_ring};
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
    if (!sc->ev_gpre) RT_HIP(hipEventCreateWithFlags(&sc->ev_gpre, hipEventDisableTiming));
    if (!sc->ev_ground) RT_HIP(hipEventCreateWithFlags(&sc->ev_ground, hipEventDisableTiming));
    // (the stream after the sky kernel's: consecutive render streams sit on different queues)
    hipStream_t g_st = sc->xs[(wb % f.pl.streams + 2u) % f.pl.streams];
    RT_HIP(hipEventRecord(sc->ev_gpre, p.xst));
    RT_HIP(hipStreamWaitEvent(g_st, sc->ev_gpre, 0));
    RT_HIP(rt::launch_ground(f.c.variant, g, g_st));
    RT_HIP(hipEventRecord(sc->ev_ground, g_st));
    return RT_OK;
}

// The redo launch of a pass with a ground kernel: the punted samples from scratch through the
// general kernel's list instantiation, a fixed grid of one workgroup per CU (the count is on the
// device); its paths reach the deep queue like the main launch's.
int launch_redo(const Frame &f, const Pass &p, const rt::KParams &k, const rt::RedoList &redo)
{
    if (p.ground_aside) RT_HIP(hipStreamWaitEvent(p.xst, f.sc->ev_ground, 0));
    const rt::KList kl{k, redo};
    rt_scene *sc = f.sc;
    RT_HIP(rt::launch_render_list(f.c.variant, kl, static_cast<uint32_t>(std::max(1, sc->cu_count)), p.xst));
    // the first part of the accumulation reads the ground tiles' slots too: ev_main after this launch
    if (p.two_part) {
        if (!sc->ev_main[p.wb]) RT_HIP(hipEventCreateWithFlags(&sc->ev_main[p.wb], hipEventDisableTiming));
        RT_HIP(hipEventRecord(sc->ev_main[p.wb], p.xst));
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
    ++sc->used_split;
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
        int &ow = sc->occ_deep_wide[variant];
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
        RT_HIP(hipMemsetAsync(sc->dbg, 0, 16 * sizeof(unsigned long long), p.xst));
        RT_HIP(hipMemsetAsync(sc->dbg + rt::kDbgEvBase, 0, rt::kDbgEvents * sizeof(unsigned long long), p.xst));
    }
    RT_HIP(rt::launch_render(variant, f.c.cull_mode, kd, dgrid, p.xst, wpb));
    sc->used_deep = static_cast<uint32_t>(wpb) | (kd.deep_static ? 16u : 0u);
    if (stats_deep_only) p.stats_waves = dgrid * static_cast<uint32_t>(wpb);
    return RT_OK;
}

// The sky kernel at the frame's last pass: the sky tiles' pixels, every sample of the frame;
// position i's sum to its sample-0 slot (which no pass of these groups uses), read by this
// pass's accumulation. A pass issued alone runs it on another stream, after the workspace is
// free, beside the main launch (which leaves it room) and the deep launch; beside other renders
// it follows the pass on its stream.
int launch_sky_tiles(const Frame &f, Pass &p, const rt::KParams &k)
{
    rt_scene *sc = f.sc;
    const uint32_t wb = p.wb;
    rt::KSky ks{};
    ks.fc = k.fc;
    ks.block_perm = k.block_perm;
    ks.pos0 = f.sky_pos0;
    ks.n_pix = k.n_pixels - f.sky_pos0;
    ks.sums = k.slots + 3u * static_cast<size_t>(f.sky_pos0);
    ks.segments = k.segments;
    p.sky_aside = f.pipe() && !p.in_flight && !(sc->opt.diag & RT_DIAG_SKY_SERIAL);
    if (!p.sky_aside) {
        RT_HIP(rt::launch_sky(ks, p.xst));
        return RT_OK;
    }
    // the next render stream, not a stream of its own: HIP maps streams to hardware
    // queues round-robin in creation order, and a ninth stream shared a queue with one
    // of the render streams, behind whose main launch the sky kernel then waited (one
    // lone frame in three at 4 queues: 0.83 vs 0.69 ms on the 8-way share). Consecutive
    // render streams sit on different queues.
    hipStream_t sky_st = sc->xs[(wb % f.pl.streams + 1u) % f.pl.streams];
    if (sc->free_valid[wb]) RT_HIP(hipStreamWaitEvent(sky_st, sc->ev_free[wb], 0));
    // (the counters it adds to are this pass's: zeroed on xst before the main launch)
    if (ks.segments) {
        if (!sc->ev_main[wb]) RT_HIP(hipEventCreateWithFlags(&sc->ev_main[wb], hipEventDisableTiming));
        if (!p.two_part) RT_HIP(hipEventRecord(sc->ev_main[wb], p.xst));
        RT_HIP(hipStreamWaitEvent(sky_st, sc->ev_main[wb], 0));
    }
    RT_HIP(rt::launch_sky(ks, sky_st));
    RT_HIP(hipEventRecord(sc->ev_sky, sky_st));
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
    a.slots = sc->slots[wb];
    a.acc = f.win_acc ? f.win_acc : sc->acc;
    a.out = f.d_rgb;
    a.out_u8 = nullptr;
    a.mom = f.win_mom ? f.win_mom : sc->mom;
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
        RT_HIP(hipStreamWaitEvent(f.st, sc->ev_main[wb], 0));
        RT_HIP(rt::launch_accumulate(a1, f.st));
        a.deep_px = k.deep.px;
        a.part = 2;
    } else if (k.deep_depth) {
        a.deep_px = k.deep.px;  // one part; clears the flags the main launch set
        a.part = 3;
    }
    if (f.pipe()) RT_HIP(hipStreamWaitEvent(f.st, sc->ev_done[wb], 0));
    if (p.sky_aside) RT_HIP(hipStreamWaitEvent(f.st, sc->ev_sky, 0));
    RT_HIP(rt::launch_accumulate(a, f.st));
    sc->ctr_dirty[wb] = false;
    if (f.pipe()) {
        RT_HIP(hipEventRecord(sc->ev_free[wb], f.st));
        sc->free_valid[wb] = true;
    }
    return RT_OK;
}

// d_var (rt_render_var_device): the frame also yields the variance of each pixel's
// mean luminance. Its samples' colours must reach the accumulation one by one, so it is planned as
// under RT_DIAG_NO_PAIRS | RT_DIAG_NO_SKY whatever the scene's options say.
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
    const rt_options &O = sc->opt;
    Frame f{sc, P, st, d_rgb, d_var, d_segments};
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
    if (c.order_ok && !pl.pairs)
        if (int rc = pass_order(sc, *camera, k, st, &f.ord); rc) return rc;
    // (max_depth 0: every sample's colour is 0, main.cxx:74, not the sky's)
    f.sky_kernel = f.ord && f.ord->d_perm && f.ord->t.n_sky && P.max_depth > 0 && !(O.diag & RT_DIAG_NO_SKY) && !moments;
    f.sky_pos0 = f.sky_kernel ? static_cast<uint32_t>(64u * static_cast<uint64_t>(f.ord->n_blocks - f.ord->t.n_sky)) : k.n_pixels;
    // the ground tiles: the order's middle class is its tiled blocks of class 1,
    // in ascending order, then the untiled blocks (class 1 too, numbered after every tile)
    f.ground = false;
    f.ground_pos0 = f.ground_pos1 = f.sky_pos0;
#ifndef RT_NO_GROUND  // A/B build switch: every pass as before the ground kernel
    // (f.sky_kernel: a culled LDS kernel dealt by tile classes, single samples, no moments, no_sky unset)
    if (f.sky_kernel && sc->ground_ok && ground_pass_ok(O, P)) {
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

    auto others_running = [&] { return f.pipe() && sc->last_ws >= 0 && hipEventQuery(sc->ev_done[sc->last_ws]) == hipErrorNotReady; };
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
        if (f.sky_kernel && s1 == P.spp)
            if (int rc = launch_sky_tiles(f, p, k); rc) return rc;
        if (c.variant == rt::V_STATS_LDS) sc->dbg_waves = p.stats_waves;
        if (s1 == s_end) RT_HIP(hipEventRecord(sc->ev_end[f.ring], p.xst));
        if (f.pipe()) {
            RT_HIP(hipEventRecord(sc->ev_done[p.wb], p.xst));
            sc->last_ws = static_cast<int>(p.wb);
        }
        if (int rc = accumulate(f, p, k); rc) return rc;
    }
    // (every launch above that reads the order's permutation is ordered before st's tail)
    return order_used(sc, f.ord, st);
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
    k.n_spheres = sc->n_spheres;
    const uint64_t n_pixels = static_cast<uint64_t>(P.width) * k.num_rows;
    if (n_pixels == 0) return RT_OK;
    if (n_pixels >= (1ull << 31)) return fail(RT_ERR_INVALID, "rt_render_device: more than 2^31 pixels in one call");
    k.n_pixels = static_cast<uint32_t>(n_pixels);
    k.n_chunks = (k.n_pixels + 63u) / 64u;
    k.shade = reinterpret_cast<const float4 *>(sc->blob[0]) + sc->shade_offset[0];
    k.out = d_rgb;
    k.ctr = sc->queue_ctr + kCompatCtr;
    k.segments = reinterpret_cast<unsigned long long *>(d_segments);
    int occ = 0;
    RT_HIP(rt::occupancy_compat(&occ));
    const uint32_t grid = static_cast<uint32_t>(
        std::max<uint64_t>(1, std::min<uint64_t>(static_cast<uint64_t>(std::max(occ, 1)) * sc->cu_count, (n_pixels + 255u) / 256u)));
    const uint32_t ring = static_cast<uint32_t>(sc->calls % rt_scene::kRing);
    ++sc->calls;
    RT_HIP(hipMemsetAsync(k.ctr, 0, sizeof(uint32_t), st));
    RT_HIP(hipEventRecord(sc->ev_begin[ring], st));
    RT_HIP(rt::launch_compat(k, grid, st));
    RT_HIP(hipEventRecord(sc->ev_end[ring], st));
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
    const bool cull = !(P.flags & RT_FLAG_BRUTE_FORCE) && sc->n_clusters[1] > 0;
    const int b = cull ? 1 : 0, cull_mode = cull ? 7 : 0;
    if (sc->static_lds_aov[b] == ~static_cast<size_t>(0)) RT_HIP(rt::static_lds_aov(cull_mode, &sc->static_lds_aov[b]));
    const size_t static_lds = sc->static_lds_aov[b];
    if (static_cast<size_t>(sc->shade_offset[b]) * 16u + static_lds > sc->max_lds)
        return fail(RT_ERR_UNSUPPORTED, "rt_render_aov_device: scene too large for LDS");
    rt::KAov a{};
    a.fc = k.fc;
    a.samples = A.samples ? A.samples : P.spp;
    a.full_frame = k.full_frame;
    a.n_blocks = (k.n_pixels + 63u) / 64u;
    a.blob = reinterpret_cast<const float4 *>(sc->blob[b]);
    a.n_geo = sc->n_geo[b];
    a.n_always = sc->n_always[b];
    a.clus_offset = sc->clus_offset[b];
    a.clus_pad = sc->clus_pad[b];
    a.n_supers = sc->n_supers[b];
    a.supers_offset = sc->supers_offset[b];
    a.use_root = (O.diag & RT_DIAG_NO_ROOT_BOX) ? 0u : 1u;
    a.transpose_max = O.transpose_max;
    a.fast_roots = sc->in_fast_range && camera_in_fast_range(*camera) && !(O.diag & RT_DIAG_IEEE_ROOTS) ? 1u : 0u;
    a.shade_offset = sc->shade_offset[b];
    a.n_spheres = sc->n_spheres;
    // the shading records join the geometry in LDS by the render kernels' rule (place_shade)
    auto occ_for = [&](int in_lds, int *out) -> int {
        int &o = sc->occ_aov[b][in_lds];
        if (o < 0) {
            RT_HIP(rt::occupancy_aov(cull_mode, &o, static_cast<size_t>(in_lds ? sc->blob_units[b] : sc->shade_offset[b]) * 16u));
            o = std::max(o, 1);
        }
        *out = o;
        return RT_OK;
    };
    const bool shade_fits = static_cast<size_t>(sc->blob_units[b]) * 16u + static_lds <= sc->max_lds;
    ShadePlace place{};
    if (int rc = place_shade(O.diag, shade_fits, false, occ_for, place); rc) return rc;
    a.shade_lds = place.in_lds;
    a.lds_units = a.shade_lds ? sc->blob_units[b] : sc->shade_offset[b];
    const int occ = place.occ;
    // the dealing order and its proven-sky blocks, under the beauty's conditions for sky_kernel
    const rt_scene::Order *ord = nullptr;
    if (sc->has_geom && cull && !(O.diag & RT_DIAG_NATURAL_ORDER))
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

int rt_scene_kernel_times(rt_scene *sc, uint32_t max, float *ms, uint32_t *n)
{
    if (!sc || !n || (max && !ms)) return fail(RT_ERR_INVALID, "rt_scene_kernel_times: null argument");
    const uint64_t avail = std::min<uint64_t>(sc->calls, rt_scene::kRing);
    const uint32_t cnt = static_cast<uint32_t>(std::min<uint64_t>(avail, max));
    RT_HIP(hipSetDevice(sc->device));
    for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t r = static_cast<uint32_t>((sc->calls - cnt + i) % rt_scene::kRing);
        RT_HIP(hipEventSynchronize(sc->ev_end[r]));
        RT_HIP(hipEventElapsedTime(ms + i, sc->ev_begin[r], sc->ev_end[r]));
    }
    *n = cnt;
    return RT_OK;
}

int rt_scene_usage_get(const rt_scene *sc, rt_scene_usage *out)
{
    if (!sc || !out) return fail(RT_ERR_INVALID, "rt_scene_usage_get: null argument");
    rt_scene_usage u{};
    uint64_t ws = sc->acc_bytes + sc->mom_bytes + sc->wq_bytes;
    for (uint32_t w = 0; w < kMaxWs; ++w) ws += sc->slots_bytes[w] + sc->deep_bytes[w];
    uint64_t fixed = kCtrWords * sizeof(uint32_t) + (sc->dbg ? rt::kDbgWords * sizeof(unsigned long long) : 0u);
    for (int b = 0; b < 2; ++b) fixed += static_cast<uint64_t>(sc->blob_units[b]) * 16u;
    fixed += static_cast<uint64_t>(std::max(sc->n_spheres, 1u)) * 16u;  // the trap windows
    fixed += static_cast<uint64_t>(sc->n_spheres) * 32u;                // the two sphere tables (rt_scene_motion)
    // the ground kernel's redo lists and counts: beside the planner's cut, so in
    // device_bytes, not in workspace_bytes
    for (uint32_t w = 0; w < kMaxWs; ++w) fixed += sc->redo_bytes[w];
    if (sc->redo_stat) fixed += rt_scene::kRing * sizeof(uint32_t);
    u.device_bytes = ws + fixed;
    u.workspace_bytes = ws;
    u.render_streams = sc->used_streams;
    u.workspaces = sc->used_ws;
    u.pass_samples = sc->used_pass;
    u.deep_launch = sc->used_deep;
    u.pair_passes = sc->used_pairs;
    u.split_passes = sc->used_split;
    u.lead_tiles = sc->used_lead;
    u.sky_tiles = sc->used_sky;
    u.static_lds_bytes = static_cast<uint32_t>(sc->static_lds[1]);
    u.max_lds_bytes = static_cast<uint32_t>(sc->max_lds);
    *out = u;
    return RT_OK;
}

int rt_scene_ground_counts(rt_scene *sc, uint64_t *ground_samples, uint64_t *redone_samples)
{
    if (!sc) return fail(RT_ERR_INVALID, "rt_scene_ground_counts: null scene");
    uint32_t redone = 0;
    if (sc->redo_stat) {
        RT_HIP(hipSetDevice(sc->device));
        RT_HIP(hipDeviceSynchronize());
        RT_HIP(hipMemcpy(&redone, sc->redo_stat + sc->ground_ring, sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (ground_samples) *ground_samples = sc->ground_samples;
    if (redone_samples) *redone_samples = redone;
    return RT_OK;
}

// New records into a live scene (include/rt_api.h): the checks, the comparison
// with the current records, the derivation on the host, then the one wait for the device, the
// upload and the swap, and at the end what was keyed by the old geometry is dropped.
int rt_scene_update(rt_scene *sc, const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials,
                    uint32_t n_materials)
{
    const char *const who = "rt_scene_update";
    if (n_spheres && !spheres) return fail(RT_ERR_INVALID, "rt_scene_update: spheres is null");
    if (!materials) return fail(RT_ERR_INVALID, "rt_scene_update: materials is null");
    if (!n_materials) return fail(RT_ERR_INVALID, "rt_scene_update: n_materials is 0");
    if (int rc = check_records(who, spheres, n_spheres, materials, n_materials); rc != RT_OK) return rc;
    if (!sc) return fail(RT_ERR_INVALID, "rt_scene_update: scene is null");
    if (n_spheres != sc->n_spheres)
        return fail(RT_ERR_INVALID, "rt_scene_update: n_spheres is " + std::to_string(n_spheres) + ", the scene has " +
                                        std::to_string(sc->n_spheres) + " (ids link the frames: the count is fixed)");
    // what changed, by the bits
    bool geometry = false, appearance = false;
    for (uint32_t i = 0; i < n_spheres; ++i) {
        const rt_material &mt = materials[spheres[i].material];
        float row[4] = {spheres[i].center[0], spheres[i].center[1], spheres[i].center[2], spheres[i].radius}, flat[5];
        std::memcpy(flat, &mt.kind, 4);
        std::memcpy(flat + 1, mt.albedo, 12);
        flat[4] = mt.param;
        geometry = geometry || std::memcmp(row, sc->cur_table.data() + 4 * static_cast<size_t>(i), 16) != 0;
        appearance = appearance || std::memcmp(flat, sc->cur_flat.data() + 5 * static_cast<size_t>(i), 20) != 0;
    }
    if (!geometry && !appearance) {
        sc->n_materials = n_materials;
        return RT_OK;
    }
    const auto t0 = std::chrono::steady_clock::now();
    SceneDerived derived;
    derive_scene(spheres, n_spheres, materials, sc->opt, derived);
    const auto t1 = std::chrono::steady_clock::now();
    int prev = 0;
    (void)hipGetDevice(&prev);
    RT_HIP(hipSetDevice(sc->device));
    // renders in flight read the blobs, the windows and the permutations: the device goes idle once
    RT_HIP(hipDeviceSynchronize());
    const auto t2 = std::chrono::steady_clock::now();
    if (int rc = install_scene(sc, derived, false); rc != RT_OK) {
        (void)hipSetDevice(prev);
        return rc;
    }
    sc->n_materials = n_materials;
    // the orders of the old geometry leave; a pool slot is free again (nothing reads it: the device is idle)
    for (auto &o : sc->orders)
        if (o.d_perm && o.slot < 0) (void)hipFree(o.d_perm);
    sc->orders.clear();
    for (auto &s : sc->perm_pool) s.read_valid = false;
    sc->deep_off.clear();
    reset_occupancy(sc);
    if (geometry) ++sc->geometry_epoch;
    if (appearance) ++sc->appearance_epoch;
    (void)hipSetDevice(prev);
    if (sc->opt.diag & RT_DIAG_VERBOSE) {
        const auto t3 = std::chrono::steady_clock::now();
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        std::fprintf(stderr, "rt_scene_update: derive %.3f ms, device wait %.3f ms, upload and swap %.3f ms\n", ms(t0, t1),
                     ms(t1, t2), ms(t2, t3));
    }
    return RT_OK;
}

int rt_scene_motion(rt_scene *sc, rt_scene_motion_t *out)
{
    if (!sc || !out) return fail(RT_ERR_INVALID, "rt_scene_motion: null argument");
    *out = rt_scene_motion_t{static_cast<uint32_t>(sizeof(rt_scene_motion_t)), sc->n_spheres, sc->centres[0], sc->centres[1],
                             sc->geometry_epoch, sc->appearance_epoch};
    return RT_OK;
}

int rt_scene_order_counts(rt_scene *sc, uint64_t *host_orders, uint64_t *device_orders, uint64_t *hits)
{
    if (!sc) return fail(RT_ERR_INVALID, "rt_scene_order_counts: null scene");
    if (host_orders) *host_orders = sc->host_orders;
    if (device_orders) *device_orders = sc->device_orders;
    if (hits) *hits = sc->order_hits;
    return RT_OK;
}

// The device twin of rt_tile_order: the two kernels on the caller's stream over
// this scene's geometry, the permutation into the caller's device buffer, the counts read back
// once the stream is idle.
int rt_tile_order_device(rt_scene *sc, const rt_camera *camera, const rt_params *params, uint32_t *d_perm, uint32_t cap,
                         uint32_t *n_blocks, uint32_t *n_lead, uint32_t *n_sky, void *stream)
{
    if (!sc || !camera || !params || !n_blocks || !n_lead || !n_sky || (cap && !d_perm))
        return fail(RT_ERR_INVALID, "rt_tile_order_device: null argument");
    if (camera->mode > RT_CAMERA_CORRECTED) return fail(RT_ERR_INVALID, "rt_tile_order_device: bad camera mode");
    const uint32_t rstride = params->row_stride ? params->row_stride : 1u;
    const uint32_t rows = params->num_rows ? params->num_rows
                          : params->row_offset >= params->height ? 0u
                                                                 : (params->height - params->row_offset + rstride - 1u) / rstride;
    if (static_cast<uint64_t>(params->width) * rows >= (1ull << 32))
        return fail(RT_ERR_INVALID, "rt_tile_order_device: more than 2^32 pixels in one pass");
    rttile::KTiles kt{};
    pass_tiles(params->width, params->height, params->row_offset, rstride, rows, 3u, kt);
    *n_blocks = kt.n_blocks;
    *n_lead = *n_sky = 0;
    if (!kt.n_blocks) return RT_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    RT_HIP(hipSetDevice(sc->device));
    if (int rc = tiles_ready(sc, kt.n_blocks); rc) return rc;
    const bool fits = cap >= kt.n_blocks;
    if (int rc = enqueue_device_order(sc, *camera, kt, fits ? d_perm : nullptr, st); rc) return rc;
    RT_HIP(hipStreamSynchronize(st));
    *n_lead = sc->h_counts[0];
    *n_sky = sc->h_counts[1];
    if (cap && !fits) return fail(RT_ERR_CAPACITY, "rt_tile_order_device: perm buffer too small");
    return RT_OK;
}

int rt_scene_debug_counters(rt_scene *sc, uint64_t out[16], int reset)
{
    if (!sc || !out) return fail(RT_ERR_INVALID, "rt_scene_debug_counters: null argument");
    RT_HIP(hipSetDevice(sc->device));
    if (!sc->dbg) {
        std::memset(out, 0, 16 * sizeof(uint64_t));
        return RT_OK;
    }
    RT_HIP(hipDeviceSynchronize());
    RT_HIP(hipMemcpy(out, sc->dbg, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) RT_HIP(hipMemset(sc->dbg, 0, 16 * sizeof(uint64_t)));
    // the instrumented kernel's bounds check (rt_device.h kDbgError): an index past its bound
    if (const uint64_t e = out[rt::kDbgError]; e) {
        static const char *const kWhat[] = {"?", "walk-shortcut neighbour slot", "shading record", "sample slot",
                                            "deep-queue append", "deep-queue item", "deep-path hint sphere", "cluster members",
                                            "deep pixel flag"};
        const uint32_t code = static_cast<uint32_t>(e >> 32);
        return fail(RT_ERR_DEVICE, std::string("rt_scene_debug_counters: bounds check: ") +
                                       kWhat[code < sizeof(kWhat) / sizeof(kWhat[0]) ? code : 0] + " index " +
                                       std::to_string(static_cast<uint32_t>(e)) + " past its bound (code " +
                                       std::to_string(code) + ")");
    }
    return RT_OK;
}

int rt_scene_debug_events(rt_scene *sc, uint64_t out[32], int reset)
{
    if (!sc || !out) return fail(RT_ERR_INVALID, "rt_scene_debug_events: null argument");
    RT_HIP(hipSetDevice(sc->device));
    std::memset(out, 0, 32 * sizeof(uint64_t));
    if (!sc->dbg) return RT_OK;
    RT_HIP(hipDeviceSynchronize());
    RT_HIP(hipMemcpy(out, sc->dbg + rt::kDbgEvBase, rt::kDbgEvents * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) RT_HIP(hipMemset(sc->dbg + rt::kDbgEvBase, 0, rt::kDbgEvents * sizeof(uint64_t)));
    return RT_OK;
}

int rt_scene_debug_timeline(rt_scene *sc, uint64_t *out, uint32_t max_waves, uint32_t *n)
{
    if (!sc || !out || !n) return fail(RT_ERR_INVALID, "rt_scene_debug_timeline: null argument");
    RT_HIP(hipSetDevice(sc->device));
    *n = 0;
    if (!sc->dbg) return RT_OK;
    const uint32_t waves = std::min({max_waves, sc->dbg_waves, rt::kDbgWaves});
    RT_HIP(hipDeviceSynchronize());
    RT_HIP(hipMemcpy(out, sc->dbg + 16, 4 * static_cast<size_t>(waves) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    *n = waves;
    return RT_OK;
}

int rt_epilogue_rgb8_device(const float *d_rgb, uint8_t *d_out, uint64_t n_pixels, void *stream)
{
    if (!d_rgb || !d_out) return fail(RT_ERR_INVALID, "rt_epilogue_rgb8_device: null argument");
    if (!n_pixels) return RT_OK;
    RT_HIP(rt::launch_epilogue(d_rgb, d_out, n_pixels * 3u, static_cast<hipStream_t>(stream)));
    return RT_OK;
}

} // extern "C"

// the preview session (rt_host_post.cpp) allocates its planes where its scene lives
int rthost::scene_device(const rt_scene *sc) { return sc->device; }

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
    void *arena = nullptr;
    size_t arena_bytes = 0;
    uint64_t *d_seg = nullptr;  // the work counters of a render with stats (24 bytes)
    hipEvent_t e0 = nullptr, e1 = nullptr;
};
std::mutex g_sync_mu;  // one synchronous call at a time per process (the reference's entry is not re-entrant)
std::map<int, SyncContext> g_sync;

void sync_release(int dev, SyncContext &c)
{
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(dev);
    if (c.sc) rt_scene_destroy(c.sc);
    for (void *p : {c.arena, (void *)c.d_seg})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : {c.e0, c.e1})
        if (e) (void)hipEventDestroy(e);
    c = SyncContext{};
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
    if (cx.arena_bytes < total || !cx.arena) {
        if (cx.arena) chk(hipFree(cx.arena), "hipFree");
        cx.arena = nullptr;
        cx.arena_bytes = 0;
        if (chk(hipMalloc(&cx.arena, std::max<size_t>(total, 256)), "hipMalloc")) cx.arena_bytes = total;
    }
    if (rc == RT_OK && s.counters && !cx.d_seg) chk(hipMalloc((void **)&cx.d_seg, 24), "hipMalloc");
    if (rc == RT_OK && !cx.e0) chk(hipEventCreate(&cx.e0), "hipEventCreate");
    if (rc == RT_OK && !cx.e1) chk(hipEventCreate(&cx.e1), "hipEventCreate");
    if (rc == RT_OK && !s.skip) {
        Plane *const end = s.planes + s.n_planes;
        for (Plane *pl = s.planes; pl != end; ++pl) {
            if (pl->kind == Plane::Absent) continue;
            pl->dev = static_cast<char *>(cx.arena) + pl->at;
            if (rc == RT_OK && pl->kind == Plane::In)
                chk(hipMemcpy(pl->dev, pl->host, pl->pixels(s.n_px) * pl->px_bytes, hipMemcpyHostToDevice), "hipMemcpy");
            if (rc == RT_OK && pl->clear) chk(hipMemsetAsync(pl->dev, 0, pl->pixels(s.n_px) * pl->px_bytes, nullptr), "hipMemset");
        }
        // the work counters (rt_stats) come from the counting instantiation of the kernels, slower than
        // the product's: only when the caller asks for them (rt::render_impl does not, as cuda_impl)
        if (rc == RT_OK && s.counters) {
            chk(hipMemsetAsync(cx.d_seg, 0, 24, nullptr), "hipMemset");
            d_counters = cx.d_seg;
        }
        if (rc == RT_OK) chk(hipEventRecord(cx.e0, nullptr), "hipEventRecord");
        if (rc == RT_OK) rc = enqueue();
        if (rc == RT_OK) chk(hipEventRecord(cx.e1, nullptr), "hipEventRecord");
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
        if (rc == RT_OK && s.counters) chk(hipMemcpy(counters, cx.d_seg, 24, hipMemcpyDeviceToHost), "hipMemcpy");
        if (rc == RT_OK) chk(hipDeviceSynchronize(), s.who);
        if (rc == RT_OK) chk(hipEventElapsedTime(&kernel_ms, cx.e0, cx.e1), "hipEventElapsedTime");
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
