// rt_scene.h — the scene record (struct rt_scene) and the few functions that cross the files built
// around it: rt_host_scene.cpp (its lifecycle, updates and reports), rt_host_order.cpp (the cache
// of dealing orders), rt_host.cpp (the render path) and rt_host_synccall.cpp (the synchronous calls'
// cached context). Private to those four: rt_host_post.cpp and rt_host_multi.cpp reach a scene
// through rt_host_sync.h and the C-ABI only.
//
// Every device buffer, pinned buffer, stream and event here is an owner (rt_hip_own.h): deleting
// the scene frees it. rt_scene_destroy makes the scene's device current and synchronises the
// scene's own streams first, so no buffer goes while work of the scene's may still read it; after
// that the order in which the members go does not matter.
#pragma once
#include <algorithm>
#include <cstdint>
#include <iterator>
#include <utility>
#include <vector>

#include "rt_hip_own.h"
#include "rt_host_build.h"
#include "rt_host_sync.h"

namespace rthost {

// counters: [kMaxWs][8 queues x kQueueStride], then [kMaxWs][4] u64 segment counters, then
// the compat kernel's counter
constexpr size_t kSegWords = kMaxWs * 8 * rt::kQueueStride;
constexpr size_t kCompatCtr = kSegWords + kMaxWs * 8 + 16;
constexpr size_t kCtrWords = kCompatCtr + rt::kQueueStride;

// The scene on the device and the host records it was derived from.
struct DeviceScene {
    uint32_t n_spheres = 0, n_materials = 0;
    // scene blobs: [0] every sphere in index order (brute force), [1] big
    // spheres always tested + spatial clusters; each with its metadata record
    DevBuf<float> blob[2];
    blob_meta meta[2];
    // trap windows (rt_host_build.cpp trap_windows): {cos_lo, cos_hi} per sphere, then as many
    // empty windows (for renders deeper than rt::kTrapDepth); all empty under RT_DIAG_NO_TRAP_END
    DevBuf<float> trap;
    bool in_fast_range = false;  // every sphere within 2^19 of the origin, radii >= 2^-40 (short exact forms)
    // The ground kernel: the culled scene has a root box and 1 to 8
    // always-tested spheres, all lambert.
    bool ground_ok = false;
    // the scene's geometry for the tile classes of a pass, on the host and as
    // classify_tiles_kernel reads it (KTiles::geom); has_geom: the scene has
    // clusters, so its passes are dealt by tile classes
    scene_geom geom;
    bool has_geom = false;
    DevBuf<float> geom_words;
    // Moving spheres (rt_scene_update). blob[], trap and geom_words keep the bytes
    // allocated behind them (DevBuf::bytes): an update whose clustering needs more grows them, one
    // that needs less keeps them. The records the scene was last derived from, as an update compares
    // them: {cx, cy, cz, r} per sphere and its flattened {kind, albedo, param}. The two device tables
    // rt_scene_motion reports, [0] the current records and [1] those before the most recent update,
    // and the two epochs.
    std::vector<float> cur_table, cur_flat;
    DevBuf<float> centres[2];
    uint64_t geometry_epoch = 0, appearance_epoch = 0;
};

// The traversal fields of a kernel record (rt::KParams, rt::KAov: the same names) from a blob.
template <class K>
void fill_traversal(K &k, const DeviceScene &d, int b)
{
    const blob_meta &m = d.meta[b];
    k.blob = reinterpret_cast<const float4 *>(d.blob[b].get());
    k.n_geo = m.n_geo;
    k.n_always = m.n_always;
    k.clus_offset = m.clus_offset;
    k.clus_pad = m.clus_pad;
    k.n_supers = m.n_supers;
    k.supers_offset = m.supers_offset;
    k.shade_offset = m.shade_offset;
    k.n_spheres = d.n_spheres;
}

// workspaces: consecutive render passes (of one frame or of consecutive frames) rotate over
// internal streams xs[b] and workspaces slots[b], so a pass renders while the caller stream
// still accumulates the previous ones
struct Workspaces {
    DevBuf<float> slots[kMaxWs];
    DevBuf<float> acc;
    // rt_render_var_device: {L_0, m1, m2} per pixel between the passes of a frame, beside acc
    // (allocated by the first multi-pass variance render)
    DevBuf<float> mom;
    // deep-path split: per workspace, the pixel flags (a byte per pixel, at the front) and then
    // the deep queue (rt::DeepQueue); deep_clean = leading bytes known to be zero (every pass's
    // accumulation clears the flags it set, so only a larger pixel count needs a memset)
    DevBuf<char> deep[kMaxWs];
    size_t deep_clean[kMaxWs] = {};
    // where the pair-arrival words of the queue of workspace w lay in its last layout (the
    // arrays' offsets follow the pixel count and the region capacity): zeroed again when moved
    size_t deep_meet_at[kMaxWs] = {};
    // the ground kernel's redo list of a pass (4 B per ground sample; beside the planner's cut,
    // like the orders' buffers)
    DevBuf<uint32_t> redo[kMaxWs];
    DevBuf<char> wq;  // RT_FLAG_WAVEFRONT: two ray queues and their counters
    // frees every workspace (slots, deep queues, redo lists, multi-pass sums, wavefront queues)
    // after the device is idle: the next render re-cuts them under max_workspace_bytes
    int release_all();
};

// The caches keyed by a blob's size, blocks per CU, -1 = unknown (as a fresh scene has them).
struct Occupancy {
    int render[4][2][2];  // [variant][culled][shade records in LDS]
    int pairs[4][2];      // the culled kernel's sample-pair instantiation, [variant][shade records in LDS]
    // [variant] the 8-wave deep kernel with the whole blob in LDS; 0 = it does not fit or holds no
    // more waves than 4-wave groups (the lone deep launch)
    int deep_wide[4];
    int aov[2][2];        // aov_kernel (rt_render_aov_device) [culled][shade records in LDS]
    int wave[2];          // wave_bounce_kernel [culled]
    Occupancy() { reset(); }
    void reset()
    {
        for (auto &r : render) for (auto &x : r) x[0] = x[1] = -1;
        for (auto &r : pairs) r[0] = r[1] = -1;
        for (int &x : deep_wide) x = -1;
        for (auto &r : aov) r[0] = r[1] = -1;
        wave[0] = wave[1] = -1;
    }
};

// The dealing orders computed from the scene's geometry, per camera and rows (a pure function of
// those and the scene, kept for the kOrders most recently used), each with its block permutation
// on the device.
struct Order {
    std::vector<unsigned char> key;
    tile_order t;           // (an order computed on the device: the counts alone, perm stays empty)
    uint32_t n_blocks = 0;  // blocks of the permutation (0: the pass keeps its natural order)
    const uint32_t *d_perm = nullptr;  // what the kernels read: own's buffer, or (borrowed) the pool slot's
    DevBuf<uint32_t> own;   // an order computed on the host: its own permutation
    int slot = -1;          // >= 0: the slot of perm_pool that d_perm is borrowed from
    uint64_t used = 0;
};
constexpr size_t kOrders = 8;
// Dealing orders computed on the device (rt_options.tile_classes = 1, rt_tile_order_device;
// DESIGN.md §4.13), made by the first such order: a stream of the scene's own for the two kernels
// (the caller's and the render streams hold the frames in flight) with the event the host waits
// on, the class bytes, the counts on the device and in pinned host memory. A cached order's
// permutation sits in a slot of perm_pool; a slot carries an event recorded after the last
// call that read it, which the classification stream waits on before the slot is written again.
struct PermSlot {
    DevBuf<uint32_t> d;  // (its bytes: the blocks it holds)
    Event ev_read;
    bool read_valid = false;
};
struct DealingOrders {
    std::vector<Order> cache;
    uint64_t tick = 0;  // the orders' LRU clock
    uint64_t host_orders = 0, device_orders = 0, hits = 0;  // rt_scene_order_counts
    Stream tile_st;
    Event ev_tiles;
    DevBuf<uint8_t> d_cls;  // (its bytes: the blocks it holds class bytes for)
    DevBuf<uint32_t> d_counts;
    PinnedBuf<uint32_t> h_counts;
    PermSlot perm_pool[kOrders];
    // every order of the old geometry leaves; the pool's slots are free again (the device is idle)
    void clear()
    {
        cache.clear();
        for (PermSlot &s : perm_pool) s.read_valid = false;
    }
};

// the last render's cut (rt_scene_usage_get)
struct Usage {
    uint32_t streams = 0, ws = 0, pass = 0, deep = 0, pairs = 0, split = 0;
    uint32_t lead = 0, sky = 0;  // the last pass's tile classes
};

} // namespace rthost

struct rt_scene {
    int device = 0;
    rt_options opt{};  // fixed at creation (rt_scene_create_ex)
    rthost::DeviceScene dev;
    rthost::Workspaces ws;
    rthost::Occupancy occ;
    rthost::DealingOrders ord;
    rthost::Usage used;
    // deep-queue overflow reports (pinned host memory written by accumulate_kernel, one word per
    // workspace, with its device alias) and the camera keys they named, with the call that last
    // reported each: renders with such a camera are not split for kDeepOffCalls calls; at most
    // kDeepOffKeys keys (LRU)
    rthost::PinnedBuf<unsigned long long> deep_over;
    unsigned long long *deep_over_dev = nullptr;
    static constexpr size_t kDeepOffKeys = 8;
    static constexpr uint64_t kDeepOffCalls = 256;
    std::vector<std::pair<unsigned long long, uint64_t>> deep_off;
    rthost::DevBuf<uint32_t> queue_ctr;  // kCtrWords: queue and segment counters (layout at kCtrWords)
    rthost::Stream xs[rthost::kMaxBufs];
    rthost::Event ev_done[rthost::kMaxWs], ev_free[rthost::kMaxWs];
    rthost::Event ev_main[rthost::kMaxWs];  // split passes: after the main launch (created on first use)
    // the sky kernel of a pass issued alone runs beside the pass's main and deep launches, on the
    // next render stream (idle: nothing else runs); ev_sky after it
    rthost::Event ev_sky;
    // a window whose sky_moments_kernel runs on a render stream: recorded on the
    // caller's stream when the call begins; that kernel, which reads and writes the session's planes, waits
    rthost::Event ev_enter;
    bool free_valid[rthost::kMaxWs] = {};
    // queue/segment counters of workspace b not known to be zero (set while a render using
    // them is enqueued, cleared once the accumulation that resets them is enqueued after it)
    bool ctr_dirty[rthost::kMaxWs];
    rt_scene() { std::fill(std::begin(ctr_dirty), std::end(ctr_dirty), true); }
    uint32_t next_buf = 0;  // workspace of the next render pass
    int last_ws = -1;       // workspace of the last render pass issued (its ev_done), -1 = none
    // the caller stream of the previous call and an event after the last work enqueued on it:
    // a call on another stream first waits for it, so the shared accumulation buffer, the
    // compat counter and (render_streams = 1) the workspaces are never used by two streams at once
    hipStream_t last_stream = nullptr;
    rthost::Event ev_tail;
    bool tail_valid = false;
    int cu_count = 0;
    rthost::DevBuf<unsigned long long> dbg;  // diagnostic counters (RT_DIAG_STATS)
    uint32_t dbg_waves = 0;                  // waves of the last instrumented launch
    size_t max_lds = 0;
    // static LDS of the render kernel per traversal, [0] brute force, [1] culled (per-wave
    // transposed-test records and per-lane arrays; hipFuncGetAttributes)
    size_t static_lds[2] = {0, 0};
    size_t static_lds_pairs = 0;  // the culled kernel's sample-pair instantiation (its parked colours)
    // aov_kernel (rt_render_aov_device), on first use: static LDS per traversal (~0 = unknown)
    size_t static_lds_aov[2] = {~static_cast<size_t>(0), ~static_cast<size_t>(0)};
    // The ground kernel. redo_stat: the samples redone per call, by the call's
    // ring slot; ground_samples / ground_ring: the last frame's ground samples and its slot
    // (rt_scene_ground_counts). ev_gpre / ev_ground: before and after the ground kernel of a pass
    // issued alone, which runs on another stream.
    rthost::DevBuf<uint32_t> redo_stat;
    uint64_t ground_samples = 0;
    uint32_t ground_ring = 0;
    uint64_t ground_call = 0;  // calls of the frame ground_samples and ground_ring belong to
    rthost::Event ev_gpre, ev_ground;
    // after an adaptive session's copy of the frame's dealing order, enqueued on the caller's stream
    // at the session's first window: the render streams, whose passes read it, wait
    rthost::Event ev_blocks;
    // ring of (start, end) events bracketing the render kernels of each rt_render_device call
    static constexpr uint32_t kRing = 256;
    std::vector<rthost::Event> ev_begin, ev_end;
    uint64_t calls = 0;
};

namespace rthost {

// ---- rt_host_order.cpp ---------------------------------------------------------------------
// The classification's stream, event, class bytes and counts, made on first use and grown to
// n_blocks class bytes.
int tiles_ready(rt_scene *sc, uint32_t n_blocks);
// The blocks of a pass as classify_tiles counts them (rt_host_build.cpp): n_blocks = 0 when the
// pass keeps its natural order, n_tiles = 0 when its width is not a multiple of the tile's.
void pass_tiles(uint32_t W, uint32_t H, uint32_t row_offset, uint32_t row_stride, uint32_t num_rows, uint32_t tile_lw,
                rttile::KTiles &k);
// Enqueues the two kernels and the copy of the counts to the pinned counts on `st`: the class bytes
// of the pass k describes, then d_perm (null: none) and the counts.
int enqueue_device_order(rt_scene *sc, const rt_camera &cam, rttile::KTiles &k, uint32_t *d_perm, hipStream_t st);
// The dealing order of a pass over these rows with this camera, cached; `st`: the stream of the
// call, on which order_used is recorded once the call's last reader is enqueued.
int pass_order(rt_scene *sc, const rt_camera &cam, const rt::KParams &k, hipStream_t st, const Order **out);
int order_used(rt_scene *sc, const Order *ord, hipStream_t st);

// ---- rt_host.cpp ---------------------------------------------------------------------------
// The arguments of the feature-buffer calls, decided before any HIP call.
int check_aov(const rt_params *p, const rt_aov_buffers *a, const char *who);

} // namespace rthost
