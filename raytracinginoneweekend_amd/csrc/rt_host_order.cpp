// rt_host_order.cpp — a scene's cache of dealing orders (rt_scene.h DealingOrders; DESIGN.md §4.7,
// §4.13): the order of a pass by camera and rows, computed on the host or by the two kernels of
// rt_tiles.hip on the scene's own stream, the pool of permutations the device orders live in, and
// the two entry points that report on them (rt_tile_order_device, rt_scene_order_counts).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rt_api.h"
#include "rt_device.h"
#include "rt_host_build.h"
#include "rt_host_sync.h"
#include "rt_scene.h"

using namespace rthost;

namespace {
// ---- dealing orders computed on the device --------------------------------
// order_blocks_kernel is one workgroup that walks the blocks 1024 at a time: passes above this
// many blocks (a 8192 x 8192 frame) have their order computed on the host under tile_classes = 1
constexpr uint32_t kDeviceOrderMaxBlocks = 1u << 20;
} // namespace

// The classification's stream, event, class bytes and counts, made on first use and grown to
// n_blocks class bytes (nothing of an earlier classification is in flight then: every one ends
// with the host waiting for it).
int rthost::tiles_ready(rt_scene *sc, uint32_t n_blocks)
{
    DealingOrders &o = sc->ord;
    // (a stream of the default priority: one of the highest priority, and the kernels' waves at a
    // raised issue priority, were measured and did not help)
    RT_HIP(o.tile_st.make(hipStreamNonBlocking));
    RT_HIP(o.ev_tiles.make(hipEventDisableTiming));
    if (!o.d_counts) RT_HIP(o.d_counts.alloc(2 * sizeof(uint32_t)));
    if (!o.h_counts) RT_HIP(o.h_counts.alloc(2 * sizeof(uint32_t), hipHostMallocDefault));
    if (o.d_cls.bytes() < n_blocks) RT_HIP(o.d_cls.alloc((n_blocks + 4095u) & ~4095u));
    return RT_OK;
}

// The blocks of a pass as classify_tiles counts them (rt_host_build.cpp): n_blocks = 0 when the
// pass keeps its natural order, n_tiles = 0 when its width is not a multiple of the tile's.
void rthost::pass_tiles(uint32_t W, uint32_t H, uint32_t row_offset, uint32_t row_stride, uint32_t num_rows, uint32_t tile_lw,
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

// Enqueues the two kernels and the copy of the counts to the pinned counts on `st`: the class bytes of
// the pass k describes, then d_perm (null: none) and the counts.
int rthost::enqueue_device_order(rt_scene *sc, const rt_camera &cam, rttile::KTiles &k, uint32_t *d_perm, hipStream_t st)
{
    const scene_geom &g = sc->dev.geom;
    DealingOrders &o = sc->ord;
    k.cam = cam;
    k.geom = sc->dev.geom_words.get();
    k.has_root = g.has_root ? 1u : 0u;
    k.n_boxes = static_cast<uint32_t>(g.boxes.size() / 6u);
    k.n_always = static_cast<uint32_t>(g.always.size());
    k.clus_pad = g.clus_pad;
    k.cls = o.d_cls.get();
    RT_HIP(rt::launch_classify_tiles(k, st));
    RT_HIP(rt::launch_order_blocks(o.d_cls.get(), k.n_blocks, d_perm, o.d_counts.get(), st));
    RT_HIP(hipMemcpyAsync(o.h_counts.get(), o.d_counts.get(), 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return RT_OK;
}

namespace {
// The least recently used order leaves when kOrders are cached. One with a permutation of its own
// (computed on the host) is freed once the device is idle: renders in flight may still read it.
// One in a pool slot just leaves: the slot's event guards its next use.
int evict_order(rt_scene *sc)
{
    std::vector<Order> &cache = sc->ord.cache;
    if (cache.size() < kOrders) return RT_OK;
    auto lru = std::min_element(cache.begin(), cache.end(), [](const Order &a, const Order &b) { return a.used < b.used; });
    if (lru->own) {
        RT_HIP(hipDeviceSynchronize());
        RT_HIP(lru->own.release());
    }
    cache.erase(lru);
    return RT_OK;
}

// A miss under tile_classes = 1: the order of the pass in a free slot of the pool, by the two
// kernels on the scene's own stream. The host waits for that stream's event alone (it needs the
// counts to size the launches), and the caller's stream waits for it too.
int device_order(rt_scene *sc, const rt_camera &cam, rttile::KTiles &kt, hipStream_t st, Order &e)
{
    if (int rc = evict_order(sc); rc) return rc;
    DealingOrders &O = sc->ord;
    auto taken = [&](int i) { return std::any_of(O.cache.begin(), O.cache.end(), [i](const Order &o) { return o.slot == i; }); };
    int slot = -1;
    for (int i = 0; i < static_cast<int>(kOrders) && slot < 0; ++i)
        if (!taken(i)) slot = i;
    if (slot < 0) return fail(RT_ERR_DEVICE, "pass_order: no free permutation slot");
    if (int rc = tiles_ready(sc, kt.n_blocks); rc) return rc;
    const size_t perm_bytes = static_cast<size_t>(kt.n_blocks) * sizeof(uint32_t);
    if (O.perm_pool[slot].d.bytes() < perm_bytes) {
        // a larger pass than the pool was cut for: every slot no cached order holds grows to it
        // (the first order of a scene allocates them all), after the last call that read it
        for (int i = 0; i < static_cast<int>(kOrders); ++i) {
            PermSlot &p = O.perm_pool[i];
            if (taken(i) || p.d.bytes() >= perm_bytes) continue;
            RT_HIP(p.ev_read.make(hipEventDisableTiming));
            if (p.read_valid) RT_HIP(hipEventSynchronize(p.ev_read.get()));
            p.read_valid = false;
            RT_HIP(p.d.alloc(perm_bytes));
        }
    }
    PermSlot &p = O.perm_pool[slot];
    if (p.read_valid) RT_HIP(hipStreamWaitEvent(O.tile_st.get(), p.ev_read.get(), 0));
    if (int rc = enqueue_device_order(sc, cam, kt, p.d.get(), O.tile_st.get()); rc) return rc;
    RT_HIP(hipEventRecord(O.ev_tiles.get(), O.tile_st.get()));
    RT_HIP(hipEventSynchronize(O.ev_tiles.get()));
    RT_HIP(hipStreamWaitEvent(st, O.ev_tiles.get(), 0));
    e.t.n_lead = O.h_counts.get()[0];
    e.t.n_sky = O.h_counts.get()[1];
    if (static_cast<uint64_t>(e.t.n_lead) + e.t.n_sky > kt.n_blocks) return fail(RT_ERR_DEVICE, "pass_order: bad class counts from the device");
    e.n_blocks = kt.n_blocks;
    e.d_perm = p.d.get();
    e.slot = slot;
    return RT_OK;
}
} // namespace

// The dealing order of a pass over these rows with this camera (DealingOrders::cache; computed on a
// miss: classify_tiles on the host, the permutation uploaded once; or, under tile_classes = 1
// for a pass whose tiles are classified at all, on the device: device_order). `st`: the stream
// of the call, on which order_used is recorded once the call's last reader is enqueued.
int rthost::pass_order(rt_scene *sc, const rt_camera &cam, const rt::KParams &k, hipStream_t st, const Order **out)
{
    *out = nullptr;
    DealingOrders &O = sc->ord;
    std::vector<unsigned char> key(sizeof(rt_camera) + 7 * sizeof(uint32_t));
    const uint32_t g[7] = {k.W, k.H, k.row_offset, k.row_stride, k.num_rows, k.tile_lw, 0u};
    std::memcpy(key.data(), &cam, sizeof(rt_camera));
    std::memcpy(key.data() + sizeof(rt_camera), g, sizeof(g));
    for (auto &o : O.cache)
        if (o.key == key) {
            o.used = ++O.tick;
            ++O.hits;
            *out = &o;
            return RT_OK;
        }
    Order e;
    e.key.swap(key);
    if (sc->opt.tile_classes == 1u) {
        rttile::KTiles kt{};
        pass_tiles(k.W, k.H, k.row_offset, k.row_stride, k.num_rows, k.tile_lw, kt);
        if (kt.n_tiles && kt.n_blocks <= kDeviceOrderMaxBlocks) {
            if (int rc = device_order(sc, cam, kt, st, e); rc) return rc;
            ++O.device_orders;
            e.used = ++O.tick;
            O.cache.push_back(std::move(e));
            *out = &O.cache.back();
            return RT_OK;
        }
    }
    e.t = classify_tiles(cam, k.W, k.H, k.row_offset, k.row_stride, k.num_rows, k.tile_lw, sc->dev.geom);
#ifdef RT_ORDER_IDENTITY  // A/B build switch: the class machinery over the natural order (one middle group)
    for (uint32_t i = 0; i < e.t.perm.size(); ++i) e.t.perm[i] = i;
    e.t.n_lead = e.t.n_sky = 0;
#endif
    e.n_blocks = static_cast<uint32_t>(e.t.perm.size());
    ++O.host_orders;
    if (!e.t.perm.empty()) {
        RT_HIP(e.own.alloc(e.t.perm.size() * sizeof(uint32_t)));
        e.d_perm = e.own.get();
        const hipError_t ce = hipMemcpy(e.own.get(), e.t.perm.data(), e.t.perm.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (ce != hipSuccess) return fail(RT_ERR_DEVICE, std::string("hipMemcpy: ") + hipGetErrorString(ce));
    }
    if (int rc = evict_order(sc); rc) return rc;
    e.used = ++O.tick;
    O.cache.push_back(std::move(e));
    *out = &O.cache.back();
    return RT_OK;
}

// After the last work of a call that reads the order's permutation is enqueued on (or ordered
// before the tail of) `st`: a permutation in a pool slot is not written again before that work.
int rthost::order_used(rt_scene *sc, const Order *ord, hipStream_t st)
{
    if (!ord || ord->slot < 0) return RT_OK;
    PermSlot &p = sc->ord.perm_pool[ord->slot];
    RT_HIP(hipEventRecord(p.ev_read.get(), st));
    p.read_valid = true;
    return RT_OK;
}

extern "C" {

int rt_scene_order_counts(rt_scene *sc, uint64_t *host_orders, uint64_t *device_orders, uint64_t *hits)
{
    if (!sc) return fail(RT_ERR_INVALID, "rt_scene_order_counts: null scene");
    if (host_orders) *host_orders = sc->ord.host_orders;
    if (device_orders) *device_orders = sc->ord.device_orders;
    if (hits) *hits = sc->ord.hits;
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
    const uint32_t rstride = params->row_stride ? params->row_stride : 1u, rows = rows_of(*params);
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
    *n_lead = sc->ord.h_counts.get()[0];
    *n_sky = sc->ord.h_counts.get()[1];
    if (cap && !fits) return fail(RT_ERR_CAPACITY, "rt_tile_order_device: perm buffer too small");
    return RT_OK;
}

} // extern "C"
