// rt_host_scene.cpp — a scene's lifecycle on the device (include/rt_api.h): creation from the
// records (rt_host_build.cpp derive_scene puts them into blobs on the host, install_scene puts
// those on the device), rt_scene_update, destruction, and what a scene reports about itself
// (usage, motion tables, kernel times, ground counts, the diagnostic counters). The record is
// rt_scene.h's; the renders that use it are rt_host.cpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rt_api.h"
#include "rt_device.h"
#include "rt_host_build.h"
#include "rt_host_sync.h"
#include "rt_scene.h"

using namespace rthost;

int rthost::Workspaces::release_all()
{
    RT_HIP(hipDeviceSynchronize());
    for (uint32_t w = 0; w < kMaxWs; ++w) {
        RT_HIP(slots[w].release());
        RT_HIP(deep[w].release());
        RT_HIP(redo[w].release());
        deep_clean[w] = 0;
        deep_meet_at[w] = 0;
    }
    RT_HIP(acc.release());
    RT_HIP(mom.release());
    RT_HIP(wq.release());
    return RT_OK;
}

namespace {

// Puts a derivation on the device and into the scene's fields. Every buffer that is too small (all
// of them at creation) is allocated first, as a local, then everything is uploaded, then the fresh
// buffers are moved in and the counts follow: an allocation or upload that fails leaves the scene
// as it was (the locals free themselves). The device is idle (an update has waited for it; at
// creation nothing runs yet). `first`: the creation, which also makes the two sphere tables, both
// with the records; an update swaps them and writes the current one.
int install_scene(rt_scene *sc, SceneDerived &d, bool first)
{
    DeviceScene &D = sc->dev;
    DevBuf<float> *const own[4] = {&D.blob[0], &D.blob[1], &D.trap, &D.geom_words};
    const std::vector<float> *const src[4] = {&d.blobs[0].data, &d.blobs[1].data, &d.trap, &d.geom_words};
    DevBuf<float> fresh[4], tables[2];
    const size_t table_bytes = d.table.size() * sizeof(float);
    hipError_t e = hipSuccess;
    for (int i = 0; i < 4; ++i) {
        const size_t bytes = src[i]->size() * sizeof(float);
        if (e == hipSuccess && (!*own[i] || own[i]->bytes() < bytes)) e = fresh[i].alloc(std::max<size_t>(bytes, 256));
    }
    for (int t = 0; first && t < 2 && e == hipSuccess; ++t) e = tables[t].alloc(std::max<size_t>(table_bytes, 256));
    for (int i = 0; i < 4; ++i)
        if (e == hipSuccess && !src[i]->empty())
            e = hipMemcpy((fresh[i] ? fresh[i] : *own[i]).get(), src[i]->data(), src[i]->size() * sizeof(float), hipMemcpyHostToDevice);
    // (the table an update writes is the older one: it becomes the current one below)
    float *const write_table = first ? tables[0].get() : D.centres[1].get();
    if (e == hipSuccess && table_bytes) e = hipMemcpy(write_table, d.table.data(), table_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && first && table_bytes) e = hipMemcpy(tables[1].get(), d.table.data(), table_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, std::string("scene upload: ") + hipGetErrorString(e));
    for (int i = 0; i < 4; ++i)
        if (fresh[i]) *own[i] = std::move(fresh[i]);
    if (first) D.centres[0] = std::move(tables[0]), D.centres[1] = std::move(tables[1]);
    else std::swap(D.centres[0], D.centres[1]);
    for (int b = 0; b < 2; ++b) D.meta[b] = d.blobs[b];
    D.has_geom = d.has_geom;
    D.ground_ok = d.ground_ok;
    D.geom = std::move(d.geom);
    D.in_fast_range = d.in_fast_range;
    D.cur_table.swap(d.table);
    D.cur_flat.swap(d.flat);
    return RT_OK;
}

} // namespace

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

// The scene's own streams are synchronised before anything of the scene goes: work on them may
// still read its buffers (rt_scene.h). Then every member frees itself.
int rt_scene_destroy(rt_scene *sc)
{
    if (!sc) return RT_OK;
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(sc->device);
    for (const Stream &s : sc->xs)
        if (s) (void)hipStreamSynchronize(s.get());
    if (sc->ord.tile_st) (void)hipStreamSynchronize(sc->ord.tile_st.get());
    delete sc;
    (void)hipSetDevice(prev);
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
    sc->device = device;
    sc->dev.n_spheres = n_spheres;
    sc->dev.n_materials = n_materials;
    int rc = install_scene(sc, derived, true);
    if (rc == RT_OK) {
        hipError_t e = sc->queue_ctr.alloc(kCtrWords * sizeof(uint32_t));
        if (e != hipSuccess) rc = fail(RT_ERR_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(e));
        if (rc == RT_OK && (sc->deep_over.alloc(kMaxWs * sizeof(unsigned long long), hipHostMallocMapped) != hipSuccess ||
                            sc->deep_over.map(&sc->deep_over_dev) != hipSuccess))
            rc = fail(RT_ERR_DEVICE, "rt_scene_create: pinned host allocation failed");
        if (rc == RT_OK) std::memset(sc->deep_over.get(), 0, kMaxWs * sizeof(unsigned long long));
        for (uint32_t b = 0; b < kMaxWs && rc == RT_OK; ++b) {
            if ((b < kMaxBufs && sc->xs[b].make(hipStreamNonBlocking) != hipSuccess) ||
                sc->ev_done[b].make(hipEventDisableTiming) != hipSuccess || sc->ev_free[b].make(hipEventDisableTiming) != hipSuccess)
                rc = fail(RT_ERR_DEVICE, "rt_scene_create: stream/event creation failed");
        }
        if (rc == RT_OK && (sc->ev_tail.make(hipEventDisableTiming) != hipSuccess || sc->ev_sky.make(hipEventDisableTiming) != hipSuccess))
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
    if (rc == RT_OK) {
        sc->ev_begin.resize(rt_scene::kRing);
        sc->ev_end.resize(rt_scene::kRing);
        for (uint32_t i = 0; rc == RT_OK && i < rt_scene::kRing; ++i)
            if (sc->ev_begin[i].make(hipEventDefault) != hipSuccess || sc->ev_end[i].make(hipEventDefault) != hipSuccess)
                rc = fail(RT_ERR_DEVICE, "hipEventCreate failed");
    }
    if (rc != RT_OK) {
        rt_scene_destroy(sc);
        return rc;
    }
    *out = sc;
    return RT_OK;
}

int rt_scene_kernel_times(rt_scene *sc, uint32_t max, float *ms, uint32_t *n)
{
    if (!sc || !n || (max && !ms)) return fail(RT_ERR_INVALID, "rt_scene_kernel_times: null argument");
    const uint64_t avail = std::min<uint64_t>(sc->calls, rt_scene::kRing);
    const uint32_t cnt = static_cast<uint32_t>(std::min<uint64_t>(avail, max));
    RT_HIP(hipSetDevice(sc->device));
    for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t r = static_cast<uint32_t>((sc->calls - cnt + i) % rt_scene::kRing);
        RT_HIP(hipEventSynchronize(sc->ev_end[r].get()));
        RT_HIP(hipEventElapsedTime(ms + i, sc->ev_begin[r].get(), sc->ev_end[r].get()));
    }
    *n = cnt;
    return RT_OK;
}

int rt_scene_usage_get(const rt_scene *sc, rt_scene_usage *out)
{
    if (!sc || !out) return fail(RT_ERR_INVALID, "rt_scene_usage_get: null argument");
    rt_scene_usage u{};
    const Workspaces &W = sc->ws;
    uint64_t ws = W.acc.bytes() + W.mom.bytes() + W.wq.bytes();
    for (uint32_t w = 0; w < kMaxWs; ++w) ws += W.slots[w].bytes() + W.deep[w].bytes();
    uint64_t fixed = kCtrWords * sizeof(uint32_t) + (sc->dbg ? rt::kDbgWords * sizeof(unsigned long long) : 0u);
    for (int b = 0; b < 2; ++b) fixed += static_cast<uint64_t>(sc->dev.meta[b].units) * 16u;
    fixed += static_cast<uint64_t>(std::max(sc->dev.n_spheres, 1u)) * 16u;  // the trap windows
    fixed += static_cast<uint64_t>(sc->dev.n_spheres) * 32u;                // the two sphere tables (rt_scene_motion)
    // the ground kernel's redo lists and counts: beside the planner's cut, so in
    // device_bytes, not in workspace_bytes
    for (uint32_t w = 0; w < kMaxWs; ++w) fixed += W.redo[w].bytes();
    if (sc->redo_stat) fixed += rt_scene::kRing * sizeof(uint32_t);
    u.device_bytes = ws + fixed;
    u.workspace_bytes = ws;
    u.render_streams = sc->used.streams;
    u.workspaces = sc->used.ws;
    u.pass_samples = sc->used.pass;
    u.deep_launch = sc->used.deep;
    u.pair_passes = sc->used.pairs;
    u.split_passes = sc->used.split;
    u.lead_tiles = sc->used.lead;
    u.sky_tiles = sc->used.sky;
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
        RT_HIP(hipMemcpy(&redone, sc->redo_stat.get() + sc->ground_ring, sizeof(uint32_t), hipMemcpyDeviceToHost));
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
    DeviceScene &D = sc->dev;
    if (n_spheres != D.n_spheres)
        return fail(RT_ERR_INVALID, "rt_scene_update: n_spheres is " + std::to_string(n_spheres) + ", the scene has " +
                                        std::to_string(D.n_spheres) + " (ids link the frames: the count is fixed)");
    // what changed, by the bits
    bool geometry = false, appearance = false;
    for (uint32_t i = 0; i < n_spheres; ++i) {
        const rt_material &mt = materials[spheres[i].material];
        float row[4] = {spheres[i].center[0], spheres[i].center[1], spheres[i].center[2], spheres[i].radius}, flat[5];
        std::memcpy(flat, &mt.kind, 4);
        std::memcpy(flat + 1, mt.albedo, 12);
        flat[4] = mt.param;
        geometry = geometry || std::memcmp(row, D.cur_table.data() + 4 * static_cast<size_t>(i), 16) != 0;
        appearance = appearance || std::memcmp(flat, D.cur_flat.data() + 5 * static_cast<size_t>(i), 20) != 0;
    }
    if (!geometry && !appearance) {
        D.n_materials = n_materials;
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
    D.n_materials = n_materials;
    // the orders of the old geometry leave; a pool slot is free again (nothing reads it: the device is idle)
    sc->ord.clear();
    sc->deep_off.clear();
    sc->occ.reset();
    if (geometry) ++D.geometry_epoch;
    if (appearance) ++D.appearance_epoch;
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
    const DeviceScene &D = sc->dev;
    *out = rt_scene_motion_t{static_cast<uint32_t>(sizeof(rt_scene_motion_t)), D.n_spheres, D.centres[0].get(), D.centres[1].get(),
                             D.geometry_epoch, D.appearance_epoch};
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
    RT_HIP(hipMemcpy(out, sc->dbg.get(), 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) RT_HIP(hipMemset(sc->dbg.get(), 0, 16 * sizeof(uint64_t)));
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
    RT_HIP(hipMemcpy(out, sc->dbg.get() + rt::kDbgEvBase, rt::kDbgEvents * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) RT_HIP(hipMemset(sc->dbg.get() + rt::kDbgEvBase, 0, rt::kDbgEvents * sizeof(uint64_t)));
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
    RT_HIP(hipMemcpy(out, sc->dbg.get() + 16, 4 * static_cast<size_t>(waves) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    *n = waves;
    return RT_OK;
}

} // extern "C"

// the preview session (rt_host_post.cpp) allocates its planes where its scene lives
int rthost::scene_device(const rt_scene *sc) { return sc->device; }
