// rt_host_multi.cpp — the multi-GPU context of the C-ABI (rt_multi_*, rt_render_multi_*): per-rank
// scenes, interleaved row tiles, the gather over RCCL (or its stand-in) and the de-interleave.
// It reaches scenes through the public scene API only (rt_scene stays rt_scene.h's record, private to the files around it).
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rt_api.h"
#include "rt_hip_own.h"
#include "rt_host_build.h"
#include "rt_host_sync.h"

using namespace rthost;

// ---- single-process multi-GPU render: interleaved row tiles + RCCL gather over xGMI -----
// RCCL is opened with dlopen (librccl.so.1) on first use, so the library has no link-time
// dependency on it and shares the process's RCCL if another component (torch) loaded it.
namespace {
struct rccl_api {
    decltype(&ncclCommInitAll) comm_init_all = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclSend) send = nullptr;
    decltype(&ncclRecv) recv = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
    bool ok = false;
};
const rccl_api &rccl()
{
    static rccl_api api = [] {
        rccl_api a;
        void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return a;
        a.comm_init_all = reinterpret_cast<decltype(a.comm_init_all)>(dlsym(h, "ncclCommInitAll"));
        a.comm_destroy = reinterpret_cast<decltype(a.comm_destroy)>(dlsym(h, "ncclCommDestroy"));
        a.send = reinterpret_cast<decltype(a.send)>(dlsym(h, "ncclSend"));
        a.recv = reinterpret_cast<decltype(a.recv)>(dlsym(h, "ncclRecv"));
        a.group_start = reinterpret_cast<decltype(a.group_start)>(dlsym(h, "ncclGroupStart"));
        a.group_end = reinterpret_cast<decltype(a.group_end)>(dlsym(h, "ncclGroupEnd"));
        a.error_string = reinterpret_cast<decltype(a.error_string)>(dlsym(h, "ncclGetErrorString"));
        a.ok = a.comm_init_all && a.comm_destroy && a.send && a.recv && a.group_start && a.group_end && a.error_string;
        return a;
    }();
    return api;
}

// RT_DIAG_STANDIN_TRANSPORT: RCCL's point-to-point calls restated as stream-ordered device
// copies between ranks that share one device, so that the RCCL gather branch of
// rt_multi_render_device (grouped send/recv per peer on the ranks' streams, slot offsets, tile
// reuse across frames in flight) runs on one GPU. Semantics kept: within a group, a send on
// rank a's stream to peer b pairs with the receive on rank b's stream from a; the receive's
// stream waits for the send stream's prior work, copies, and the send stream's later work
// waits for the copy (the tile may not be overwritten before it has left), as with RCCL.
namespace standin {
struct comm { int rank, n, dev; };
struct op { bool is_send; const void *src; void *dst; size_t bytes; int peer; comm *c; hipStream_t st; };
thread_local std::vector<op> g_ops;
thread_local int g_depth = 0;
size_t type_bytes(ncclDataType_t t) { return t == ncclFloat ? 4u : t == ncclUint8 ? 1u : 0u; }
ncclResult_t comm_init_all(ncclComm_t *comms, int n, const int *devs)
{
    for (int i = 0; i < n; ++i) comms[i] = reinterpret_cast<ncclComm_t>(new comm{i, n, devs ? devs[i] : i});
    return ncclSuccess;
}
ncclResult_t comm_destroy(ncclComm_t c)
{
    delete reinterpret_cast<comm *>(c);
    return ncclSuccess;
}
ncclResult_t push(bool is_send, const void *src, void *dst, size_t count, ncclDataType_t t, int peer, ncclComm_t c,
                  hipStream_t st)
{
    comm *cc = reinterpret_cast<comm *>(c);
    if (!cc || !type_bytes(t) || peer < 0 || peer >= cc->n || peer == cc->rank) return ncclInvalidArgument;
    // only grouped calls are emulated: a call outside a group is refused and leaves nothing behind
    // for the next group to pair with
    if (!g_depth) return ncclInvalidUsage;
    g_ops.push_back({is_send, src, dst, count * type_bytes(t), peer, cc, st});
    return ncclSuccess;
}
ncclResult_t send(const void *buf, size_t count, ncclDataType_t t, int peer, ncclComm_t c, hipStream_t st)
{
    return push(true, buf, nullptr, count, t, peer, c, st);
}
ncclResult_t recv(void *buf, size_t count, ncclDataType_t t, int peer, ncclComm_t c, hipStream_t st)
{
    return push(false, nullptr, buf, count, t, peer, c, st);
}
ncclResult_t group_start()
{
    if (!g_depth) g_ops.clear();
    ++g_depth;
    return ncclSuccess;
}
ncclResult_t group_end()
{
    if (g_depth <= 0) return ncclInvalidUsage;
    if (--g_depth) return ncclSuccess;
    std::vector<op> ops;
    ops.swap(g_ops);
    std::vector<bool> used(ops.size(), false);
    ncclResult_t res = ncclSuccess;
    for (size_t i = 0; i < ops.size() && res == ncclSuccess; ++i) {
        if (!ops[i].is_send) continue;
        const op &sd = ops[i];
        size_t j = 0;
        for (; j < ops.size(); ++j)
            if (!used[j] && !ops[j].is_send && ops[j].c->rank == sd.peer && ops[j].peer == sd.c->rank) break;
        if (j == ops.size() || ops[j].bytes != sd.bytes) {
            res = ncclInvalidUsage;
            break;
        }
        used[i] = used[j] = true;
        const op &rv = ops[j];
        hipEvent_t sent = nullptr, landed = nullptr;
        if (hipEventCreateWithFlags(&sent, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&landed, hipEventDisableTiming) != hipSuccess || hipEventRecord(sent, sd.st) != hipSuccess ||
            hipStreamWaitEvent(rv.st, sent, 0) != hipSuccess ||
            hipMemcpyAsync(rv.dst, sd.src, sd.bytes, hipMemcpyDeviceToDevice, rv.st) != hipSuccess ||
            hipEventRecord(landed, rv.st) != hipSuccess || hipStreamWaitEvent(sd.st, landed, 0) != hipSuccess)
            res = ncclUnhandledCudaError;
        if (sent) (void)hipEventDestroy(sent);
        if (landed) (void)hipEventDestroy(landed);
    }
    for (size_t i = 0; i < ops.size() && res == ncclSuccess; ++i)
        if (!used[i]) res = ncclInvalidUsage;  // a receive without its send
    return res;
}
const char *error_string(ncclResult_t r) { return r == ncclSuccess ? "success" : "stand-in transport: unmatched or failed call"; }
} // namespace standin

const rccl_api &standin_api()
{
    static rccl_api api = [] {
        rccl_api a;
        a.comm_init_all = standin::comm_init_all;
        a.comm_destroy = standin::comm_destroy;
        a.send = standin::send;
        a.recv = standin::recv;
        a.group_start = standin::group_start;
        a.group_end = standin::group_end;
        a.error_string = standin::error_string;
        a.ok = true;
        return a;
    }();
    return api;
}
} // namespace

// Persistent multi-GPU context (rt_multi_*): rank r of N renders the rows y = r, r + N, ...
// (interleaved single rows balance sky against ground) on its device into a packed tile;
// optionally the gamma/u8 epilogue runs on the tile (3 B per pixel instead of 12 over xGMI);
// the tiles are gathered to rank 0's device and de-interleaved into the caller's frame.
// Everything that does not depend on the frame is built once at rt_multi_create: per-device
// scenes, rank streams, the RCCL communicators (ncclCommInitAll over the distinct devices), the
// segment counters; tiles and the gather buffer grow on first use of a frame size. Ranks that
// share a device with rank 0 ("virtual ranks": a one-GPU rehearsal of an N-way split) move
// their tile with a device copy where RCCL would send/recv; the tile layout, the gather buffer
// and the de-interleave are the same code either way.
struct rt_multi {
    int n = 0;
    std::vector<int> dev;
    bool rccl = false;  // every rank on its own device: gather over RCCL
    const rccl_api *api = nullptr;  // RCCL, or the stand-in (RT_DIAG_STANDIN_TRANSPORT)
    std::vector<rt_scene *> sc;
    std::vector<ncclComm_t> comm;
    // what a rank owns on its device (rt_multi_destroy lets it go with that device current)
    struct Rank {
        Stream st;              // rank r > 0: its stream (rank 0 runs on the caller's stream)
        DevBuf<float> tile;     // f32 tile
        DevBuf<uint8_t> tile8;  // u8 tile (RT_OUTPUT_RGB8)
        DevBuf<uint64_t> seg;   // {segments, sphere tests, box tests}
        Event ev_ready;         // a virtual rank: its tile is complete
    };
    std::vector<Rank> rk;
    DevBuf<char> gather;  // on rank 0's device: N slots of the largest tile
    Event ev_copied;      // caller stream: virtual ranks' tiles copied out
    bool copied_valid = false;
    Event ev_t0, ev_t1;
};

namespace {

int multi_fail_destroy(rt_multi *m, int rc);

uint32_t multi_rows(uint32_t H, int n, int r)
{
    return static_cast<uint32_t>(r) < H ? (H - static_cast<uint32_t>(r) + static_cast<uint32_t>(n) - 1) / static_cast<uint32_t>(n) : 0u;
}

} // namespace

extern "C" {

int rt_multi_create(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials, uint32_t n_materials,
                    const int *devices, int n_ranks, rt_multi **out)
{
    return rt_multi_create_ex(spheres, n_spheres, materials, n_materials, devices, n_ranks, nullptr, out);
}

int rt_multi_create_ex(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials, uint32_t n_materials,
                       const int *devices, int n_ranks, const rt_options *options, rt_multi **out)
{
    if (!out) return fail(RT_ERR_INVALID, "rt_multi_create: null output");
    *out = nullptr;
    rt_options opt;
    if (options) {
        if (int rc = check_options(*options); rc) return rc;
        opt = *options;
    } else if (int rc = default_options(opt); rc) {
        return rc;
    }
    // two supported layouts: every rank on its own device (RCCL), or every rank on rank 0's
    // device (virtual ranks); a mix would gather through cross-device copies no test covers.
    // Checked before any HIP call.
    bool distinct = true, all_same = true;
    if (devices && n_ranks > 0) {
        if (n_ranks > 64) return fail(RT_ERR_INVALID, "rt_multi_create: at most 64 ranks");
        for (int r = 1; r < n_ranks; ++r) {
            all_same = all_same && devices[r] == devices[0];
            for (int q = 0; q < r; ++q) distinct = distinct && devices[q] != devices[r];
        }
        if (!distinct && !all_same)
            return fail(RT_ERR_INVALID, "rt_multi_create: devices must be all distinct or all rank 0's device");
    }
    const bool standin = (opt.diag & RT_DIAG_STANDIN_TRANSPORT) != 0u;
    if (standin && !(devices && n_ranks > 1 && all_same))
        return fail(RT_ERR_INVALID, "rt_multi_create: the stand-in transport needs two or more ranks on one device");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RT_ERR_DEVICE, "rt_multi_create: no HIP device");
    const int N = n_ranks <= 0 ? ndev : n_ranks;
    if (!devices && N > ndev) return fail(RT_ERR_INVALID, "rt_multi_create: more ranks than devices (pass a device list)");
    if (N > 64) return fail(RT_ERR_INVALID, "rt_multi_create: at most 64 ranks");
    for (int r = 0; r < N; ++r) {
        const int d = devices ? devices[r] : r;
        if (d < 0 || d >= ndev) return fail(RT_ERR_INVALID, "rt_multi_create: bad device index");
    }
    rt_multi *m = new rt_multi();
    m->n = N;
    for (int r = 0; r < N; ++r) m->dev.push_back(devices ? devices[r] : r);
    m->rccl = N > 1 && (distinct || standin);
    m->api = standin ? &standin_api() : &rccl();
    m->sc.assign(N, nullptr);
    m->rk.resize(N);
    int rc = RT_OK;
    auto chk = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && rc == RT_OK) rc = fail(RT_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
        return rc == RT_OK;
    };
    for (int r = 0; r < N && rc == RT_OK; ++r) {
        rc = rt_scene_create_ex(spheres, n_spheres, materials, n_materials, m->dev[r], &opt, &m->sc[r]);
        if (rc != RT_OK) break;
        chk(hipSetDevice(m->dev[r]), "hipSetDevice");
        if (r > 0) chk(m->rk[r].st.make(hipStreamNonBlocking), "hipStreamCreate");
        chk(m->rk[r].seg.alloc(3 * sizeof(uint64_t)), "hipMalloc");
        chk(hipMemset(m->rk[r].seg.get(), 0, 3 * sizeof(uint64_t)), "hipMemset");
        chk(m->rk[r].ev_ready.make(hipEventDisableTiming), "hipEventCreate");
    }
    if (rc == RT_OK) {
        chk(hipSetDevice(m->dev[0]), "hipSetDevice");
        chk(m->ev_copied.make(hipEventDisableTiming), "hipEventCreate");
        chk(m->ev_t0.make(hipEventDefault), "hipEventCreate");
        chk(m->ev_t1.make(hipEventDefault), "hipEventCreate");
    }
    if (rc == RT_OK && m->rccl) {
        const rccl_api &api = *m->api;
        if (!api.ok) {
            rc = fail(RT_ERR_COMM, "rt_multi_create: librccl.so.1 not loadable");
        } else {
            m->comm.assign(N, nullptr);
            const ncclResult_t nr = api.comm_init_all(m->comm.data(), N, m->dev.data());
            if (nr != ncclSuccess) {
                m->comm.clear();
                rc = fail(RT_ERR_COMM, std::string("ncclCommInitAll: ") + api.error_string(nr));
            }
        }
    }
    if (rc != RT_OK) return multi_fail_destroy(m, rc);
    (void)hipSetDevice(m->dev[0]);
    *out = m;
    return RT_OK;
}

int rt_multi_destroy(rt_multi *m)
{
    if (!m) return RT_OK;
    for (int r = 0; r < m->n; ++r) {
        (void)hipSetDevice(m->dev[r]);
        if (m->rk[r].st) (void)hipStreamSynchronize(m->rk[r].st.get());
    }
    (void)hipSetDevice(m->dev[0]);
    (void)hipDeviceSynchronize();
    for (auto c : m->comm)
        if (c) m->api->comm_destroy(c);
    for (int r = 0; r < m->n; ++r) {
        (void)hipSetDevice(m->dev[r]);
        m->rk[r] = rt_multi::Rank{};
        if (m->sc[r]) rt_scene_destroy(m->sc[r]);
    }
    (void)hipSetDevice(m->dev[0]);
    delete m;  // (the gather buffer and the three events: rank 0's device)
    return RT_OK;
}

int rt_multi_info(const rt_multi *m, int *n_ranks, int *uses_rccl)
{
    if (!m) return fail(RT_ERR_INVALID, "rt_multi_info: null context");
    if (n_ranks) *n_ranks = m->n;
    if (uses_rccl) *uses_rccl = m->rccl ? 1 : 0;
    return RT_OK;
}

int rt_multi_render_device(rt_multi *m, const rt_camera *camera, const rt_params *params, uint32_t format,
                           void *d_out, void *stream)
{
    if (!m || !camera || !d_out) return fail(RT_ERR_INVALID, "rt_multi_render_device: null argument");
    if (format != RT_OUTPUT_F32 && format != RT_OUTPUT_RGB8) return fail(RT_ERR_INVALID, "rt_multi_render_device: bad format");
    if (int rc = check_params(params); rc != RT_OK) return rc;
    const rt_params base = *params;
    const int N = m->n;
    const uint32_t W = base.width, H = base.height;
    const size_t es = format == RT_OUTPUT_F32 ? 4u : 1u;
    const size_t row_vals = static_cast<size_t>(W) * 3u;
    const uint32_t rows_max = multi_rows(H, N, 0);
    hipStream_t cs = static_cast<hipStream_t>(stream);
    // buffers (grow only: a new, larger frame size costs one synchronisation)
    for (int r = 0; r < N; ++r) {
        const size_t rows = multi_rows(H, N, r);
        RT_HIP(hipSetDevice(m->dev[r]));
        if (int rc = m->rk[r].tile.ensure(std::max<size_t>(rows, 1) * row_vals * 4u); rc) return rc;
        if (format == RT_OUTPUT_RGB8)
            if (int rc = m->rk[r].tile8.ensure(std::max<size_t>(rows, 1) * row_vals); rc) return rc;
    }
    RT_HIP(hipSetDevice(m->dev[0]));
    if (N > 1)
        if (int rc = m->gather.ensure(static_cast<size_t>(N) * rows_max * row_vals * es); rc) return rc;
    auto tile_of = [&](int r) -> void * { return format == RT_OUTPUT_F32 ? static_cast<void *>(m->rk[r].tile.get()) : m->rk[r].tile8.get(); };
    // 1. every rank renders its rows (rank 0 on the caller's stream); virtual ranks wait until
    //    the caller stream has copied their previous tile out
    for (int r = 0; r < N; ++r) {
        const uint32_t rows = multi_rows(H, N, r);
        if (!rows) continue;
        rt_params p = base;
        p.row_offset = static_cast<uint32_t>(r);
        p.row_stride = static_cast<uint32_t>(N);
        p.num_rows = rows;
        p.flags &= ~static_cast<uint32_t>(RT_FLAG_FULL_FRAME);
        hipStream_t rs = r == 0 ? cs : m->rk[r].st.get();
        RT_HIP(hipSetDevice(m->dev[r]));
        if (r > 0 && !m->rccl && m->copied_valid) RT_HIP(hipStreamWaitEvent(rs, m->ev_copied.get(), 0));
        if (int rc = rt_render_device(m->sc[r], camera, &p, m->rk[r].tile.get(), rs, m->rk[r].seg.get()); rc) return rc;
        if (format == RT_OUTPUT_RGB8)
            RT_HIP(rt::launch_epilogue(m->rk[r].tile.get(), m->rk[r].tile8.get(),
                                       static_cast<uint64_t>(rows) * row_vals, rs));
        if (r > 0 && !m->rccl) RT_HIP(hipEventRecord(m->rk[r].ev_ready.get(), rs));
    }
    // 2. the gather: tile r -> slot r of the gather buffer on rank 0's device
    const size_t slot_bytes = static_cast<size_t>(rows_max) * row_vals * es;
    if (N > 1 && m->rccl) {
        const rccl_api &api = *m->api;
        ncclResult_t nr = api.group_start();
        for (int r = 1; r < N && nr == ncclSuccess; ++r) {
            const size_t cnt = static_cast<size_t>(multi_rows(H, N, r)) * row_vals;
            if (!cnt) continue;
            const ncclDataType_t ty = format == RT_OUTPUT_F32 ? ncclFloat : ncclUint8;
            nr = api.send(tile_of(r), cnt, ty, 0, m->comm[r], m->rk[r].st.get());
            if (nr == ncclSuccess)
                nr = api.recv(m->gather.get() + r * slot_bytes, cnt, ty, r, m->comm[0], cs);
        }
        const ncclResult_t ne = api.group_end();
        if (nr == ncclSuccess) nr = ne;
        if (nr != ncclSuccess) return fail(RT_ERR_COMM, std::string("RCCL gather: ") + api.error_string(nr));
    } else if (N > 1) {
        RT_HIP(hipSetDevice(m->dev[0]));
        for (int r = 1; r < N; ++r) {
            const size_t bytes = static_cast<size_t>(multi_rows(H, N, r)) * row_vals * es;
            if (!bytes) continue;
            RT_HIP(hipStreamWaitEvent(cs, m->rk[r].ev_ready.get(), 0));
            RT_HIP(hipMemcpyAsync(m->gather.get() + r * slot_bytes, tile_of(r), bytes,
                                  hipMemcpyDeviceToDevice, cs));
        }
        RT_HIP(hipEventRecord(m->ev_copied.get(), cs));
        m->copied_valid = true;
    }
    // 3. de-interleave on rank 0's device: frame row r + i N <- tile r row i
    RT_HIP(hipSetDevice(m->dev[0]));
    const size_t row_bytes = row_vals * es;
    for (int r = 0; r < N; ++r) {
        const uint32_t rows = multi_rows(H, N, r);
        if (!rows) continue;
        const void *src = r == 0 ? tile_of(0) : static_cast<const void *>(m->gather.get() + r * slot_bytes);
        RT_HIP(hipMemcpy2DAsync(static_cast<char *>(d_out) + r * row_bytes, row_bytes * N, src, row_bytes, row_bytes,
                                rows, hipMemcpyDeviceToDevice, cs));
    }
    return RT_OK;
}

} // extern "C"

namespace {

int multi_fail_destroy(rt_multi *m, int rc)
{
    const std::string msg = g_error;
    rt_multi_destroy(m);
    g_error = msg;
    return rc;
}

// Synchronous host-buffer frame through a context: every rank's counters are zeroed, the frame
// is enqueued on an internal stream of rank 0's device, copied to `out` and timed.
int multi_render_host(rt_multi *m, const rt_camera *camera, const rt_params *params, uint32_t format, void *out,
                      rt_stats *stats)
{
    if (!m || !camera || !out) return fail(RT_ERR_INVALID, "rt_multi_render: null argument");
    if (int rc = check_params(params); rc != RT_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t es = format == RT_OUTPUT_F32 ? 4u : 1u;
    const size_t bytes = static_cast<size_t>(params->width) * params->height * 3u * es;
    for (int r = 0; r < m->n; ++r) {
        RT_HIP(hipSetDevice(m->dev[r]));
        RT_HIP(hipMemset(m->rk[r].seg.get(), 0, 3 * sizeof(uint64_t)));
    }
    RT_HIP(hipSetDevice(m->dev[0]));
    DevBuf<char> d_out;
    Stream own_cs;
    RT_HIP(own_cs.make(hipStreamNonBlocking));
    const hipStream_t cs = own_cs.get();
    int rc = RT_OK;
    auto chk = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && rc == RT_OK) rc = fail(RT_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
        return rc == RT_OK;
    };
    chk(d_out.alloc(bytes), "hipMalloc");
    if (rc == RT_OK) chk(hipEventRecord(m->ev_t0.get(), cs), "hipEventRecord");
    if (rc == RT_OK) rc = rt_multi_render_device(m, camera, params, format, d_out.get(), cs);
    (void)hipSetDevice(m->dev[0]);
    if (rc == RT_OK) chk(hipEventRecord(m->ev_t1.get(), cs), "hipEventRecord");
    if (rc == RT_OK) chk(hipMemcpyAsync(out, d_out.get(), bytes, hipMemcpyDeviceToHost, cs), "hipMemcpyAsync");
    for (int r = 0; r < m->n; ++r) {
        (void)hipSetDevice(m->dev[r]);
        if (m->rk[r].st) chk(hipStreamSynchronize(m->rk[r].st.get()), "hipStreamSynchronize");
    }
    (void)hipSetDevice(m->dev[0]);
    chk(hipStreamSynchronize(cs), "hipStreamSynchronize");
    uint64_t segs[3] = {0, 0, 0};
    for (int r = 0; r < m->n && rc == RT_OK; ++r) {
        uint64_t v[3];
        (void)hipSetDevice(m->dev[r]);
        chk(hipMemcpy(v, m->rk[r].seg.get(), sizeof v, hipMemcpyDeviceToHost), "hipMemcpy");
        for (int i = 0; i < 3; ++i) segs[i] += v[i];
    }
    (void)hipSetDevice(m->dev[0]);
    float ms = 0.f;
    if (rc == RT_OK) chk(hipEventElapsedTime(&ms, m->ev_t0.get(), m->ev_t1.get()), "hipEventElapsedTime");
    if (rc == RT_OK && stats) {
        stats->primaries = static_cast<uint64_t>(params->width) * params->height * params->spp;
        stats->segments = segs[0];
        stats->sphere_tests = segs[1];
        stats->box_tests = segs[2];
        stats->kernel_ms = ms;
        stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return rc;
}

int render_multi_once(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials, uint32_t n_materials,
                      const rt_camera *camera, const rt_params *params, int ngpu, uint32_t format, void *out,
                      rt_stats *stats)
{
    if (!camera || !out) return fail(RT_ERR_INVALID, "rt_render_multi: null argument");
    if (int rc = check_params(params); rc != RT_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RT_ERR_DEVICE, "rt_render_multi: no HIP device");
    rt_multi *m = nullptr;
    if (int rc = rt_multi_create(spheres, n_spheres, materials, n_materials, nullptr,
                                 ngpu <= 0 ? ndev : std::min(ngpu, ndev), &m); rc)
        return rc;
    const int rc = multi_render_host(m, camera, params, format, out, stats);
    const std::string msg = g_error;
    rt_multi_destroy(m);
    g_error = msg;
    return rc;
}

} // namespace

extern "C" {

int rt_multi_render_f32(rt_multi *m, const rt_camera *camera, const rt_params *params, float *rgb_out, rt_stats *stats)
{
    return multi_render_host(m, camera, params, RT_OUTPUT_F32, rgb_out, stats);
}

int rt_multi_render_rgb8(rt_multi *m, const rt_camera *camera, const rt_params *params, uint8_t *rgb_out,
                         rt_stats *stats)
{
    return multi_render_host(m, camera, params, RT_OUTPUT_RGB8, rgb_out, stats);
}

int rt_render_multi_f32(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials,
                        uint32_t n_materials, const rt_camera *camera, const rt_params *params, int ngpu,
                        float *rgb_out, rt_stats *stats)
{
    return render_multi_once(spheres, n_spheres, materials, n_materials, camera, params, ngpu, RT_OUTPUT_F32, rgb_out,
                             stats);
}

int rt_render_multi_rgb8(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials,
                         uint32_t n_materials, const rt_camera *camera, const rt_params *params, int ngpu,
                         uint8_t *rgb_out, rt_stats *stats)
{
    return render_multi_once(spheres, n_spheres, materials, n_materials, camera, params, ngpu, RT_OUTPUT_RGB8, rgb_out,
                             stats);
}


} // extern "C"
