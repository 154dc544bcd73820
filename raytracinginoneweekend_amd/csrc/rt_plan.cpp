// rt_plan.cpp — the pass planner (rt_plan.h): the cut of a frame into passes, streams and
// workspaces, the deep queue's sizes and the launch grids. Plain C++ (no HIP), compiled as
// rt_host_build.cpp is and checked by the stand-alone sanitizer program (tests/sanitize).
#include "rt_plan.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace rthost {

// Item dealing (guided): each queue's chunks shrink geometrically from 1/K of its remaining
// share per wave down to 128 items — few queue atomics, big coherent chunks for most of the
// launch, small ones at its end. Config 3 frame stream: K = 6 3.93 ms/frame with single-frame
// latency unchanged (5.3-5.4 ms); K = 4 3.89-3.92 but 6.2 ms latency; fixed 512-item chunks
// with a 64-item tail 4.39 ms (round 1; the fixed scheme was removed in round 4). A pass
// issued while no other render runs (a lone frame) deals with K = 12 — its end is not hidden
// by other launches, and smaller last chunks even it out (config 3 lone frame 3.37-3.45 vs
// 3.55-3.59 ms, frame stream alike at K = 6/9/12/16; profiles/r03/ab/guided_k.txt).
float guided_l2b(uint32_t total_waves, bool in_flight)
{
    const double k = in_flight ? 6.0 : 12.0;
    const double wq = std::max(1.0, total_waves / 8.0);
    const double beta = std::max(1.0 - 1.0 / (k * wq), 1.0 / (1 << 20));
    return static_cast<float>(std::log2(beta));
}

// Workgroups per CU of a render launch. A launch that finds no other render in flight (a
// single frame, the first of a stream) takes the occupancy: the lowest latency. One issued
// while earlier renders still run takes half of it, (occ + 1) / 2, so consecutive launches run
// side by side instead of each waiting for the previous one's workgroups to retire, and each
// one's drain overlaps the others' bulk: half the occupancy, and for passes of at most
// kShortPassItems samples with n render streams ceil(occ / (n - 1)) (4 streams: a third).
// Measured with 3 streams (occupancy 6, in-flight grid 3 / 4 / 6):
// config 3 frame stream 3.80-3.92 / 3.81-3.88 / 3.89-3.93 ms; 2-way row share 1.97-2.01 /
// 2.03-2.05 / 2.08; 8-way row share 0.63 / 0.66 / 0.68 (2: 0.66); configs 4 and 5 equal.
// With 4 streams (GPU_MAX_HW_QUEUES=8): grid 2: config 3 3.83-3.84 ms, 8-way 0.60-0.61; grid
// 3: 3.84-3.86, 0.65 — but config 3 with the corrected camera (7 segments per primary, 29 ms
// frames) 32.0-34.3 ms at grid 2 vs 29.8 at grid 3 (28.8 with 2 streams and full grids), so
// the third applies to short passes only. Round 3 re-swept 3/5/7 (7 streams): the default best
// or within noise (profiles/r03/ab/knobs_s3.txt).
#ifndef RT_SHORT_OTHERS  // A/B build switch: the divisor for short passes in flight (-1: streams - 1)
#define RT_SHORT_OTHERS -1
#endif
int grid_wg_per_cu(int occ, bool in_flight, uint32_t streams, uint64_t pass_items)
{
    if (!in_flight) return occ;
    const int short_others = RT_SHORT_OTHERS > 0 ? RT_SHORT_OTHERS : std::max(1, static_cast<int>(streams) - 1);
    const int others = pass_items <= kShortPassItems ? short_others
                                                     : std::min(2, std::max(1, static_cast<int>(streams) - 1));
    return std::max(1, (occ + others - 1) / others);
}

// deep queue of a pass: 8 regions of 1/1024 of its samples each (at least 512): 0.8% of the
// samples, where 0.2-0.3% reach the split depth on config 3; paths past a full region stay in the
// main launch. A pass of fewer than rt_options.deep_min_items samples (2^25) issued while no
// other render runs (a lone frame) is not split: its deep launch would be a serial tail of
// about max_depth - split iterations, which such a pass's own drain does not outweigh (config
// 3's 8-way row share alone: 1.28-1.30 ms split vs 1.03-1.10). Passes issued while others run
// (a frame stream) are split at any size: the unsplit drain costs issue (the 8-way share ran
// 42% more VALU instructions per sample than the full frame) and the deep launches run beside
// the other frames (8-way share, 7 streams: 0.50-0.51 ms per frame vs 0.58-0.59 unsplit).
uint32_t deep_region_cap(uint64_t n_samples)
{
    return static_cast<uint32_t>(std::max<uint64_t>(512u, n_samples / 1024u));
}
size_t deep_px_bytes(uint64_t n_pixels) { return (n_pixels + 255u) & ~static_cast<size_t>(255u); }
size_t deep_queue_bytes(uint64_t n_pixels, uint64_t n_samples)
{
    return deep_px_bytes(n_pixels) + static_cast<size_t>(8u) * deep_region_cap(n_samples) * 60u;
}

// Pass planning. The slot workspace of one pass (12 B per sample and pixel) stays within
// max_pass_bytes; passes hold a multiple of 4 samples so no reduce block straddles two.
// Frames in flight: render pass p runs on internal stream xs[p % bufs] with workspace
// w = p % n_ws, ordered after that stream's previous render and after the caller-stream
// work that last read workspace w (the accumulation of pass p - n_ws); render kernels
// touch no caller memory, so the caller stream sees the same results in the same order.
// One stream: everything on the caller stream. Under max_workspace_bytes one workspace per
// stream goes first, then the passes shrink (frames in flight are what keeps the machine
// full), then the streams; the bits never depend on the cut. Config 3 under 4 GiB: 2.68 ms
// per frame in that order (7 workspaces, 52-sample passes) vs 2.79 shrinking the passes first
// (14 workspaces, 24-sample passes), 2.56 uncapped (19.1 GiB; profiles/r04).
//
// Sample pairs: a pass's full blocks of 4 samples take two pair slots each,
// its tail samples one: half the slot memory. Their bookkeeping costs the main launch ~3% of
// the frame period (profiles/r05/ab/pairs_cost.txt), so they are taken under a workspace cap
// (after one workspace per stream, before shorter passes) or on request (diag `pairs`), by
// passes issued while other renders run; a pass issued alone (a lone frame) takes single
// samples, whose shorter items end the launch sooner (config 3: 3.23-3.26 vs 3.38-3.45 ms),
// in a workspace of its own beside the ring. Culled LDS kernels only (the wavefront variant,
// brute force and the scalar-cache variant store single samples).
namespace {

uint64_t per_sample(const PlanInput &f) { return f.n_pixels * 12ull; }

uint64_t rows_between(const PlanInput &f, uint64_t a, uint64_t b, bool pr)  // samples [a, b), a a multiple of 4
{
    const uint64_t full_blocks_end = f.spp & ~3u;  // samples [0, full_blocks_end) form blocks of 4
    const uint64_t nb = (std::min<uint64_t>(b, full_blocks_end) - std::min<uint64_t>(a, full_blocks_end)) / 4u;
    return pr ? (b - a) - 2u * nb : (b - a);
}
// the most slot rows of a pass of at most sp samples: a pass holding the tail (single samples)
// can take more rows than a full one (pairs)
uint64_t max_rows(const PlanInput &f, uint64_t sp, bool pr)
{
    uint64_t m = 0;
    for (uint64_t a = 0; a < f.spp; a += sp) m = std::max(m, rows_between(f, a, std::min<uint64_t>(f.spp, a + sp), pr));
    return m;
}
uint64_t ws_bytes(const PlanInput &f, uint64_t sp, bool pr) { return per_sample(f) * max_rows(f, sp, pr); }
uint32_t wave_cap_of(const PlanInput &f, uint64_t sp)
{
    return static_cast<uint32_t>(std::min<uint64_t>(f.n_pixels * std::min<uint64_t>(sp, f.spp), f.wave_queue_rays));
}
uint32_t n_ws_of(uint32_t streams, uint32_t wsps) { return streams > 1 ? streams * wsps : 1u; }

// Ring passes (rt_options.ring_pass_bytes): with frames in flight, a pass issued while other
// renders run holds at most that many slot bytes, the frame's samples cut into equal passes
// of a multiple of 4; a frame that fits one pass of max_pass_bytes and is issued alone (a
// lone frame, the drop-in's synchronous call) still runs in one pass, in a workspace of its
// own. The ring's 14 workspaces then hold 32-sample passes on config 3 (6.2 GiB in all
// instead of 19.2, frame period alike: profiles/r05/ab/ring_pass.txt) and the lone frame
// keeps its single launch pair. Ring passes hold at least kRingMinSamples samples per pixel:
// every pass reads and writes the frame's running sums (24 B per pixel), which 4-sample
// passes made 5% of config 4's frame (46.6 vs 44.2 ms); below that the passes stay as they were.
constexpr uint64_t kRingMinSamples = 32;
uint64_t ring_of(const PlanInput &f, uint64_t sp, uint32_t streams)
{
    const uint64_t sf = std::min<uint64_t>(sp, f.spp);
    if (streams <= 1 || !f.ring_pass_bytes) return sf;
    const uint64_t cap = (f.ring_pass_bytes / per_sample(f)) & ~3ull;
    if (cap >= sf || cap < kRingMinSamples) return sf;
    const uint64_t n = (f.spp + cap - 1) / cap;  // passes of the frame at that size
    return std::min<uint64_t>(cap, (((f.spp + n - 1) / n) + 3u) & ~3ull);
}
// a lone frame's one pass in its own workspace (beside the ring's smaller ones)
bool lone_whole(const PlanInput &f, uint64_t sp, uint32_t streams)
{
    return streams > 1 && sp >= f.spp && ring_of(f, sp, streams) < f.spp;
}
uint64_t dq_of(const PlanInput &f, uint64_t sp)
{
    return f.may_split ? deep_queue_bytes(f.n_pixels, f.n_pixels * std::min<uint64_t>(sp, f.spp)) : 0u;
}
// the ring's workspaces (pairs when there is a ring) and the lone passes' own one (singles:
// a whole lone frame, or a ring pass issued alone when the ring holds pairs)
uint64_t footprint_of(const PlanInput &f, uint32_t streams, uint32_t wsps, uint64_t sp, bool pairs)
{
    const uint64_t sr = ring_of(f, sp, streams);
    const bool ring_pairs = pairs && streams > 1, whole = lone_whole(f, sp, streams);
    uint64_t t = static_cast<uint64_t>(n_ws_of(streams, wsps)) * (ws_bytes(f, sr, ring_pairs) + dq_of(f, sr));
    if (whole) t += ws_bytes(f, sp, false) + dq_of(f, sp);
    else if (ring_pairs) t += ws_bytes(f, sr, false) + dq_of(f, sr);
    if (sr < f.spp) t += f.moments ? 2u * per_sample(f) : per_sample(f);  // the multi-pass sums (and moments)
    if (f.wave) t += 2ull * wave_cap_of(f, sp) * 52u + 512u;
    return t;
}

} // namespace

uint64_t Plan::slot_rows(uint64_t a, uint64_t b, bool paired) const { return rows_between(in, a, b, paired); }
uint64_t Plan::slot_bytes(uint32_t w) const { return ws_bytes(in, pass_samples(w), ring_pairs && w != lone_ws); }
uint64_t Plan::deep_bytes(uint32_t w) const { return dq_of(in, pass_samples(w)); }
uint64_t Plan::footprint() const { return footprint_of(in, streams, wsps, spp_pass, pairs); }

int plan_frame(const PlanInput &f, Plan &p)
{
    const uint64_t items_cap = ((1ull << 31) - 8192) / f.n_pixels;  // items fit 31 bits
    uint64_t spp_full = std::min<uint64_t>({f.spp, f.max_pass_bytes / per_sample(f), items_cap});
    if (spp_full < f.spp) spp_full &= ~3ull;
    if (spp_full == 0) spp_full = 4;
    if (f.n_pixels * std::min<uint64_t>(spp_full, f.spp) >= (1ull << 31) - 8192)
        return fail(RT_ERR_INVALID, "rt_render_device: too many pixels in one call");
    bool pairs = f.pairs_ok && f.pairs_forced;
    uint32_t bufs = f.streams, wsps = f.workspaces_per_stream;
    uint64_t spp_pass = spp_full;
    if (const uint64_t cap = f.max_workspace_bytes) {
        while (footprint_of(f, bufs, wsps, spp_pass, pairs) > cap) {
            if (bufs > 1 && wsps > 1) {
                wsps = 1;
                continue;
            }
            if (bufs > 1 && f.pairs_ok && !pairs) {
                pairs = true;
                continue;
            }
            if (spp_pass > 4) {
                spp_pass = std::max<uint64_t>(4, (std::min<uint64_t>(spp_pass, f.spp) - 1) & ~3ull);
                continue;
            }
            spp_pass = spp_full;
            if (bufs > 1) --bufs;
            else return fail(RT_ERR_CAPACITY, "rt_render_device: max_workspace_bytes " + std::to_string(cap) +
                                                  " below one 4-sample pass of this frame (" +
                                                  std::to_string(footprint_of(f, 1, 1, 4, pairs)) + " bytes)");
        }
    }
    p.in = f;
    p.streams = bufs;
    p.wsps = wsps;
    p.n_ws = n_ws_of(bufs, wsps);
    p.spp_pass = spp_pass;
    p.lone_samples = std::min<uint64_t>(spp_pass, f.spp);
    p.ring_samples = ring_of(f, spp_pass, bufs);
    p.pairs = pairs;
    p.ring_pairs = pairs && bufs > 1;
    p.whole = lone_whole(f, spp_pass, bufs);
    p.lone_ws = (p.ring_pairs || p.whole) ? p.n_ws : kMaxWs;  // the lone passes' workspace (singles), if any
    p.wave_cap = wave_cap_of(f, spp_pass);
    return RT_OK;
}

} // namespace rthost
