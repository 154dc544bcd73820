// rt_plan.h — the pass planner (rt_plan.cpp): how a frame is cut into render passes, streams and
// workspaces under the scene's options, and the sizes that follow from the cut (slot workspaces,
// deep queues, launch grids). Integer arithmetic over the frame and the options: no HIP and no
// scene, so it is part of the host-only half and of the CPU sanitizer builds (tests/sanitize).
#pragma once
#include <cstddef>
#include <cstdint>

#include "rt_host_build.h"

namespace rthost {

// the deep queue of a pass (sizes: rt_plan.cpp)
uint32_t deep_region_cap(uint64_t n_samples);
size_t deep_px_bytes(uint64_t n_pixels);
size_t deep_queue_bytes(uint64_t n_pixels, uint64_t n_samples);

// item dealing and the grid of a render launch (rt_plan.cpp)
float guided_l2b(uint32_t total_waves, bool in_flight);
constexpr uint64_t kShortPassItems = 32ull << 20;
int grid_wg_per_cu(int occ, bool in_flight, uint32_t streams, uint64_t pass_items);

// What the plan of a frame depends on: the frame, the scene's options, and what the kernel
// choice allows.
struct PlanInput {
    uint64_t n_pixels;  // below 2^31
    uint32_t spp;
    uint32_t streams;   // render_streams_of(options); 1 for the wavefront variant
    uint32_t workspaces_per_stream;
    uint64_t max_pass_bytes, max_workspace_bytes, ring_pass_bytes;  // rt_options
    uint32_t wave_queue_rays;                                       // rt_options
    bool wave;          // RT_FLAG_WAVEFRONT
    bool moments;       // the variance render: the per-pixel moments beside the multi-pass sums
    bool pairs_ok;      // the kernel of this frame has a sample-pair instantiation
    bool pairs_forced;  // RT_DIAG_PAIRS
    bool may_split;     // the passes may have a deep queue
};

// The cut. Workspaces 0..n_ws-1 are the ring's; lone_ws (n_ws when there is one, kMaxWs
// otherwise) is the lone passes' own workspace of single samples.
struct Plan {
    PlanInput in;
    uint32_t streams, wsps, n_ws, lone_ws;
    uint64_t spp_pass;      // the pass size the cap left (a multiple of 4 when below spp)
    uint64_t lone_samples;  // a pass issued alone when the frame runs whole
    uint64_t ring_samples;  // every other pass
    bool pairs;       // sample pairs taken (under the cap or forced)
    bool ring_pairs;  // ... by the ring's passes: pairs and more than one stream
    bool whole;       // a frame issued alone runs as one pass in lone_ws, beside a ring of smaller ones
    uint32_t wave_cap;  // rays per wavefront queue

    bool has_lone() const { return lone_ws < kMaxWs; }
    // slot rows of samples [a, b), a a multiple of 4: a full block of 4 takes two pair rows
    uint64_t slot_rows(uint64_t a, uint64_t b, bool paired) const;
    uint64_t pass_samples(uint32_t w) const { return w == lone_ws && whole ? lone_samples : ring_samples; }
    uint64_t slot_bytes(uint32_t w) const;  // the slots of workspace w
    uint64_t deep_bytes(uint32_t w) const;  // its deep queue (0: the passes are not split)
    uint64_t wave_bytes() const { return in.wave ? 2ull * wave_cap * 52u + 512u : 0u; }  // both ray queues and their counters
    uint64_t footprint() const;  // every workspace of the cut, the multi-pass sums and the ray queues
};

// RT_OK and the cut in `out`, or RT_ERR_INVALID ("too many pixels in one call") or
// RT_ERR_CAPACITY (max_workspace_bytes below one 4-sample pass). No allocation: it runs once
// per frame on the path that keeps frames in flight.
int plan_frame(const PlanInput &in, Plan &out);

} // namespace rthost
