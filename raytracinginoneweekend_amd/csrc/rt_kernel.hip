// rt_kernel.hip — the hot path: per-pixel path tracing (color -> closest hit -> scatter) as a
// persistent HIP megakernel for gfx950 (CDNA4): render_body, its two kernels and their launchers.
// The device functions (vector math, RNG, closest hit) are rt_trace.h's; the other kernel families
// are translation units of their own (rt_sky.hip, rt_accum.hip, rt_compat.hip, rt_wavefront.hip,
// rt_aov.hip), so this unit's code object, which bench.kernel_sha256 stamps, holds the render
// kernels alone.
// Every binary32 op is separately rounded in the reference's order: this file is compiled
// with -ffp-contract=off and without fast-math, so div/sqrt are the correctly rounded
// sequences and NaN semantics (total internal reflection, src/math.hxx:308) survive.
//
// Execution model: one lane owns one work item (a block of 4 samples or
// one tail sample of one pixel) at a time. Every loop iteration traces ONE segment for every
// lane whose path is alive; lanes whose path ended refill from a per-wave item cursor
// (ballot + mbcnt prefix, no atomics), and the wave refills its cursor from one of 8 chunk
// queues. So lanes never idle waiting for the longest path of their wave (active-lane
// compaction across bounces) and the sphere loop always runs with the wave's live lanes.
#include "rt_trace.h"

namespace rt {

// ---- the megakernel ----------------------------------------------------------------------
// sphere ib's dielectric record {1 / ior, x(ior), x(1 / ior), shortcut word}, x(r) = (1 - r) / (1 + r),
// from LDS or global memory (the blob's tail)
template <int V, class KP>
__device__ __forceinline__ float4 dielectric_record(const KP &P, const float4 *blob, uint32_t ib)
{
    const uint32_t di = P.shade_offset + 2 * P.n_spheres + (P.n_spheres + 15u) / 16u + ib;
    if (V != V_EXACT_SCALAR && P.shade_lds) {
        const float4 r = blob[di];
        asm volatile("");  // no merged (flat) load with the global branch
        return r;
    }
    return gld4(P.blob, di);
}
#ifndef RT_MIN_WAVES_PER_SIMD
#define RT_MIN_WAVES_PER_SIMD 1  // measured: forcing 8 waves (64 VGPRs) spills and runs slower
#endif
// Structure 7 (the default) is held to 6 waves per SIMD: unhinted it takes 83 VGPRs (5 waves);
// hinted, the allocator keeps 79 and parks one 12-byte constant that only the metal-absorption
// path reloads (measured: 5.03-5.06 ms vs 5.19-5.24 per config-3 launch).
#ifndef RT_CULL7_WAVES
#define RT_CULL7_WAVES 7
#endif
template <int V, int CULL, bool STATS>
constexpr int kMinWaves = (CULL == 7 && !STATS) ? RT_CULL7_WAVES : RT_MIN_WAVES_PER_SIMD;
// the lone deep kernel's occupancy bound (waves per SIMD; 6: 3 workgroups of 8 waves per CU)
#ifndef RT_DEEP_REGHINT
#define RT_DEEP_REGHINT 0
#endif
#ifndef RT_DEEP_HOIST
// the lone deep kernel keeps its parameters in registers (106 SGPRs, no spills at its 6-wave bound;
// lone deep launch 0.341-0.351 vs 0.351-0.360 ms re-reading them, profiles/r05/deep/lone_deep_tmax.txt)
#define RT_DEEP_HOIST 1
#endif
#ifndef RT_DEEP_WIDE_WAVES
#define RT_DEEP_WIDE_WAVES 6
#endif
// The render loop; DEEP: the deep launch of a split pass (KParams::deep_mode),
// whose items are queued paths (no sample starts, no lens draws, no split) — its own
// instantiation, render_deep_kernel, so neither launch carries the other's code.
// WPB: waves per workgroup (4; the lone deep launch 8, which shares one LDS copy of the scene
// between twice the waves)
// PAIRS: the main launch of a pass that stores sample pairs (KParams::n_pair_items != 0,
// DESIGN.md §4.2), its own instantiation: the pair bookkeeping costs the loop ~3% of its issue
// LIST: the redo launch of a pass with a ground kernel, its own instantiation:
// the items are the words of the redo list `lx`, dealt in chunks of 64 by one atomic; each is
// rendered from scratch like any item of the main launch
template <int V, int CULL, bool STATS, bool COUNT, bool DEEP, int WPB, bool PAIRS, bool LIST = false>
__device__ __forceinline__ void render_body(const KParams &p, const RedoList &lx = RedoList{})
{
    constexpr bool FAST = (V == V_FAST_LDS);
    // Scene blob -> LDS (or read in place from global for the scalar-cache A/B variant):
    // [geo float4 x n_geo][sidx u32 x n_geo, 16-B padded][clusters float4 x 2 x n_clusters]
    extern __shared__ float4 lds_blob[];
    const float4 *blob;
    if constexpr (V == V_EXACT_SCALAR) {
        blob = p.blob;
    } else {
        for (uint32_t i = threadIdx.x; i < p.lds_units; i += blockDim.x) lds_blob[i] = p.blob[i];
        __syncthreads();
        blob = lds_blob;
    }
    // Per-render constants used only where a sample or an item starts are re-read from the
    // kernarg segment at each use (scalar loads) through a pointer made opaque every loop
    // iteration, so they do not pin ~30 SGPRs for the whole kernel (SGPR count bounds the
    // workgroups per CU on gfx950).
    typedef const __attribute__((address_space(4))) FrameConsts *fc_ptr_t;
    const fc_ptr_t fc_base =
        (fc_ptr_t)((const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr() +
                   offsetof(KParams, fc));
    typedef const __attribute__((address_space(4))) KParams *kp_ptr_t;
    const kp_ptr_t kp_base = (kp_ptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    const float4 *geo = blob;
    const uint32_t *sidx = reinterpret_cast<const uint32_t *>(blob + p.n_geo);
    const float4 *clus = blob + p.clus_offset;

    const uint32_t lane = threadIdx.x & 63u;
    // per-wave LDS of the transposed member tests
    TransposeLds *tw = nullptr;
    if constexpr (CULL == 7) {
        __shared__ TransposeLds s_tw[WPB];
        tw = &s_tw[threadIdx.x >> 6];
    }
    // per lane: a pending metal scatter's normal and roughness, or the geo entry {C, fl(r r)} of
    // the dielectric sphere the lane's path last hit (hint_candidate; its original index in lds_hid)
    __shared__ float4 lds_pn[64 * WPB];
    __shared__ uint32_t lds_hid[64 * WPB];
    __shared__ uint32_t lds_nb[64 * WPB];  // the dielectric sphere's shortcut word (hint_candidate)
    // (the lone deep kernel keeps the three in registers: RT_DEEP_REGHINT, an A/B build switch)
    constexpr bool kRegHint = DEEP && WPB == 8 && RT_DEEP_REGHINT;
    uint32_t r_hid = ~0u, r_nb = 0u;
    float4 r_pn = make_float4(0.f, 0.f, 0.f, 0.f);
    auto HID = [&](uint32_t sl) -> uint32_t & { if constexpr (kRegHint) return r_hid; else return lds_hid[sl]; };
    auto NB = [&](uint32_t sl) -> uint32_t & { if constexpr (kRegHint) return r_nb; else return lds_nb[sl]; };
    auto PN = [&](uint32_t sl) -> float4 & { if constexpr (kRegHint) return r_pn; else return lds_pn[sl]; };
    // sample pairs, per lane (structure of arrays): the main launch parks a pair's first colour
    // here while the lane traces the second (or, in word 0, the first's deep-queue index when it
    // went to the queue); the deep launch keeps the path's own queue index in word 0
    // (three words per lane for the pair's parked colour; one, the queue index, in the deep launch)
    __shared__ float lds_park[PAIRS ? 3 : 1][64 * WPB];
    auto park = [&](int c, uint32_t sl) -> float & { return lds_park[PAIRS ? c : 0][sl]; };
    const uint32_t wave_base = __builtin_amdgcn_readfirstlane(threadIdx.x & ~63u);

    // the deep launch's waves issue ahead of other launches' waves (KParams::deep_prio): each of
    // its paths is a chain of ~56 dependent iterations, which beside other renders' waves on the
    // same SIMD would take ~7x as long
    if (DEEP && p.deep_prio) __builtin_amdgcn_s_setprio(3);
    // wave-uniform cursor over the item space (the deep launch: over the queued paths)
    // (the main launch: q / 8 is the item group the wave deals from, KParams::n_groups)
    uint32_t q = blockIdx.x & 7u, q_tried = 0;
    // static dealing (KParams::deep_static): this wave's next chunk of the deep queue, in the
    // order of the regions' chunks; the grid's waves take chunks w, w + waves, w + 2 waves, ...
    uint32_t deep_next = __builtin_amdgcn_readfirstlane(blockIdx.x * (uint32_t)WPB + (threadIdx.x >> 6));
    uint32_t cnext = 0, cend = 0;
    // the main launch: the chunk's items [cnext, run_end) lie in one sample, at slots run_base + ...
    uint32_t run_end = 0, run_base = 0;
    bool exhausted = false;

    // lane state: the lane's item is one sample (pixel enumeration index, sample of the pass)
    bool alive = false;
    // the main launch: it = the item word (rt_device.h kIt*); the deep launch: pix = the path's
    // slot, ls = its pair link
    uint32_t it = 0, pix = 0, ls = 0;
    f3 o = mk(0.f, 0.f, 0.f), d = o, att = o;
    uint32_t depth = 0;
    uint64_t rng = 0;
    // a lambert/metal hit leaves its scatter offset to the next iteration's rejection loop:
    // o = hit point; d = p + n (lambert) or reflect(unit(d), n) (metal); the metal's normal and
    // roughness wait in the lane's LDS word (pn: 16 B per lane, no registers held across the loop)
    bool pend = false, pend_metal = false;
    // a fresh sample whose lens draw did not finish within RT_REJECT_CAP attempts: its camera
    // stream state waits in (o.x, o.y) and its jittered (u, v) in (d.x, d.y) until it does
    bool pend_lens = false;
    // HID(lane) != ~0: the lane's last hit was a dielectric sphere, tested first next segment
    // (hint_candidate); kept in LDS, not in a register (at 72 VGPRs one more value spills)
    HID(thread_slot(wave_base)) = ~0u;
    // the instrumented kernel: neighbour words that no dielectric hit wrote point past any blob
    // (hint_candidate's bounds check)
    if (STATS) NB(thread_slot(wave_base)) = 0x3fffffffu;
    WaveTally<COUNT> wt;
    Dbg dbg{};
    uint32_t dbg_iters = 0, dbg_refills = 0, dbg_iters_dry = 0, dbg_dealt = 0, dbg_walks = 0;
    uint32_t dbg_walks_nohint = 0;  // (deep launch) walks with a walking lane that has no hint sphere
    uint64_t t_dry = 0;  // STATS: realtime when this wave found every queue empty
    // STATS build only: shader-clock cycles per loop region, summed over the wave's iterations
    uint64_t cyc[5] = {0, 0, 0, 0, 0};  // refill, sample start, closest hit, shading, fold
    uint64_t t_prev = STATS ? __builtin_amdgcn_s_memtime() : 0;
    const uint64_t t_wave0 = STATS ? __builtin_amdgcn_s_memrealtime() : 0;  // 100 MHz clock
    auto stamp = [&](int r) {
        if (STATS) {
            const uint64_t t = __builtin_amdgcn_s_memtime();
            cyc[r] += t - t_prev;
            t_prev = t;
        }
    };

    for (;;) {
        stamp(4);
#ifdef RT_EXTRA_VALU  // timing probe only (scripts/build_variant.sh): RT_EXTRA_VALU more VALU per wave iteration
        {
            float e0 = o.x, e1 = o.y, e2 = o.z, e3 = d.x;
            asm volatile("" : "+v"(e0), "+v"(e1), "+v"(e2), "+v"(e3));
#pragma unroll
            for (int k = 0; k < RT_EXTRA_VALU / 4; ++k) {
                e0 = fmaf(e0, 1.0001f, 0.5f); e1 = fmaf(e1, 1.0001f, 0.5f);
                e2 = fmaf(e2, 1.0001f, 0.5f); e3 = fmaf(e3, 1.0001f, 0.5f);
            }
            asm volatile("" ::"v"(e0), "v"(e1), "v"(e2), "v"(e3));
        }
#endif
#ifdef RT_EXTRA_SALU  // timing probe only: RT_EXTRA_SALU more SALU per wave iteration
        {
            uint32_t s0 = __builtin_amdgcn_readfirstlane(pix);
#pragma unroll
            for (int k = 0; k < RT_EXTRA_SALU; ++k) asm volatile("s_add_u32 %0, %0, 3" : "+s"(s0));
            asm volatile("" ::"s"(s0));
        }
#endif
        fc_ptr_t fc = fc_base;
#if RT_DEEP_HOIST
        if (!(DEEP && WPB == 8))
#endif
        asm volatile("" : "+s"(fc));
        // the kernel parameters, re-read from the kernarg segment each iteration through an
        // opaque pointer: their uses (the deep split, the shading records, the refill) then
        // hold no SGPRs across the loop (31 SGPRs were spilled to VGPR lanes otherwise)
        kp_ptr_t kpp = kp_base;
#if RT_DEEP_HOIST
        if (!(DEEP && WPB == 8))
#endif
        asm volatile("" : "+s"(kpp));
        const __attribute__((address_space(4))) KParams &P = *kpp;
        // ---- refill items for idle lanes and start their samples -------------------
        uint64_t need = ballot(!alive);
        bool fresh = false;
        if (STATS && need && !exhausted && lane == 0) ++dbg_refills;
        while (need && !exhausted) {
            RT_EV(EV_REFILL_TRIP);
            // (the main launch: run_end <= cend, so a finished chunk is a finished run)
            if (DEEP ? cnext >= cend : cnext >= run_end) {
            if (cnext >= cend) {
                uint32_t c = 0;
                if constexpr (LIST) {
                    // the list's count is final (the ground kernel has ended): 64 items per ticket
                    if (lane == 0) c = atomicAdd(lx.ctr + kRedoDeal, 1u);
                    c = __builtin_amdgcn_readfirstlane(c);
                    const uint32_t n = __builtin_amdgcn_readfirstlane(min(lx.ctr[kRedoCount], lx.cap));
                    if (c >= (n + 63u) / 64u) {
                        exhausted = true;
                        continue;
                    }
                    cnext = 64u * c;
                    cend = min(64u * c + 64u, n);
                } else if constexpr (DEEP) {
                    if (WPB == 8 && P.deep_static) {  // (the lone deep launch's instantiation only)
                        // the regions' path counts are final (the main launch has ended): lanes
                        // 0-7 read them in one round trip; chunk j of the concatenated regions
                        // goes to wave j mod waves. No atomics: thousands of waves probing eight
                        // shared counters at the end of a launch cost more than the paths
                        const uint32_t n = lane < 8u ? min(P.deep.ctr[lane * kQueueStride + kDeepCount], P.deep.rcap) : 0u;
                        const uint32_t j = deep_next;
                        deep_next += gridDim.x * (uint32_t)WPB;
                        // lane k < 8: region k's chunks and their first index (exclusive prefix
                        // over lanes 0..k-1, three shuffle steps); the region holding chunk j
                        const uint32_t ck = (n + 63u) / 64u;
                        uint32_t incl = ck;
#pragma unroll
                        for (uint32_t off = 1; off < 8u; off <<= 1) {
                            const uint32_t v = (uint32_t)__shfl_up((int)incl, off);
                            if (lane >= off) incl += v;
                        }
                        const uint64_t hit = ballot(lane < 8u && j < incl && j >= incl - ck);
                        if (!hit) {
                            exhausted = true;
                            continue;
                        }
                        const uint32_t r = (uint32_t)__builtin_ctzll(hit);
                        const uint32_t base = (uint32_t)__builtin_amdgcn_readlane((int)(incl - ck), (int)r);
                        const uint32_t nr = (uint32_t)__builtin_amdgcn_readlane((int)n, (int)r);
                        cnext = r * P.deep.rcap + 64u * (j - base);
                        cend = r * P.deep.rcap + min(64u * (j - base) + 64u, nr);
                        goto deal;
                    }
                    // the deep launch: 64 queued paths per grab from region q, then the next
                    // region (a wave starts on its workgroup's region)
                    if (lane == 0) c = atomicAdd(P.deep.ctr + q * kQueueStride + kDeepDeal, 1u);
                    c = __builtin_amdgcn_readfirstlane(c);
                    const uint32_t nq = __builtin_amdgcn_readfirstlane(
                        min(P.deep.ctr[q * kQueueStride + kDeepCount], P.deep.rcap));
                    if (c >= (nq + 63u) / 64u) {
                        q = (q + 1u) & 7u;
                        if (++q_tried == 8u) exhausted = true;
                        continue;
                    }
                    cnext = __builtin_amdgcn_readfirstlane(q * P.deep.rcap + 64u * c);
                    cend = __builtin_amdgcn_readfirstlane(q * P.deep.rcap + min(64u * c + 64u, nq));
                } else {
                const uint32_t grp = q >> 3, qq = q & 7u;
                if (lane == 0) c = atomicAdd(P.queue_ctr + qq * kQueueStride + grp, 1u);  // word grp of queue qq's line
                c = __builtin_amdgcn_readfirstlane(c);
                // guided: queue q owns blocks [qb0, qb1) of 64 items of the group (group-local
                // indices, KParams::n_groups); ticket c takes blocks
                // [S(c), S(c+1)), S(t) = min(B, floor(B (1 - beta^t)) + 2t): chunks shrink
                // geometrically from ~B / (K waves per queue) to 2 blocks, so a queue is
                // served by few atomics and its last chunks are small. S is the same
                // function for every wave, so consecutive tickets tile the range; the 2t
                // term keeps it increasing even if exp2 or the float product is off by an
                // ulp (one block at most).
                const uint32_t GB = grp == 0u ? P.grp_blocks[0] : grp == 1u ? P.grp_blocks[1] : P.grp_blocks[2];
                const uint32_t qb0 = (uint32_t)(((uint64_t)GB * qq) >> 3);
                const uint32_t B = (uint32_t)(((uint64_t)GB * (qq + 1u)) >> 3) - qb0;
                auto S = [&](uint32_t t) -> uint32_t {
                    const float x = t ? exp2f((float)t * P.guided_l2b) : 1.f;
                    const uint64_t g = (uint64_t)floorf((float)B * (1.f - x)) + 2ull * t;
                    return g < B ? (uint32_t)g : B;
                };
                const uint32_t s0 = __builtin_amdgcn_readfirstlane(S(c));
                if (s0 >= B) {
                    // the group's next queue; after all 8, the next group (a group is dealt
                    // whole, by every wave, before the next one starts)
                    q = (q & ~7u) | ((q + 1u) & 7u);
                    if (++q_tried == 8u) {
                        q_tried = 0;
                        q += 8u;
                        if (q >= 8u * P.n_groups) exhausted = true;
                    }
                    continue;
                }
                const uint32_t GI = grp == 0u ? P.grp_items[0] : grp == 1u ? P.grp_items[1] : P.grp_items[2];
                cnext = 64u * (qb0 + s0);
                cend = __builtin_amdgcn_readfirstlane(min(64u * (qb0 + S(c + 1u)), GI));
                }
            }
            if constexpr (LIST) {
                run_end = cend;
                run_base = cnext;
            } else if constexpr (!DEEP) {
                // the chunk's run within one sample: group grp's item J is sample J / ng at
                // position p0 + J % ng, slot [sample][position] (sample-major over the pass's
                // permuted enumeration); one group (natural order): slot J
                const uint32_t grp = q >> 3;
                const uint32_t p0 = grp == 0u ? 0u : grp == 1u ? P.grp_pix[1] : P.grp_pix[2];
                const uint32_t ng = (grp == 0u ? P.grp_pix[1] : grp == 1u ? P.grp_pix[2] : P.grp_pix[3]) - p0;
                UDiv dv;
                dv.m = grp == 0u ? P.div_grp[0].m : grp == 1u ? P.div_grp[1].m : P.div_grp[2].m;
                dv.s1 = grp == 0u ? P.div_grp[0].s1 : grp == 1u ? P.div_grp[1].s1 : P.div_grp[2].s1;
                dv.s2 = grp == 0u ? P.div_grp[0].s2 : grp == 1u ? P.div_grp[1].s2 : P.div_grp[2].s2;
                const uint32_t sj = __builtin_amdgcn_readfirstlane(udiv(cnext, dv));
                run_end = __builtin_amdgcn_readfirstlane(min(cend, (sj + 1u) * ng));
                run_base = __builtin_amdgcn_readfirstlane(sj * P.n_pixels + p0 + (cnext - sj * ng));
            }
            }
        deal:
            const uint32_t avail = (DEEP ? cend : run_end) - cnext;
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32),
                                                            __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
            if (!alive && rank < avail) {
                uint32_t I = (DEEP ? cnext : run_base) + rank;
                if constexpr (DEEP) {
                    // a queued path resumes where the main launch left it: the ray of its next
                    // segment, attenuation, data stream and segment count; ls = 0 and pix = the
                    // slot index address the same slot
                    const uint32_t cap = 8u * P.deep.rcap;
                    I = checked<STATS>(I, cap, BC_DEEP_ITEM, p.dbg);
                    const float *f = P.deep.f;
                    o = mk(f[I], f[cap + I], f[2 * cap + I]);
                    d = mk(f[3 * cap + I], f[4 * cap + I], f[5 * cap + I]);
                    att = mk(f[6 * cap + I], f[7 * cap + I], f[8 * cap + I]);
                    rng = P.deep.rng[I];
                    pix = P.deep.slot[I];
                    ls = P.deep.link[I];  // the deep launch: ls is the path's pair link
                    depth = P.deep_mode;
                    alive = true;
                    // its hint sphere (hint_candidate): the geo entry from the shading record
                    const uint32_t hid = P.deep.hid[I], sl = thread_slot(wave_base);
                    lds_park[0][sl] = __uint_as_float(I);
                    if (hid != ~0u) {
                        // (from LDS when the launch staged the shading records there: a lone
                        // deep launch, whose refills then wait on no second global round trip)
                        const uint32_t ib = checked<STATS>(hid & 0x7fffffffu, P.n_spheres, BC_DEEP_HINT, p.dbg);
                        const uint32_t di = P.shade_offset + 2 * P.n_spheres + (P.n_spheres + 15u) / 16u + ib;
                        float4 sf, dr;
                        if (P.shade_lds) {
                            sf = blob[P.shade_offset + 2u * ib];
                            dr = blob[di];
                            asm volatile("");
                        } else {
                            sf = gld4(P.blob + P.shade_offset, 2u * ib);
                            dr = gld4(P.blob, di);
                        }
                        PN(sl) = make_float4(sf.x, sf.y, sf.z, sf.w * sf.w);
                        NB(sl) = __float_as_uint(dr.w);
                    }
                    HID(sl) = hid;
                } else {
                    // a pair item (the pass's full blocks) or a single tail sample; its slot
                    if constexpr (LIST) it = lx.items[checked<STATS>(I, lx.cap, BC_REDO_ITEM, p.dbg)];
                    else it = I;
                    alive = fresh = true;
                }
            }
            const uint32_t took = min((uint32_t)__popcll(need), avail);
            if (STATS) dbg_dealt += took;
            cnext += took;
            if (!DEEP) run_base += took;
            need = ballot(!alive);
        }

        // a pair whose first sample ended last iteration: its second sample starts now
        if (!DEEP && PAIRS && (it & kItRestart)) {
            fresh = true;
            it &= ~kItRestart;
        }
        stamp(0);
        // ---- start the sample of a freshly assigned item (main.cxx:192-200) -----------
        const uint64_t inc_data = ((uint64_t)fc->inc_data_hi << 32) | fc->inc_data_lo;
        // A sample's colour is final (main.cxx:205 sums it): a single's goes to its slot; a pair's
        // first is parked in the lane's scratch word and its second sample starts next iteration
        // (true: the lane sits out the rest of this one); the second's completes the pair sum
        // RN(c_2j + c_2j+1) in the pair's slot. In the deep launch the path's pair link says where
        // its partner's colour is.
        // the pixel (enumeration index) and the sample of the pass of the lane's item word
        auto item_pixel = [&](uint32_t &s) -> uint32_t {
            const uint32_t sl = it & kItSlot;
            const uint32_t npi = PAIRS ? (uint32_t)P.n_pair_items : 0u;
            const bool pr = sl < npi;
            const uint32_t J = pr ? sl : sl - npi;
            const uint32_t q = udiv(J, fc->div_n_pixels);
            s = !PAIRS ? q : pr ? 2u * q + (it >> 31) : 2u * fc->n_pairs + q;
            return J - q * fc->n_pixels;
        };
        auto finish = [&](f3 col) -> bool {
            float *dst;
            if constexpr (DEEP) {
                const uint32_t role = ls >> 30;
                dst = P.slots + (size_t)checked<STATS>(pix, P.n_slots, BC_SLOT, p.dbg) * 3u;
                if (role == kRolePartnerDone) {
                    // the partner ended in the main launch and left its colour in the slot
                    // (IEEE addition is commutative: the order of the pair's two terms is moot)
                    col = mk(dst[0], dst[1], dst[2]) + col;
                } else if (role != kRoleSingle) {
                    // both samples of the pair came here: the second of the two to end sums.
                    // Each leaves its colour in its own entry (its o.xyz words, read at its
                    // refill) with device-scope atomics, then counts its arrival at the first's
                    // entry; the one that finds the other arrived reads that colour back with
                    // atomics (device-scope atomics are coherent across the XCDs' L2s)
                    const uint32_t cap = 8u * P.deep.rcap, self = __float_as_uint(lds_park[0][thread_slot(wave_base)]);
                    const uint32_t partner = ls & kLinkIndex, first = role == kRoleBothFirst ? self : partner;
                    uint32_t *fw = reinterpret_cast<uint32_t *>(P.deep.f);
                    const uint32_t r = atomicExch(fw + self, __float_as_uint(col.x)) ^
                                       atomicExch(fw + cap + self, __float_as_uint(col.y)) ^
                                       atomicExch(fw + 2u * cap + self, __float_as_uint(col.z));
                    uint32_t one = 1u;
                    asm volatile("" : "+v"(one) : "v"(r));  // the arrival after the colour is stored
                    if (atomicAdd(P.deep.meet + first, one) != 1u) {
                        alive = false;  // the partner has not ended: it sums
                        return false;
                    }
                    const f3 cp = mk(__uint_as_float(atomicOr(fw + partner, 0u)), __uint_as_float(atomicOr(fw + cap + partner, 0u)),
                                     __uint_as_float(atomicOr(fw + 2u * cap + partner, 0u)));
                    col = role == kRoleBothFirst ? col + cp : cp + col;  // RN(c_2j + c_2j+1)
                    if (STATS) ++dbg.ev[EV_BOTH_MEET];
                    atomicExch(P.deep.meet + first, 0u);               // zero again for the next pass
                }
            } else {
                const uint32_t slot = it & kItSlot;
                if (PAIRS && slot < P.n_pair_items) {
                    const uint32_t sl = thread_slot(wave_base);
                    if (!(it & kItSecond)) {
                        park(0, sl) = col.x;
                        park(1, sl) = col.y;
                        park(2, sl) = col.z;
                        it |= kItSecond | kItRestart;
                        return true;
                    }
                    // the first's colour, unless it went to the deep queue (which then adds this one)
                    if (!(it & kItFirstDeep)) {
                        col = mk(park(0, sl), park(1, sl), park(2, sl)) + col;  // RN(c_2j + c_2j+1)
                        if (STATS) ++dbg.ev[EV_PAIR_SUM];
                    }
                }
                dst = P.slots + (size_t)checked<STATS>(slot, P.n_slots, BC_SLOT, p.dbg) * 3u;  // < 2^29: one pass holds <= 2 GiB of slots
            }
            dst[0] = col.x;
            dst[1] = col.y;
            dst[2] = col.z;
            alive = false;
            return false;
        };
        uint64_t rc = 0;  // the camera stream of a fresh sample
        float uu = 0.f, vv = 0.f;
        if (fresh) {
            RT_EV(EV_FRESH);
            uint32_t px, rr, ls;
            pixel_of(*fc, item_pixel(ls), px, rr, P.block_perm);
            const uint32_t py = fc->row_offset + rr * fc->row_stride;
            const uint32_t s = fc->sample_begin + ls;
            // key = (y W + x) spp + s (y W + x < 2^32: the host bounds W H)
            const uint64_t key = (uint64_t)(py * fc->W + px) * fc->spp + s;
            const uint64_t inc_cam = ((uint64_t)fc->inc_cam_hi << 32) | fc->inc_cam_lo;
            // pcg_seed(key, inc) = (inc + key) M + inc = key M + inc (M + 1): one vector multiply
            // for both streams, the inc (M + 1) terms are wave-uniform (scalar)
            const uint64_t km = key * kPcgMul;
            rng = km + inc_data * (kPcgMul + 1u);
            rc = km + inc_cam * (kPcgMul + 1u);
            const float fW = fc->fW, fH = fc->fH, rW = fc->rW, rH = fc->rH;
            const uint32_t df = fc->div_fast;
            const float xu = canonical(rng, inc_data);  // the u jitter's draw, then v's
            const float xv = canonical(rng, inc_data);
            if (df == 3u) {
                // both divisors take the checked short form (the common case): one uniform
                // branch for the four divisions instead of one per division
                uu = div_const((float)px, fW, rW, true) + div_const(xu, fW, rW, true);
                vv = div_const((float)py, fH, rH, true) + div_const(xv, fH, rH, true);
            } else {
                const bool fw = df & 1u, fh = df & 2u;
                uu = div_const((float)px, fW, rW, fw) + div_const(xu, fW, rW, fw);
                vv = div_const((float)py, fH, rH, fh) + div_const(xv, fH, rH, fh);
            }
            att = mk(1.f, 1.f, 1.f);
            depth = 0;
            HID(thread_slot(wave_base)) = ~0u;
        }
        // ---- one rejection loop for the wave (raytracer.hxx:32-43) ------------------------
        // Fresh lanes draw the lens offset from their camera stream (camera.hxx:52); lanes
        // whose last hit was lambert or metal draw their scatter offset from their data stream
        // (raytracer.hxx:135,147). Serving both in ONE loop makes the wave pay the longest
        // rejection run of the union of those lanes once per iteration instead of once per
        // kind; every stream still sees exactly its own draws in its own order.
        // A lane whose draws are not accepted within RT_REJECT_CAP attempts sits this iteration
        // out (`defer`) and resumes its own draw sequence in the next one: the wave no longer
        // waits for its unluckiest lane's whole run (mean 1.91 attempts, ~6.9 for the worst of
        // 64 lanes), and every stream still sees the same draws in the same order.
        bool defer = false;
        bool absorbed = false;  // a metal scatter absorbed: colour 0, finished at the iteration's end

        const bool lens = !DEEP && (fresh || pend_lens);
        if (lens || pend) {
            const uint64_t inc = lens ? (((uint64_t)fc->inc_cam_hi << 32) | fc->inc_cam_lo) : inc_data;
            if (pend_lens) {
                uu = d.x;
                vv = d.y;
                rc = ((uint64_t)__float_as_uint(o.y) << 32) | __float_as_uint(o.x);
            }
            uint64_t st = lens ? rc : rng;
            bool got;
            const f3 r = random_in_unit_sphere_capped<STATS>(st, inc, got, dbg);
            if (!got) {
                defer = true;
                if (lens) {
                    pend_lens = true;
                    o.x = __uint_as_float((uint32_t)st);
                    o.y = __uint_as_float((uint32_t)(st >> 32));
                    d.x = uu;
                    d.y = vv;
                } else {
                    rng = st;  // pend stays set
                }
            } else if (lens) {
                RT_EV(EV_LENS_DONE);
                pend_lens = false;
                // camera.hxx:46-57
                const f3 rd = r * fc->lens;
                const f3 off = mk(uu * rd.x, vv * rd.y, 0.f);
                const f3 org = mk(fc->org[0], fc->org[1], fc->org[2]);
                o = org + off;
                d = ((mk(fc->llc[0], fc->llc[1], fc->llc[2]) + mk(fc->hor[0], fc->hor[1], fc->hor[2]) * uu) +
                     mk(fc->ver[0], fc->ver[1], fc->ver[2]) * (1.f - vv)) - off;
                if (fc->corrected) d = d - org;
            } else {
                RT_EV(EV_SCATTER_DONE);
                rng = st;
                if (!pend_metal) {
                    d = (d + r) - o;                       // lambert :135, d held p + n, o = p
                } else {
                    const float4 pn = PN(thread_slot(wave_base));
                    const f3 nd = d + r * pn.w;            // metal :147, d held reflect(unit(d), n)
                    if (dot(nd, mk(pn.x, pn.y, pn.z)) > 0.f) {
                        d = nd;
                    } else {                               // absorbed: main.cxx:68, colour 0
                        RT_EV(EV_METAL_ABSORB);
                        absorbed = defer = true;  // it traces nothing more
                    }
                }
                pend = false;
            }
        }
        stamp(1);
        // no live lane: the wave's refill found the item space exhausted (a metal path absorbed
        // above stays alive until finish() stores its colour at the end of this iteration)
        if (ballot(alive) == 0) {
            if (exhausted) break;
            continue;
        }
        // ---- deep-path split: a path that has traced deep_depth segments (with its scatter
        // resolved) moves to the deep queue, whole state, and the lane takes a new item next
        // iteration. The few paths that run to max_depth (the reference's refract traps rays in
        // glass spheres) then no longer hold this launch's waves for ~max_depth iterations after
        // the item queues run dry; the deep launch runs them with every lane busy. Each path
        // sees the same operations and draws in the same order: same bits.
        // A path goes to region (its dielectric sphere's index) % 8 of the queue, or
        // blockIdx % 8 if its last hit was not dielectric: the paths trapped in one sphere then
        // share a region, and the deep launch's waves, which deal 64 paths at a time from one
        // region, trace paths of the same few spheres, whose segments reach the same few
        // clusters (8 counters on separate lines spread the appends). A path that finds its
        // region full stays in this launch.
        if (!DEEP && P.deep_depth) {
            const bool dv = alive && !defer && depth == P.deep_depth;
            if (ballot(dv)) {
                uint32_t j = ~0u, r = 0;
                if (dv) {
                    const uint32_t hid = HID(thread_slot(wave_base));
                    r = hid != ~0u ? (hid & 7u) : (blockIdx.x & 7u);
                    j = atomicAdd(P.deep.ctr + r * kQueueStride + kDeepCount, 1u);
                }
                if (dv && j < P.deep.rcap) {
                    const uint32_t cap = 8u * P.deep.rcap;
                    j = checked<STATS>(j + r * P.deep.rcap, cap, BC_DEEP_APPEND, p.dbg);
                    uint32_t ss;
                    const uint32_t px = checked<STATS>(item_pixel(ss), fc->n_pixels, BC_DEEP_PX, p.dbg);
                    float *f = P.deep.f;
                    f[j] = o.x; f[cap + j] = o.y; f[2 * cap + j] = o.z;
                    f[3 * cap + j] = d.x; f[4 * cap + j] = d.y; f[5 * cap + j] = d.z;
                    f[6 * cap + j] = att.x; f[7 * cap + j] = att.y; f[8 * cap + j] = att.z;
                    P.deep.rng[j] = rng;
                    P.deep.hid[j] = HID(thread_slot(wave_base));
                    P.deep.px[px] = 1;
                    // the path's slot and pair link (rt_device.h kRole*)
                    const uint32_t slot = it & kItSlot, sl = thread_slot(wave_base);
                    uint32_t link = kRoleSingle << 30;
                    if (!PAIRS || slot >= P.n_pair_items) {
                        alive = false;
                    } else {
                        link = kRolePartnerDone << 30;
                        if (!(it & kItSecond)) {
                            // the pair's first: the lane traces the second next iteration, which
                            // leaves its colour in the slot (or joins this one in the queue)
                            lds_park[0][sl] = __uint_as_float(j);
                            it |= kItSecond | kItFirstDeep | kItRestart;
                            defer = true;  // sits out the rest of this iteration
                        } else {
                            if (it & kItFirstDeep) {  // both of the pair queued: they meet there
                                const uint32_t j1 = __float_as_uint(lds_park[0][sl]);
                                link = (kRoleBothSecond << 30) | j1;
                                P.deep.link[j1] = (kRoleBothFirst << 30) | j;
                            } else {  // the first's colour, parked in the lane's LDS words, to the slot
                                float *dst = P.slots + (size_t)checked<STATS>(slot, P.n_slots, BC_SLOT, p.dbg) * 3u;
                                dst[0] = park(0, sl);
                                dst[1] = park(1, sl);
                                dst[2] = park(2, sl);
                            }
                            alive = false;
                        }
                    }
                    P.deep.slot[j] = slot;
                    P.deep.link[j] = link;
                }
            }
        }
        RT_EV(EV_ITER);
        if (STATS) {
            const uint32_t nl = lanes(alive);
            if (first_active_lane()) {
                dbg.ev[EV_LIVE_LANES] += nl;
                if (exhausted) {
                    ++dbg.ev[EV_DRY_ITER];
                    dbg.ev[EV_DRY_LANES] += nl;
                }
            }
        }
        if (STATS && lane == 0) {
            ++dbg_iters;
            if (exhausted) {
                if (!dbg_iters_dry) t_dry = __builtin_amdgcn_s_memrealtime();
                ++dbg_iters_dry;
            }
        }

        // ---- closest hit of one segment for every live lane -----------------------------
        const bool seg = alive && !defer && depth < P.max_depth;  // depth check: main.cxx:74
        // |d|^2 (raytracer.hxx:56) and its refined reciprocal for this segment's roots; the sky
        // below reuses both (unit_direction's length is sqrt of the same sum)
        const float a = d.x * d.x + d.y * d.y + d.z * d.z;
        const uint64_t segm = ballot(seg);
        const RayDiv rd = ray_div(a, segm, P.fast_roots);
        Hit h{kNoHit};
        if constexpr (CULL == 7) {  // whole wave: every lane helps with transposed member tests
            uint64_t key0 = no_hit();
            bool skip = false;
            const uint32_t sl = thread_slot(wave_base);
            const uint32_t hid = HID(sl);
            if (ballot(seg && hid != ~0u))
                key0 = hint_candidate<FAST, STATS>(seg && hid != ~0u, PN(sl), hid, NB(sl), geo, sidx, o, d, rd, P.iso,
                                                   skip, P.n_geo, P.diag_unbounded_nb, p.dbg);
            const bool walk = seg && !skip;
            const uint64_t wm = ballot(walk);
            if (STATS && first_active_lane()) {
                dbg.ev[EV_ISO_LANES] += (uint32_t)__popcll(segm & ~wm);
                if (segm && !wm) ++dbg.ev[EV_WALK_SKIPPED];
                const uint32_t nw = (uint32_t)__popcll(wm);
                if (nw == 1u) ++dbg.ev[EV_WALK1];
                else if (nw == 2u) ++dbg.ev[EV_WALK2];
                else if (nw >= 3u && nw <= 4u) ++dbg.ev[EV_WALK4];
                else if (nw >= 5u && nw <= 8u) ++dbg.ev[EV_WALK8];
            }
            if (STATS) {
                const uint64_t nh = ballot(walk && hid == ~0u);
                if (lane == 0 && wm) ++dbg_walks;  // iterations in which the wave walked
                if (lane == 0 && nh) ++dbg_walks_nohint;
            }
            h = closest_hit<FAST, CULL, STATS, COUNT>(P, geo, sidx, clus, o, d, rd, dbg, wt, walk, wm, tw, key0);
            if (!seg) h = Hit{kNoHit};
        } else if (seg) {
            h = closest_hit<FAST, CULL, STATS, COUNT>(P, geo, sidx, clus, o, d, rd, dbg, wt, true, segm, nullptr, no_hit());
        }
        stamp(2);
        {
            const uint32_t ns = lanes(seg);  // segments of this iteration (main.cxx:74 passed)
            wt.add_seg(ns);
            wt.add_sph((uint64_t)ns * P.n_always);
        }

        // ---- shading: the hit of every live lane -----------------------------------------
        bool done = absorbed;
        f3 col = mk(0.f, 0.f, 0.f);
        uint32_t trap_rem = 0;  // COUNT: the segments a path ended by its trap window would still trace
        if (alive && !defer) {
            if (!seg) {
                done = true;  // main.cxx:74 (only reachable with max_depth == 0)
            } else {
                const float t = h.t();
                uint32_t ib = h.id();
                ++depth;
                if (ib == 0xffffffffu) {
                    RT_EV(EV_SKY);
                    // main.cxx:71: background(.5 * unit_direction.y + 1) * attenuation. With the
                    // short forms (rd.fd: a in [2^-40, 2^40]) the length is sqrt_scaled(a) >= 2^-20
                    // and d.y / length is exact unless |d.y| < 2^-100, where both forms give
                    // |y| < 2^-80 and tt rounds to 1 either way.
                    float uy;
                    if (rd.fd != 0u) {
                        const float l = sqrt_scaled(a);
                        const float y0 = __builtin_amdgcn_rcpf(l);
                        uy = div_ray(d.y, RayDiv{l, fmaf(fmaf(-l, y0, 1.f), y0, y0), true});
                    } else {
                        uy = normalize(d).y;
                    }
                    const float tt = .5f * uy + 1.f;
                    const f3 bg = mk(1.f, 1.f, 1.f) * (1.f - tt) + mk(.5f, .7f, 1.f) * tt;
                    col = bg * att;
                    done = true;
                } else if (depth >= P.max_depth) {
                    // main.cxx:65-74: a scattered ray would not be traced and an absorbed one
                    // returns 0 too; this sample's streams are not drawn from again
                    done = true;
                } else {
                    RT_EV(EV_HIT);
                    ib = checked<STATS>(ib, P.n_spheres, BC_SHADE, p.dbg);
                    float4 sf, md;
                    uint32_t kind;
                    if (V != V_EXACT_SCALAR && P.shade_lds) {
                        const float4 *shade = blob + P.shade_offset;
                        sf = shade[2 * ib];
                        md = shade[2 * ib + 1];
                        kind = reinterpret_cast<const uint8_t *>(shade + 2 * P.n_spheres)[ib];
                        asm volatile("");  // keeps the LDS and global loads apart (no sinking)
                    } else {
                        // global memory, named as such: the two branches' loads would otherwise be
                        // merged into flat loads through a selected pointer
                        const float4 *shade = P.blob + P.shade_offset;
                        sf = gld4(shade, 2 * ib);
                        md = gld4(shade, 2 * ib + 1);
                        kind = ((const __attribute__((address_space(1))) uint8_t *)(shade + 2 * P.n_spheres))[ib];
                    }
                    const f3 ctr = mk(sf.x, sf.y, sf.z);
                    const f3 hp = o + d * t;                    // ray::point_at, math.hxx:353
                    // raytracer.hxx:71. With the scene in the short-form range (|r| in [2^-40, 2^19],
                    // P.fast_roots) the division by r takes the short form unless a lane's offset has
                    // a component below 2^-100 (zero included).
                    const f3 dv = hp - ctr;
                    f3 hn;
                    if (P.fast_roots && all_lanes_min_abs_ok(dv)) hn = div3_short(dv, sf.w);
                    else hn = dv / sf.w;
                    att = att * mk(md.x, md.y, md.z);           // main.cxx:65 (unused if absorbed)
                    // raytracer.hxx:120-199
                    o = hp;
                    if (kind != 2u) HID(thread_slot(wave_base)) = ~0u;  // no hint after lambert, metal
                    if (kind == 0u) {                           // lambert, :132-141
                        RT_EV(EV_LAMBERT);
                        d = hp + hn;                            // + rius next iteration, then - p
                        pend = true;
                        pend_metal = false;
                    } else {
                        // metal and dielectric lanes share one unit direction and one reflection
                        // (one code path for the wave instead of two)
                        RT_EV(EV_UNIT_DIR);
                        // unit_vector(d) (math.hxx:219-227): length sqrt(a) with a = |d|^2 as above;
                        // under rd.fd, a in [2^-40, 2^40], so the length is sqrt_scaled(a) in
                        // [2^-20, 2^20] and the three divisions take the short form unless a
                        // lane's direction has a component below 2^-100
                        f3 ud;
                        if (rd.fd != 0u && all_lanes_min_abs_ok(d)) ud = div3_short(d, sqrt_scaled(a));
                        else ud = normalize(d);
                        const f3 rf = reflect(ud, hn);
                        if (kind == 1u) {                       // metal, :143-156
                            d = rf;                             // + rius * roughness next iteration
                            PN(thread_slot(wave_base)) = make_float4(hn.x, hn.y, hn.z, md.w);
                            pend = true;
                            pend_metal = true;
                        } else {                                // dielectric, :158-194
                            RT_EV(EV_DIELECTRIC);
                            // {1 / ior, x(ior), x(1 / ior), shortcut word} of this sphere, x(r) = (1 - r) / (1 + r)
                            const float4 dcs = dielectric_record<V>(P, blob, ib);
                            {   // the next segment tests this sphere first (hint_candidate)
                                const uint32_t sl = thread_slot(wave_base);
                                PN(sl) = make_float4(sf.x, sf.y, sf.z, sf.w * sf.w);  // its geo entry, raytracer.hxx:58
                                const uint32_t w = __float_as_uint(dcs.w);  // its shortcut word
                                HID(sl) = ib | (w & kShortcut);
                                NB(sl) = w;
                            }
                            f3 outward = mk(-hn.x, -hn.y, -hn.z);
                            float ri = md.w, xs = dcs.y;
                            float cosv = dot(ud, hn);
                            const bool inside = cosv > 0.f;
                            if (cosv <= 0.f) {
                                outward = outward * -1.f;
                                ri = dcs.x;                     // 1.f / ri
                                xs = dcs.z;
                                cosv *= -1.f;
                            }
                            const f3 refr = refract(ud, outward, ri);
                            float prob = 1.f;
                            // length(refr) > 0 <=> norm > 0 (correctly rounded sqrt; NaN -> false)
                            const float rn = refr.x * refr.x + refr.y * refr.y + refr.z * refr.z;
                            if (rn > 0.f) {
                                prob = schlick_x(xs, cosv);
                            } else if (inside && rn != rn) {
                                // Total reflection inside the ball (refract gave NaN: reflected with
                                // probability 1). With the cosine in the ball's trap window (rt_host_build.cpp
                                // trap_windows) every later hit is proven to be this
                                // ball's far root on this branch until max_depth, where the path returns 0
                                // (main.cxx:74): it ends here with that colour. Ordered compares: a NaN
                                // cosine never triggers. The skipped draws are this sample's own.
                                const __attribute__((address_space(1))) float *win =
                                    (const __attribute__((address_space(1))) float *)(P.trap + ib);
                                if (cosv >= win[0] && cosv <= win[1]) {
                                    done = true;
                                    if (COUNT) trap_rem = P.max_depth - depth;
                                }
                            }
                            d = canonical(rng, inc_data) < prob ? rf : refr;
                        }
                    }
                }
            }
            stamp(3);
        }
        if constexpr (COUNT) {
            // the tally stays the reference's hit_world count: the segments the ended paths skip
            uint32_t r = trap_rem;
            for (int off = 32; off >= 1; off >>= 1) r += (uint32_t)__shfl_xor((int)r, off);
            wt.add_seg(r);
        }
        if (done) {
            RT_EV(EV_STORE);
            // the sample's colour goes to its slot or its pair; accumulate_kernel forms the
            // reference's blocked sum over the slots (main.cxx:205)
            finish(col);
        }
    }

    if (COUNT && p.segments) {
        // wave reductions, one atomic per wave and counter: [0] segments, [1] sphere tests,
        // [2] cluster box tests (lane-level, executed)
        if (lane == 0) {  // one atomic per wave and counter
            atomicAdd(p.segments + 0, (unsigned long long)wt.seg);
            atomicAdd(p.segments + 1, (unsigned long long)wt.sph);
            atomicAdd(p.segments + 2, (unsigned long long)wt.box);
        }
    }
    if (STATS && p.dbg) {
        const uint32_t c[8] = {dbg_iters, dbg_refills, dbg.wave_blocks, dbg.lane_blocks, dbg.wave_roots,
                               dbg.lane_roots, lane == 0 ? (uint32_t)wt.seg : 0u, dbg.wave_member_blocks};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            unsigned long long v = c[i];
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
            if (lane == 0) atomicAdd(p.dbg + i, v);
        }
#pragma unroll
        for (int i = 0; i < (int)EV_COUNT; ++i) {
            unsigned long long v = dbg.ev[i];
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
            if (lane == 0) atomicAdd(p.dbg + kDbgEvBase + i, v);
        }
        if (lane == 0) {
            for (int i = 0; i < 5; ++i) atomicAdd(p.dbg + 8 + i, (unsigned long long)cyc[i]);
            atomicMax(p.dbg + 14, ~t_wave0);  // launch start = ~max(~t) = earliest wave start
            atomicAdd(p.dbg + 13, (unsigned long long)dbg_dealt);  // items (deep: paths) dealt
        }
        // wave timeline: [16 + 4w] time the queues were found dry (realtime ticks), [17 + 4w] exit,
        // [18 + 4w] shader-clock cycles in the loop << 32 | refill rounds << 16 | loop iterations,
        // [19 + 4w] hardware id << 48 | iterations after dry << 32 | the wave's start (low 32 bits of
        // the realtime clock); w = wave of the grid. The launch starts at t_wave0 of the earliest wave.
        const uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        if (lane == 0 && w < kDbgWaves) {
            const unsigned long long cy = cyc[0] + cyc[1] + cyc[2] + cyc[3] + cyc[4];
            // (a deep launch: the walks with a lane that has no hint sphere << 32 | the walks)
            p.dbg[16 + 4 * w] = DEEP ? ((unsigned long long)dbg_walks_nohint << 32 | dbg_walks)
                                     : (t_dry ? t_dry : __builtin_amdgcn_s_memrealtime());
            p.dbg[17 + 4 * w] = __builtin_amdgcn_s_memrealtime();
            p.dbg[18 + 4 * w] = (min(cy, 0xffffffffull) << 32) | (min(dbg_refills, 65535u) << 16) | min(dbg_iters, 65535u);
            p.dbg[19 + 4 * w] = ((unsigned long long)(__smid() & 0xffffu) << 48) |
                                ((unsigned long long)min(DEEP ? dbg_walks : dbg_iters_dry, 65535u) << 32) | (uint32_t)t_wave0;
        }
    }
}

template <int V, int CULL, bool STATS, bool COUNT, bool PAIRS = false>
__global__ __launch_bounds__(256, (kMinWaves<V, CULL, STATS>)) void render_kernel(const KParams p)
{
    render_body<V, CULL, STATS, COUNT, false, 4, PAIRS>(p);
}
// the deep launch of a split pass (culled scenes only); WPB = 8: the lone deep launch with the
// shading records in LDS, whose workgroups per CU the LDS bounds
template <int V, bool STATS, bool COUNT, int WPB>
__global__ __launch_bounds__(64 * WPB, (WPB == 8 && !STATS ? RT_DEEP_WIDE_WAVES : kMinWaves<V, 7, STATS>)) void render_deep_kernel(const KParams p)
{
    render_body<V, 7, STATS, COUNT, true, WPB, false>(p);
}

// the redo launch of a pass with a ground kernel (culled scenes, single samples): the items of the
// pass's redo list through the unchanged loop
template <int V, bool STATS, bool COUNT>
__global__ __launch_bounds__(256, (kMinWaves<V, 7, STATS>)) void render_list_kernel(const KList k)
{
    if (k.redo.stat && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(k.redo.stat, min(k.redo.ctr[kRedoCount], k.redo.cap));
    render_body<V, 7, STATS, COUNT, false, 4, false, true>(k.p, k.redo);
}

// ---- launchers (called from rt_host.cpp) ---------------------------------------------
// cull: 0 = brute force (every sphere, index order), 7 = two-level cluster walk with
// transposed member tests (the default)
// COUNT: the instantiation that tallies segments and tests (when the caller passes counters)
// pairs: the pass stores sample pairs (culled scenes only)
template <int V, bool STATS, bool COUNT> static const void *ptr_cull(int cull, bool pairs)
{
    if (cull == 7) return pairs ? reinterpret_cast<const void *>(&render_kernel<V, 7, STATS, COUNT, true>)
                                : reinterpret_cast<const void *>(&render_kernel<V, 7, STATS, COUNT>);
    return pairs ? nullptr : reinterpret_cast<const void *>(&render_kernel<V, 0, STATS, COUNT>);
}

template <bool COUNT> static const void *render_ptr_c(int variant, int cull, bool pairs)
{
    switch (variant) {
    case V_EXACT_LDS: return ptr_cull<V_EXACT_LDS, false, COUNT>(cull, pairs);
    case V_FAST_LDS: return ptr_cull<V_FAST_LDS, false, COUNT>(cull, pairs);
    case V_EXACT_SCALAR:
        return cull || pairs ? nullptr : reinterpret_cast<const void *>(&render_kernel<V_EXACT_SCALAR, 0, false, COUNT>);
    case V_STATS_LDS: return ptr_cull<V_EXACT_LDS, true, true>(cull, pairs);
    default: return nullptr;
    }
}
static const void *render_ptr(int variant, int cull, bool count, bool pairs = false)
{
    return count ? render_ptr_c<true>(variant, cull, pairs) : render_ptr_c<false>(variant, cull, pairs);
}

template <bool COUNT, int WPB> static const void *render_deep_ptr_w(int variant)
{
    switch (variant) {
    case V_EXACT_LDS: return reinterpret_cast<const void *>(&render_deep_kernel<V_EXACT_LDS, false, COUNT, WPB>);
    case V_FAST_LDS: return reinterpret_cast<const void *>(&render_deep_kernel<V_FAST_LDS, false, COUNT, WPB>);
    case V_STATS_LDS: return reinterpret_cast<const void *>(&render_deep_kernel<V_EXACT_LDS, true, true, WPB>);
    default: return nullptr;
    }
}
static const void *render_deep_ptr(int variant, bool count, int wpb)
{
    if (wpb == 8) return count ? render_deep_ptr_w<true, 8>(variant) : render_deep_ptr_w<false, 8>(variant);
    if (wpb == 4) return count ? render_deep_ptr_w<true, 4>(variant) : render_deep_ptr_w<false, 4>(variant);
    return nullptr;
}

hipError_t launch_render(int variant, int cull, const KParams &p, uint32_t grid, hipStream_t stream, int wpb)
{
    // the deep launch (deep_mode != 0) exists for culled scenes only; only it has 8-wave groups
    const bool count = p.segments != nullptr;
    const void *fn = p.deep_mode ? (cull == 7 ? render_deep_ptr(variant, count, wpb) : nullptr)
                                 : (wpb == 4 ? render_ptr(variant, cull, count, p.n_pair_items != 0) : nullptr);
    if (!fn) return hipErrorInvalidValue;
    const size_t lds = (size_t)p.lds_units * 16u;
    void *args[] = {const_cast<KParams *>(&p)};
    return hipLaunchKernel(fn, dim3(grid), dim3(64u * (uint32_t)wpb), args, lds, stream);
}

template <bool COUNT> static const void *render_list_ptr(int variant)
{
    switch (variant) {
    case V_EXACT_LDS: return reinterpret_cast<const void *>(&render_list_kernel<V_EXACT_LDS, false, COUNT>);
    case V_FAST_LDS: return reinterpret_cast<const void *>(&render_list_kernel<V_FAST_LDS, false, COUNT>);
    case V_STATS_LDS: return reinterpret_cast<const void *>(&render_list_kernel<V_EXACT_LDS, true, true>);
    default: return nullptr;
    }
}
hipError_t launch_render_list(int variant, const KList &k, uint32_t grid, hipStream_t stream)
{
    const void *fn = k.p.segments ? render_list_ptr<true>(variant) : render_list_ptr<false>(variant);
    if (!fn) return hipErrorInvalidValue;
    void *args[] = {const_cast<KList *>(&k)};
    return hipLaunchKernel(fn, dim3(grid), dim3(256), args, (size_t)k.p.lds_units * 16u, stream);
}

// workgroups per CU and static LDS of the deep kernel with wpb waves per workgroup
hipError_t deep_occupancy(int variant, int wpb, size_t lds, int *blocks_per_cu, size_t *static_lds)
{
    const void *fn = render_deep_ptr(variant, false, wpb);
    if (!fn) return hipErrorInvalidValue;
    hipFuncAttributes a{};
    hipError_t e = hipFuncGetAttributes(&a, fn);
    if (e != hipSuccess) return e;
    *static_lds = a.sharedSizeBytes;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, fn, 64 * wpb, lds);
}

hipError_t occupancy_render(int variant, int cull, int *blocks_per_cu, size_t lds, bool pairs)
{
    const void *fn = render_ptr(variant, cull, false, pairs);
    if (!fn) return hipErrorInvalidValue;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, fn, 256, lds);
}

// the static LDS of a render kernel (per-wave and per-lane arrays; the scene blob comes on top)
hipError_t static_lds_render(int variant, int cull, size_t *bytes, bool pairs)
{
    const void *fn = render_ptr(variant, cull, false, pairs);
    if (!fn) return hipErrorInvalidValue;
    hipFuncAttributes a{};
    const hipError_t e = hipFuncGetAttributes(&a, fn);
    if (e == hipSuccess) *bytes = a.sharedSizeBytes;
    return e;
}

} // namespace rt
