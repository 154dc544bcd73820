// rt_adaptive.hip — the two kernels of an adaptive session (rt_adaptive_step_device).
// adaptive_resolve is progressive_resolve with a sample count per 64-pixel block: every block's
// estimate after the d_b samples folded into it, the block's number of noisy pixels, and the retire
// rule for the blocks that are still active. compact_blocks restricts a dealing order to the blocks
// whose flag is still set, which is the next window's block list. A translation unit of its own: no
// other kernel's machine code depends on it, and the render and accumulation kernels stay as they
// are (a window over a block list is a pass with fewer positions, rt_host.cpp).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rt_device.h"
#include "rt_texel.h"

namespace rt {

// One wave per natural 64-pixel block (the session's pixel count is a multiple of 64: every wave is
// whole), four waves per workgroup as progressive_resolve. The block's number is the same in every
// lane and formed through readfirstlane, and the two words read with it (the block's flag and its
// sample count) are read before anything is stored: they come in as scalar loads. No LDS, no
// scratch. Every operation is a separate binary32 operation in the contract's order
// (include/rt_api.h): with d = done in every block these are progressive_resolve's bits.
// OUT_F32 / OUT_VAR / OUT_U8 / OUT_SAMPLES: which planes are stored.
template <bool OUT_F32, bool OUT_VAR, bool OUT_U8, bool OUT_SAMPLES>
__global__ __launch_bounds__(256) void adaptive_resolve(const KAdaptive k)
{
    const uint32_t ni = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t b = __builtin_amdgcn_readfirstlane(ni >> 6);
    if (b >= k.n_blocks) return;  // (a whole wave)
    const uint32_t act = k.active[b];
    const uint32_t d = act ? k.done : k.d_b[b];  // an active block holds every sample rendered so far

    const float nf = (float)d;
    const size_t s3 = (size_t)3u * ni;
    const float r = k.acc[s3] / nf, g = k.acc[s3 + 1u] / nf, bl = k.acc[s3 + 2u] / nf;
    const float mean = k.mom[s3 + 1u] / nf, ex2 = k.mom[s3 + 2u] / nf;
    const float var = fmaxf(0.0f, ex2 - mean * mean) / (float)(d - 1u);
    const float l = (0.2126f * r + 0.7152f * g) + 0.0722f * bl;
    const bool noisy = var > k.t2 * (l * l);

    if (OUT_F32 || OUT_VAR || OUT_U8 || OUT_SAMPLES) {
        // output position (accumulate_pixels)
        uint32_t x, rr;
        const uint32_t tiled_px = k.tiled_rows * k.W;
        if (ni < tiled_px) {
            const uint32_t w = ni & 63u;
            const uint32_t ty = b / k.tiles_x, tx = b - ty * k.tiles_x;
            x = (tx << k.tile_lw) + (w & ((1u << k.tile_lw) - 1u));
            rr = (ty << (6u - k.tile_lw)) + (w >> k.tile_lw);
        } else {
            const uint32_t jj = ni - tiled_px;
            rr = jj / k.W;
            x = jj - rr * k.W;
            rr += k.tiled_rows;
        }
        const uint32_t row = k.full_frame ? k.row_offset + rr * k.row_stride : rr;
        const size_t p = (size_t)row * k.W + x;
        if (OUT_F32) {
            k.out[3u * p] = r;
            k.out[3u * p + 1u] = g;
            k.out[3u * p + 2u] = bl;
        }
        if (OUT_VAR) k.var[p] = var;
        if (OUT_SAMPLES) k.samples[p] = d;
        if (OUT_U8) {
            k.out_u8[3u * p] = rgb8_texel(r);
            k.out_u8[3u * p + 1u] = rgb8_texel(g);
            k.out_u8[3u * p + 2u] = rgb8_texel(bl);
        }
    }
    // c_b: the block's noisy pixels. Lane 0 alone writes the block's words (vector stores).
    const uint32_t c = (uint32_t)__popcll(__ballot(noisy));
    if ((threadIdx.x & 63u) == 0u) {
        if (act) {
            k.d_b[b] = d;
            k.active[b] = (d >= k.min_samples && c <= k.max_noisy) ? 0u : 1u;
        }
        if (k.noisy && c) atomicAdd(k.noisy, c);  // an integer sum: its order does not matter
    }
}

hipError_t launch_adaptive_resolve(const KAdaptive &k, hipStream_t stream)
{
#define RT_ARESOLVE(a, b, c, d) reinterpret_cast<const void *>(&adaptive_resolve<a, b, c, d>)
    static const void *const fn[16] = {
        RT_ARESOLVE(false, false, false, false), RT_ARESOLVE(true, false, false, false),
        RT_ARESOLVE(false, true, false, false),  RT_ARESOLVE(true, true, false, false),
        RT_ARESOLVE(false, false, true, false),  RT_ARESOLVE(true, false, true, false),
        RT_ARESOLVE(false, true, true, false),   RT_ARESOLVE(true, true, true, false),
        RT_ARESOLVE(false, false, false, true),  RT_ARESOLVE(true, false, false, true),
        RT_ARESOLVE(false, true, false, true),   RT_ARESOLVE(true, true, false, true),
        RT_ARESOLVE(false, false, true, true),   RT_ARESOLVE(true, false, true, true),
        RT_ARESOLVE(false, true, true, true),    RT_ARESOLVE(true, true, true, true)};
#undef RT_ARESOLVE
    const int which = (k.out ? 1 : 0) | (k.var ? 2 : 0) | (k.out_u8 ? 4 : 0) | (k.samples ? 8 : 0);
    if (k.done < 2u || !k.n_blocks || !k.acc || !k.mom || !k.d_b || !k.active) return hipErrorInvalidValue;
    void *args[] = {const_cast<KAdaptive *>(&k)};
    return hipLaunchKernel(fn[which], dim3((k.n_blocks + 3u) / 4u), dim3(256), args, 0, stream);
}

// The stable compaction of a dealing order by a flag per natural block: out = the entries of src
// whose block's flag is set, in src's order; counts = {kept, kept of src's first n0 entries, of its
// next n1, of the rest}, so the lead / other / sky structure of src carries over. One workgroup of
// 16 waves walks src in chunks of 1024, once: a kept entry goes to the entries kept before the
// chunk + those kept by the chunk's earlier waves (LDS) + those kept by the wave's earlier lanes
// (ballot and mbcnt). Kept entries only move towards the front, so out is complete after one walk.
// src null: the identity (entry i is block i); active null: every entry is kept (a copy).
// An entry that names no block (>= n_nat) is dropped, not looked up.
constexpr uint32_t kCompactLanes = 1024, kCompactWaves = kCompactLanes / 64;

__global__ __launch_bounds__(kCompactLanes) void compact_blocks_kernel(const KCompact k)
{
    __shared__ uint32_t wsum[2][kCompactWaves];
    __shared__ uint32_t wcls[3][kCompactWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t c1 = k.n0 + k.n1;  // entries [0, n0) are class 0, [n0, c1) class 1, [c1, n) class 2

    uint32_t run = 0;               // entries kept before this chunk (the same in every lane)
    uint32_t w0 = 0, w1 = 0, w2 = 0;  // this wave's kept entries of each class
    uint32_t buf = 0;
    for (uint32_t base = 0; base < k.n; base += kCompactLanes, buf ^= 1u) {
        const uint32_t i = base + threadIdx.x;
        uint32_t blk = 0;
        bool keep = false;
        if (i < k.n) {
            blk = k.src ? k.src[i] : i;
            keep = blk < k.n_nat && (!k.active || k.active[blk] != 0u);
        }
        const unsigned long long m = __ballot(keep);
        const uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
        w0 += (uint32_t)__popcll(__ballot(keep && i < k.n0));
        w1 += (uint32_t)__popcll(__ballot(keep && i >= k.n0 && i < c1));
        w2 += (uint32_t)__popcll(__ballot(keep && i >= c1));
        if (lane == 0) wsum[buf][wave] = (uint32_t)__popcll(m);
        // (one barrier per chunk: the chunk after the next writes this buffer again, and a wave
        // gets there only through the next chunk's barrier, after every wave has read this one)
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < kCompactWaves; ++w) {
            const uint32_t v = wsum[buf][w];
            before += w < wave ? v : 0u;
            total += v;
        }
        // (at <= i < n: an entry never moves towards the back)
        const uint32_t at = run + before + __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
        if (keep && at < k.n) k.out[at] = blk;
        run += total;
    }
    if (lane == 0) {
        wcls[0][wave] = w0;
        wcls[1][wave] = w1;
        wcls[2][wave] = w2;
    }
    __syncthreads();
    if (threadIdx.x < 4u) {
        // lanes 1..3: a class each; lane 0: their sum
        uint32_t s = 0;
        for (uint32_t q = 0; q < 3u; ++q)
            if (threadIdx.x == 0u || threadIdx.x == q + 1u)
                for (uint32_t w = 0; w < kCompactWaves; ++w) s += wcls[q][w];
        k.counts[threadIdx.x] = s;
    }
}

hipError_t launch_compact_blocks(const KCompact &k, hipStream_t stream)
{
    if (!k.out || !k.counts || k.n > k.n_nat || static_cast<uint64_t>(k.n0) + k.n1 > k.n) return hipErrorInvalidValue;
    void *args[] = {const_cast<KCompact *>(&k)};
    return hipLaunchKernel(reinterpret_cast<const void *>(&compact_blocks_kernel), dim3(1), dim3(kCompactLanes), args, 0, stream);
}

} // namespace rt
