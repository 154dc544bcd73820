// rt_accum.h — the body of both accumulation kernels (rt_accum.hip): the ordered accumulation of
// the slots, the average, optional gamma/u8.
#pragma once
#include "rt_trace.h"

namespace rt {

// MOMENTS (rt_render_var_device; single-sample slots): from the same slot loads,
// in sample order, the shifted moments of the samples' luminance, carried between passes in
// k.mom[ni] = {L_0, m1, m2}; the last pass writes the variance of the mean to k.var. The sky
// positions of a plan with sky_moments_kernel (rt_sky.hip) are folded there: the
// last pass of a one-shot frame finds their sums at their sample-0 slots and {L_0, m1, m2} at their
// sample-1 slots.
// A template on MOMENTS: accumulate_kernel (false) and accumulate_moments_kernel (true).
//
// One sample's colour into the shifted moments, samples in order: its luminance L, d = L - L_0
// (frame_first: the frame's sample 0, L_0 = L and d = 0), m1 += d, m2 += d d. The one statement of
// this arithmetic, for accumulate_pixels<true> and sky_moments_kernel.
__device__ __forceinline__ void fold_luminance(const f3 &c, bool frame_first, float &l0, float &m1, float &m2)
{
    const float l = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;
    if (frame_first) l0 = l;
    const float d = l - l0;
    m1 = m1 + d;
    m2 = m2 + d * d;
}

template <bool MOMENTS>
__device__ __forceinline__ void accumulate_pixels(const KAccum &k)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && k.seg_to)
        for (int c = 0; c < 3; ++c) {
            k.seg_to[c] += k.seg_from[c];
            k.seg_from[c] = 0ull;
        }
    // the render that used this workspace has finished: reset its queue counters (no memset
    // kernel in front of the next render)
    if (k.queue_reset)
        for (uint32_t w = i; w < k.queue_words; w += gridDim.x * blockDim.x) {
            if (k.deep_over && (w & (kQueueStride - 1u)) == kDeepCount && k.queue_reset[w] > k.deep_rcap)
                *k.deep_over = k.deep_key;
            k.queue_reset[w] = 0u;
        }
    if (i >= k.n_pixels) return;
    // split passes (KAccum::part): 1 = pixels without deep samples, 2 = the others, 3 = all
    // pixels in one part; 2 and 3 clear the flags for the workspace's next pass
    // the sky kernel's pixels: their sums wait at their sample-0 slots for the
    // frame's last pass, after the sky kernel (not in part 1, which runs beside the deep launch)
    const bool sky = i >= k.sky_pos0;
    if (sky) {
        if (!k.last || k.part == 1) return;
    } else if (k.part) {
        const bool flagged = k.deep_px[i];
        if (k.part == 1 && flagged) return;
        if (k.part == 2 && !flagged) return;
        if (k.part != 1 && flagged) k.deep_px[i] = 0;
    }
    // i: the pixel's position in this pass's slots (its permuted enumeration);
    // ni: its natural enumeration index, which indexes the running sums (passes of one frame may
    // be dealt in different orders) and places the output
    const uint32_t ni = k.block_perm ? (k.block_perm[i >> 6] << 6) | (i & 63u) : i;
    f3 acc;
    float l0 = 0.f, m1 = 0.f, m2 = 0.f;  // MOMENTS: L_0 and the shifted sums
    (void)l0; (void)m1; (void)m2;
    if (sky) {
        acc = mk(k.slots[3 * i], k.slots[3 * i + 1], k.slots[3 * i + 2]);
        if (MOMENTS) {
            const float *m = k.slots + 3u * ((size_t)k.n_pixels + i);
            l0 = m[0], m1 = m[1], m2 = m[2];
        }
    } else if (k.first) acc = mk(0.f, 0.f, 0.f);
    else acc = mk(k.acc[3 * ni], k.acc[3 * ni + 1], k.acc[3 * ni + 2]);
    // main.cxx:205 = libstdc++ reduce (<numeric>:443-460): ((c0+c1)+(c2+c3)) per block of 4,
    // blocks in order, then the spp % 4 tail one by one. Passes start on a multiple of 4.
    auto ld = [&](uint32_t s) {
        const float *v = k.slots + ((size_t)s * k.n_pixels + i) * 3u;
        return mk(v[0], v[1], v[2]);
    };
    if (sky) {
        // (summed by sky_kernel over every sample of the frame)
    } else if (k.paired) {
        // pair sums: slot 2b holds c0+c1, slot 2b+1 c2+c3 of block b; then the tail's samples
        for (uint32_t b = 0; b < k.n_blocks; ++b) acc = acc + (ld(2u * b) + ld(2u * b + 1u));
        for (uint32_t t = 4u * k.n_blocks; t < k.n_samples; ++t) acc = acc + ld(t - 2u * k.n_blocks);
    } else if (MOMENTS) {
        if (!k.first) l0 = k.mom[3 * ni], m1 = k.mom[3 * ni + 1], m2 = k.mom[3 * ni + 2];
        auto fold = [&](const f3 &c, uint32_t t) { fold_luminance(c, k.first && t == 0u, l0, m1, m2); };  // sample t of the pass
        uint32_t s = 0;
        for (; s < 4u * k.n_blocks; s += 4u) {
            const f3 c0 = ld(s), c1 = ld(s + 1u), c2 = ld(s + 2u), c3 = ld(s + 3u);
            acc = acc + ((c0 + c1) + (c2 + c3));
            fold(c0, s);
            fold(c1, s + 1u);
            fold(c2, s + 2u);
            fold(c3, s + 3u);
        }
        for (; s < k.n_samples; ++s) {
            const f3 c = ld(s);
            acc = acc + c;
            fold(c, s);
        }
    } else {
        uint32_t s = 0;
        for (; s < 4u * k.n_blocks; s += 4u) acc = acc + ((ld(s) + ld(s + 1u)) + (ld(s + 2u) + ld(s + 3u)));
        for (; s < k.n_samples; ++s) acc = acc + ld(s);
    }
    if (!k.last) {
        k.acc[3 * ni] = acc.x; k.acc[3 * ni + 1] = acc.y; k.acc[3 * ni + 2] = acc.z;
        if (MOMENTS) k.mom[3 * ni] = l0, k.mom[3 * ni + 1] = m1, k.mom[3 * ni + 2] = m2;
        return;
    }
    const f3 col = acc / (float)k.spp;  // main.cxx:207
    // output position
    uint32_t x, rr;
    {
        const uint32_t tiled_px = k.tiled_rows * k.W;
        if (ni < tiled_px) {
            uint32_t t = ni >> 6, w = ni & 63u;
            uint32_t ty = t / k.tiles_x, tx = t - ty * k.tiles_x;
            x = (tx << k.tile_lw) + (w & ((1u << k.tile_lw) - 1u));
            rr = (ty << (6u - k.tile_lw)) + (w >> k.tile_lw);
        } else {
            uint32_t jj = ni - tiled_px;
            rr = jj / k.W;
            x = jj - rr * k.W;
            rr += k.tiled_rows;
        }
    }
    const uint32_t row = k.full_frame ? k.row_offset + rr * k.row_stride : rr;
    const size_t o = ((size_t)row * k.W + x) * 3u;
    k.out[o] = col.x; k.out[o + 1] = col.y; k.out[o + 2] = col.z;
    if (MOMENTS) {
        // the variance of the mean luminance: the unbiased sample variance over spp
        const float n = (float)k.spp, mean = m1 / n, ex2 = m2 / n;
        k.var[(size_t)row * k.W + x] = fmaxf(0.0f, ex2 - mean * mean) / (float)(k.spp - 1u);
        return;  // (no out_u8 in this path)
    }
    if (k.out_u8) {
        // main.cxx:39-45,77-85: pow(c, 1/2.2f) then (uint8)(255 * c); powf evaluated in double
        // and rounded once (glibc's powf agrees to the last bit except at rare ties).
        const double g = (double)(1.f / 2.2f);
        k.out_u8[o] = (uint8_t)(255.f * (float)pow((double)col.x, g));
        k.out_u8[o + 1] = (uint8_t)(255.f * (float)pow((double)col.y, g));
        k.out_u8[o + 2] = (uint8_t)(255.f * (float)pow((double)col.z, g));
    }
}

} // namespace rt
