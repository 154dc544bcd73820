// rt_progressive.hip — the one kernel of a progressive session (rt_progressive_step_device,
// DESIGN.md §4.19): progressive_resolve turns the session's carried planes, the running sums `acc`
// and the luminance moments {L_0, m1, m2} after `done` samples of the frame, into the estimate the
// frame's own last accumulation would store if the frame ended there: the mean, the variance of
// the mean luminance, the texels, and the number of pixels still noisier than a threshold.
// A translation unit of its own: no other kernel's machine code depends on it, and the accumulation
// kernels (rt_accum.hip), which fold every window into the planes, stay as they are.
//
// One lane per pixel of the natural enumeration, 256-lane workgroups as accumulate_pixels: the
// loads of acc and mom have unit stride over the lanes (12 B per lane each), the stores go where
// accumulate_pixels puts a frame's (an 8 x 8 tile per wave over the tiled rows). No scratch and no
// LDS: the noise count is reduced per wave by a ballot and its population count, one atomic add per
// wave. include/rt_api.h states the arithmetic; every operation below is a separate binary32
// operation, in the contract's order (with done == spp they are accumulate_pixels' last-pass ones).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rt_device.h"
#include "rt_texel.h"

namespace rt {

// OUT_F32 / OUT_VAR / OUT_U8: which planes are stored; COUNT: the noise count is wanted
template <bool OUT_F32, bool OUT_VAR, bool OUT_U8, bool COUNT>
__global__ __launch_bounds__(256) void progressive_resolve(const KResolve k)
{
    const uint32_t ni = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = ni < k.n_pixels;  // (no early return: the ballot below takes whole waves)
    bool noisy = false;
    if (live) {
        const float nf = (float)k.done;
        const size_t s3 = (size_t)3u * ni;  // (n_pixels reaches 2^31: 3 ni does not fit 32 bits)
        const float r = k.acc[s3] / nf, g = k.acc[s3 + 1u] / nf, b = k.acc[s3 + 2u] / nf;
        float var = 0.f;
        if (OUT_VAR || COUNT) {
            const float mean = k.mom[s3 + 1u] / nf, ex2 = k.mom[s3 + 2u] / nf;
            var = fmaxf(0.0f, ex2 - mean * mean) / (float)(k.done - 1u);
        }
        if (COUNT) {
            const float l = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
            noisy = var > k.t2 * (l * l);
        }
        if (OUT_F32 || OUT_VAR || OUT_U8) {
            // output position (accumulate_pixels)
            uint32_t x, rr;
            const uint32_t tiled_px = k.tiled_rows * k.W;
            if (ni < tiled_px) {
                const uint32_t t = ni >> 6, w = ni & 63u;
                const uint32_t ty = t / k.tiles_x, tx = t - ty * k.tiles_x;
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
                k.out[3u * p + 2u] = b;
            }
            if (OUT_VAR) k.var[p] = var;
            if (OUT_U8) {
                k.out_u8[3u * p] = rgb8_texel(r);
                k.out_u8[3u * p + 1u] = rgb8_texel(g);
                k.out_u8[3u * p + 2u] = rgb8_texel(b);
            }
        }
    }
    if (COUNT) {
        // an integer sum: its order does not matter
        const unsigned long long m = __ballot(noisy);
        if ((threadIdx.x & 63u) == 0u && m) atomicAdd(k.noisy, (uint32_t)__popcll(m));
    }
}

// (at least one of k.out, k.var, k.out_u8, k.noisy is given: the host checks it)
hipError_t launch_progressive_resolve(const KResolve &k, hipStream_t stream)
{
#define RT_RESOLVE(a, b, c, d) reinterpret_cast<const void *>(&progressive_resolve<a, b, c, d>)
    static const void *const fn[16] = {
        nullptr,                                 RT_RESOLVE(true, false, false, false),
        RT_RESOLVE(false, true, false, false),   RT_RESOLVE(true, true, false, false),
        RT_RESOLVE(false, false, true, false),   RT_RESOLVE(true, false, true, false),
        RT_RESOLVE(false, true, true, false),    RT_RESOLVE(true, true, true, false),
        RT_RESOLVE(false, false, false, true),   RT_RESOLVE(true, false, false, true),
        RT_RESOLVE(false, true, false, true),    RT_RESOLVE(true, true, false, true),
        RT_RESOLVE(false, false, true, true),    RT_RESOLVE(true, false, true, true),
        RT_RESOLVE(false, true, true, true),     RT_RESOLVE(true, true, true, true)};
#undef RT_RESOLVE
    const int which = (k.out ? 1 : 0) | (k.var ? 2 : 0) | (k.out_u8 ? 4 : 0) | (k.noisy ? 8 : 0);
    if (!which || k.done < 2u || !k.n_pixels) return hipErrorInvalidValue;
    void *args[] = {const_cast<KResolve *>(&k)};
    return hipLaunchKernel(fn[which], dim3((k.n_pixels + 255u) / 256u), dim3(256), args, 0, stream);
}

} // namespace rt
