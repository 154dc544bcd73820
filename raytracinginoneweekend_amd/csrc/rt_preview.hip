// rt_preview.hip — the two kernels of the preview session that are not a stage of their own
// (rt_preview_frame_device): preview_split turns a frame's beauty and variance
// into illumination and its variance before the temporal stage, preview_merge multiplies the
// filter's output by the albedo again and stores the frame as f32, as rgb8 or as both in one pass.
// A translation unit of its own: the render, feature-buffer, denoise and temporal kernels' machine
// code does not depend on it.
//
// One lane per pixel, 64 x 4 workgroups as temporal_accumulate: a wave covers 64 consecutive pixels
// of a row, so every load and store has unit stride over the lanes. No LDS, no scratch. Each pixel
// reads and writes its own position only. include/rt_api.h states the arithmetic; every operation
// below is a separate binary32 operation, in the contract's order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rt_device.h"
#include "rt_texel.h"

namespace rt {

// A' of RT_DENOISE_DEMODULATE
__device__ __forceinline__ float pv_floor(float a) { return fmaxf(a, 0.0078125f); }

__global__ __launch_bounds__(256) void preview_split(const KPreviewSplit k)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= (int)k.W || y >= (int)k.H) return;
    const size_t p = (size_t)y * k.W + x;
    const float ar = pv_floor(k.albedo[3u * p]), ag = pv_floor(k.albedo[3u * p + 1u]), ab = pv_floor(k.albedo[3u * p + 2u]);
    const float la = (0.2126f * ar + 0.7152f * ag) + 0.0722f * ab;
    k.illum[3u * p] = k.beauty[3u * p] / ar;
    k.illum[3u * p + 1u] = k.beauty[3u * p + 1u] / ag;
    k.illum[3u * p + 2u] = k.beauty[3u * p + 2u] / ab;
    k.var_out[p] = k.variance[p] / (la * la);
}

// DEMOD: the filter's output times A'(p); OUT_F32 / OUT_U8: which outputs are stored (the texel is
// formed from the value the f32 store holds)
template <bool DEMOD, bool OUT_F32, bool OUT_U8>
__global__ __launch_bounds__(256) void preview_merge(const KPreviewMerge k)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= (int)k.W || y >= (int)k.H) return;
    const size_t p = (size_t)y * k.W + x;
    float r = k.filtered[3u * p], g = k.filtered[3u * p + 1u], b = k.filtered[3u * p + 2u];
    if (DEMOD) {
        r = r * pv_floor(k.albedo[3u * p]);
        g = g * pv_floor(k.albedo[3u * p + 1u]);
        b = b * pv_floor(k.albedo[3u * p + 2u]);
    }
    if (OUT_F32) {
        k.out[3u * p] = r;
        k.out[3u * p + 1u] = g;
        k.out[3u * p + 2u] = b;
    }
    if (OUT_U8) {
        k.out_u8[3u * p] = rgb8_texel(r);
        k.out_u8[3u * p + 1u] = rgb8_texel(g);
        k.out_u8[3u * p + 2u] = rgb8_texel(b);
    }
}

hipError_t launch_preview_split(const KPreviewSplit &k, hipStream_t stream)
{
    void *args[] = {const_cast<KPreviewSplit *>(&k)};
    const dim3 grid((k.W + 63) / 64, (k.H + 3) / 4);
    return hipLaunchKernel(reinterpret_cast<const void *>(&preview_split), grid, dim3(64, 4), args, 0, stream);
}

// (at least one of k.out, k.out_u8 is given: the host checks it)
hipError_t launch_preview_merge(const KPreviewMerge &k, hipStream_t stream)
{
    static const void *const fn[2][3] = {
        {reinterpret_cast<const void *>(&preview_merge<false, true, false>),
         reinterpret_cast<const void *>(&preview_merge<false, false, true>),
         reinterpret_cast<const void *>(&preview_merge<false, true, true>)},
        {reinterpret_cast<const void *>(&preview_merge<true, true, false>),
         reinterpret_cast<const void *>(&preview_merge<true, false, true>),
         reinterpret_cast<const void *>(&preview_merge<true, true, true>)}};
    if (!k.out && !k.out_u8) return hipErrorInvalidValue;
    void *args[] = {const_cast<KPreviewMerge *>(&k)};
    const dim3 grid((k.W + 63) / 64, (k.H + 3) / 4);
    const int outs = (k.out ? 1 : 0) + (k.out_u8 ? 2 : 0) - 1;
    return hipLaunchKernel(fn[k.albedo ? 1 : 0][outs], grid, dim3(64, 4), args, 0, stream);
}

} // namespace rt
