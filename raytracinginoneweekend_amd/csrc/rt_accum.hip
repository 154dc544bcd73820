// rt_accum.hip — the accumulation kernels (accumulate_pixels<MOMENTS>, rt_accum.h) and the rgb8
// epilogue, with their launchers.
#include "rt_accum.h"
#include "rt_texel.h"

namespace rt {

// ---- ordered accumulation of the slots, average, optional gamma/u8 --------------------
__global__ __launch_bounds__(256) void accumulate_kernel(const KAccum k)
{
    accumulate_pixels<false>(k);
}

// the accumulation of a variance render (rt_render_var_device)
__global__ __launch_bounds__(256) void accumulate_moments_kernel(const KAccum k)
{
    accumulate_pixels<true>(k);
}

__global__ __launch_bounds__(256) void epilogue_rgb8_kernel(const float *in, uint8_t *out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = rgb8_texel(in[i]);
}

hipError_t launch_accumulate(const KAccum &k, hipStream_t stream)
{
    const uint32_t grid = (k.n_pixels + 255u) / 256u;
    if (k.var) {
        hipLaunchKernelGGL(accumulate_moments_kernel, dim3(grid), dim3(256), 0, stream, k);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(accumulate_kernel, dim3(grid), dim3(256), 0, stream, k);
    return hipGetLastError();
}

hipError_t launch_epilogue(const float *in, uint8_t *out, uint64_t n, hipStream_t stream)
{
    const uint64_t grid = (n + 255u) / 256u;
    hipLaunchKernelGGL(epilogue_rgb8_kernel, dim3((uint32_t)grid), dim3(256), 0, stream, in, out, n);
    return hipGetLastError();
}

} // namespace rt
