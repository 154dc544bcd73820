// rt_moments.hip — the accumulation of a variance render (rt_render_var_device):
// the MOMENTS instantiation of rt_kernel.hip's accumulate_pixels. A translation unit of its own, as
// rt_aov.hip is, so that the code object of the render kernels keeps its layout: their machine code
// and kernel descriptors (bench.kernel_sha256) do not change with it.
#define RT_DEVICE_FUNCTIONS_ONLY 1
#include "rt_kernel.hip"

namespace rt {

__global__ __launch_bounds__(256) void accumulate_moments_kernel(const KAccum k)
{
    accumulate_pixels<true>(k);
}

hipError_t launch_accumulate_moments(const KAccum &k, uint32_t grid, hipStream_t stream)
{
    hipLaunchKernelGGL(accumulate_moments_kernel, dim3(grid), dim3(256), 0, stream, k);
    return hipGetLastError();
}

} // namespace rt
