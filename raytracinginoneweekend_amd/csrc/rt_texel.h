// rt_texel.h — the gamma/u8 texel of a linear f32 value, shared by the kernels that store rgb8:
// epilogue_rgb8_kernel (rt_accum.hip, rt_epilogue_rgb8_device) and preview_merge (rt_preview.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rt {

// main.cxx:39-45,77-85: std::pow(c, 1 / 2.2f) in double, narrowed, then (uint8)(255 c)
__device__ __forceinline__ uint8_t rgb8_texel(float c)
{
    const double g = (double)(1.f / 2.2f);
    return (uint8_t)(255.f * (float)pow((double)c, g));
}

} // namespace rt
