// rt_sky.hip — the sky kernel, its moments form (§4.21) and their launchers, a
// translation unit of its own over rt_trace.h's vector math, RNG and pixel enumeration.
#include "rt_accum.h"
#include "rt_trace.h"

namespace rt {

// ---- the sky kernel -----------------------------------------------------
// The pixels of the tiles proven to send every primary ray to the sky: each sample is the
// reference's primary ray (main.cxx:192-200, camera.hxx:46-57) and its colour the sky's
// (main.cxx:71: background(.5 unit_direction(d).y + 1) times an attenuation of 1, exact), the
// closest hit being proven empty. One thread per pixel, its samples in order, summed in the
// blocked order of main.cxx:205's std::reduce: ((c0 + c1) + (c2 + c3)) per block of 4, added to
// the running sum block after block, then the tail samples one by one; accumulate_kernel divides
// by spp. (4 threads per pixel with an LDS combine, so that the kernel's last waves end sooner,
// were not faster: profiles/r06/ab/sky_parts.txt, deep_sky_tail.txt; the kernel is
// throughput-bound on what the main launch leaves it.)
// The loop has two decoupled sides. The lens draws come from the camera stream alone (seeded per
// sample by addition), so a lane draws ahead of its colours: an attempt round is one attempt of
// raytracer.hxx:32-43 for every lane with samples left to draw and room in its ring, and an
// accepted point's (x, y) is pushed to the lane's ring in LDS (z only decides acceptance). The
// colour side is wave-synchronous: its sample index sc is the same for every lane of the wave,
// and a colour round (the sample's start, its ray and colour, its place in the blocked sum) runs
// only when every lane has a point waiting, so it never runs for a part of the wave, and the
// block position sc & 3 and the tail test are scalar. A lane without a point has room, so the
// wave always has one of the two rounds to run. Same draws per stream, same order, same bits;
// only when an operation executes differs from a loop that finishes sample after sample.
// The ring: RT_SKY_RING accepted points per lane, laid out [slot][thread] (a wave's 8-byte
// accesses are consecutive); slots are cursor & (RT_SKY_RING - 1), so every index is in the array
// whatever the cursors hold (§4.6).
//
// MOMENTS (sky_moments_kernel; rt_options.sky_moments = 1): the same pixels for a
// frame that carries per-pixel moments, samples [s_a, s_b) of the frame's fc.spp (s_a a multiple of
// 4, s_b one or fc.spp: a whole one-shot frame, or a session's window). Draws and colours are the
// same operations: sample s's streams are those of key (y W + x) spp + s, so the stepping constants
// start at key0 + s_a, and both sides of the ring index it by the frame's sample number, so a start
// that is no multiple of the ring's depth changes nothing. The sum takes the frame's block
// positions (s & 3, the tail from spp & ~3) and starts from the carried sum when s_a > 0; each
// colour is folded into the shifted moments of the luminance as accumulate_pixels<true> folds it
// (fold_luminance, rt_accum.h), in sample order, {L_0, m1, m2} carried beside the sum. The body
// is shared (rt_sky_body.h, included by both kernels); sky_kernel is the one without any of this.
#ifndef RT_SKY_RING
#define RT_SKY_RING 8
#endif
#ifndef RT_SKY_VCONST
#define RT_SKY_VCONST 0  // A/B build switch: camera constants held in VGPRs (1: the divisors and the lens, 2: all)
#endif
static_assert(RT_SKY_RING >= 2 && (RT_SKY_RING & (RT_SKY_RING - 1)) == 0, "ring depth: a power of two");

__global__ __launch_bounds__(256) void sky_kernel(const KSky p)
{
    __shared__ float2 ring[RT_SKY_RING][256];
    constexpr bool MOMENTS = false;
    const KSkyMoments *const q = nullptr;
#include "rt_sky_body.h"
}

__global__ __launch_bounds__(256) void sky_moments_kernel(const KSkyMoments k)
{
    __shared__ float2 ring[RT_SKY_RING][256];
    constexpr bool MOMENTS = true;
    const KSky &p = k.sky;
    const KSkyMoments *const q = &k;
#include "rt_sky_body.h"
}

hipError_t launch_sky(const KSky &k, hipStream_t stream)
{
    if (!k.n_pix) return hipSuccess;
    hipLaunchKernelGGL(sky_kernel, dim3((k.n_pix + 255u) / 256u), dim3(256), 0, stream, k);
    return hipGetLastError();
}

hipError_t launch_sky_moments(const KSkyMoments &k, hipStream_t stream)
{
    if (!k.sky.n_pix || k.s_a >= k.s_b) return hipSuccess;
    hipLaunchKernelGGL(sky_moments_kernel, dim3((k.sky.n_pix + 255u) / 256u), dim3(256), 0, stream, k);
    return hipGetLastError();
}

} // namespace rt
