// rt_aov.hip — first-hit feature buffers (rt_render_aov_device): per pixel the
// albedo, normal, depth and coverage of its samples' primary hits and the sphere of sample 0,
// for a denoiser or compositor. A translation unit of its own, as every kernel family is; the device
// functions are rt_trace.h's.
//
// Sample s of a pixel is the beauty render's sample s (main.cxx:192-200): the same streams, the
// same jitter and lens draws, camera::ray (camera.hxx:46-57) and hit_world (raytracer.hxx:94-118)
// through closest_hit. Its values:
//   albedo  the hit sphere's material albedo; on a miss the sky's colour, main.cxx:71 with an
//           attenuation of 1 (what the beauty's sample is then)
//   normal  (p - c) / r, raytracer.hxx:71; (0, 0, 0) on a miss
//   depth   hit.time (in units of the un-normalised direction); 0 on a miss
//   alpha   1 on a hit, 0 on a miss
// and a pixel's value of each is the samples' blocked sum of main.cxx:205 (libstdc++ reduce:
// ((c0 + c1) + (c2 + c3)) per block of 4 added to the running sum, then the tail one by one)
// divided by float(samples).
#include "rt_trace.h"

namespace rt {

// the eight float channels of a sample: albedo rgb, normal xyz, depth, alpha
struct Aov8 { float v[8]; };
__device__ __forceinline__ Aov8 operator+(const Aov8 &a, const Aov8 &b)
{
    Aov8 r;
#pragma unroll
    for (int c = 0; c < 8; ++c) r.v[c] = a.v[c] + b.v[c];
    return r;
}

// One wave per 64-pixel block of the pass's enumeration (grid-stride over the blocks), one lane
// per pixel; every lane of the wave is at the same sample, so closest_hit runs once per sample
// for the whole wave and the blocked sum's control flow is wave-uniform. The lanes past the end
// of a partial last block repeat the block's first pixel and store nothing.
template <int CULL>
__global__ __launch_bounds__(256) void aov_kernel(const KAov p)
{
    extern __shared__ float4 lds_blob[];
    for (uint32_t i = threadIdx.x; i < p.lds_units; i += blockDim.x) lds_blob[i] = p.blob[i];
    __syncthreads();
    const float4 *blob = lds_blob;
    const float4 *geo = blob;
    const uint32_t *sidx = reinterpret_cast<const uint32_t *>(blob + p.n_geo);
    const float4 *clus = blob + p.clus_offset;
    __shared__ TransposeLds s_tw[4];
    TransposeLds *tw = &s_tw[threadIdx.x >> 6];
    const FrameConsts &fc = p.fc;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t n_waves = gridDim.x * 4u;
    const uint64_t inc_data = ((uint64_t)fc.inc_data_hi << 32) | fc.inc_data_lo;
    const uint64_t inc_cam = ((uint64_t)fc.inc_cam_hi << 32) | fc.inc_cam_lo;
    // pcg_seed(key, inc) = key M + inc (M + 1), as render_kernel
    const uint64_t cd = inc_data * (kPcgMul + 1u), cc = inc_cam * (kPcgMul + 1u);
    const float fW = fc.fW, fH = fc.fH, rW = fc.rW, rH = fc.rH;
    const bool dw = fc.div_fast & 1u, dh = fc.div_fast & 2u;
    const f3 org = mk(fc.org[0], fc.org[1], fc.org[2]), llc = mk(fc.llc[0], fc.llc[1], fc.llc[2]);
    const f3 hor = mk(fc.hor[0], fc.hor[1], fc.hor[2]), ver = mk(fc.ver[0], fc.ver[1], fc.ver[2]);
    const uint32_t samples = p.samples, full_end = samples & ~3u;
    WaveTally<false> wt;
    Dbg dbg{};
    for (uint32_t b = wave0; b < p.n_blocks; b += n_waves) {
        const uint32_t i = 64u * b + lane;
        const bool live = i < fc.n_pixels;
        const uint64_t lm = ballot(live);
        // blocks from sky_block0 on: every primary ray proven to meet no sphere
        const bool sky = b >= p.sky_block0;
        uint32_t px, rr;
        pixel_of(fc, live ? i : 64u * b, px, rr, p.block_perm);
        const uint32_t py = fc.row_offset + rr * fc.row_stride;
        // key = (y W + x) spp + s with the frame's spp: the beauty's first `samples` samples
        const uint64_t key0 = (uint64_t)(py * fc.W + px) * fc.spp;
        const float ux = div_const((float)px, fW, rW, dw), vy = div_const((float)py, fH, rH, dh);
        // the running sum, the block's current pair (c0 or c2) and its first pair sum c0 + c1
        Aov8 acc, pa, pb;
#pragma unroll
        for (int c = 0; c < 8; ++c) acc.v[c] = pa.v[c] = pb.v[c] = 0.f;
        uint32_t id0 = 0xffffffffu;
        for (uint32_t s = 0; s < samples; ++s) {
            // the sample's start, main.cxx:192-200 (as wave_gen_kernel)
            const uint64_t km = (key0 + s) * kPcgMul;
            uint64_t rng = km + cd, rc = km + cc;
            const float uu = ux + div_const(canonical(rng, inc_data), fW, rW, dw);
            const float vv = vy + div_const(canonical(rng, inc_data), fH, rH, dh);
            const f3 r = random_in_unit_sphere(rc, inc_cam);  // camera.hxx:52
            const f3 rl = r * fc.lens;                        // camera.hxx:46-57
            const f3 off = mk(uu * rl.x, vv * rl.y, 0.f);
            const f3 o = org + off;
            f3 d = ((llc + hor * uu) + ver * (1.f - vv)) - off;
            if (fc.corrected) d = d - org;
            const float a = d.x * d.x + d.y * d.y + d.z * d.z;
            const RayDiv rd = ray_div(a, lm, p.fast_roots);
            Hit h{kNoHit};
            if (!sky)
                h = closest_hit<false, CULL, false, false>(p, geo, sidx, clus, o, d, rd, dbg, wt, live, lm,
                                                           CULL ? tw : nullptr, no_hit());
            if (!live) h = Hit{kNoHit};
            const uint32_t ib = h.id();
            Aov8 v;
            if (ib == 0xffffffffu) {
                // main.cxx:71: background(.5 unit_direction(d).y + 1), the short forms as render_kernel's sky
                float uy;
                if (rd.fd != 0u) {
                    const float l = sqrt_scaled(a);
                    const float y0 = __builtin_amdgcn_rcpf(l);
                    uy = div_ray(d.y, RayDiv{l, fmaf(fmaf(-l, y0, 1.f), y0, y0), 1u});
                } else {
                    uy = normalize(d).y;
                }
                const float tt = .5f * uy + 1.f;
                const f3 bg = mk(1.f, 1.f, 1.f) * (1.f - tt) + mk(.5f, .7f, 1.f) * tt;
                v = Aov8{{bg.x, bg.y, bg.z, 0.f, 0.f, 0.f, 0.f, 0.f}};
            } else {
                // the hit's shading record, point and normal as render_kernel forms them
                float4 sf, md;
                if (p.shade_lds) {
                    const float4 *shade = blob + p.shade_offset;
                    sf = shade[2 * ib];
                    md = shade[2 * ib + 1];
                    asm volatile("");  // keeps the LDS and global loads apart
                } else {
                    const float4 *shade = p.blob + p.shade_offset;
                    sf = gld4(shade, 2 * ib);
                    md = gld4(shade, 2 * ib + 1);
                }
                const float t = h.t();
                const f3 hp = o + d * t;                       // ray::point_at, math.hxx:353
                const f3 dv = hp - mk(sf.x, sf.y, sf.z);
                f3 hn;
                if (p.fast_roots && all_lanes_min_abs_ok(dv)) hn = div3_short(dv, sf.w);
                else hn = dv / sf.w;                           // raytracer.hxx:71
                v = Aov8{{md.x, md.y, md.z, hn.x, hn.y, hn.z, t, 1.f}};
            }
            if (s == 0u) id0 = ib;
            // main.cxx:205's blocked sum; s is wave-uniform
            const uint32_t j = s & 3u;
            if (s >= full_end) acc = acc + v;
            else if (j == 0u || j == 2u) pa = v;
            else if (j == 1u) pb = pa + v;
            else acc = acc + (pb + (pa + v));
        }
        if (live) {
            const float n = (float)samples;
            const uint32_t row = p.full_frame ? py : rr;
            const size_t at = (size_t)row * fc.W + px;
            if (p.albedo) {
                p.albedo[3u * at] = acc.v[0] / n;
                p.albedo[3u * at + 1u] = acc.v[1] / n;
                p.albedo[3u * at + 2u] = acc.v[2] / n;
            }
            if (p.normal) {
                p.normal[3u * at] = acc.v[3] / n;
                p.normal[3u * at + 1u] = acc.v[4] / n;
                p.normal[3u * at + 2u] = acc.v[5] / n;
            }
            if (p.depth) p.depth[at] = acc.v[6] / n;
            if (p.alpha) p.alpha[at] = acc.v[7] / n;
            if (p.sphere_id) p.sphere_id[at] = id0;
        }
    }
}

static const void *aov_ptr(int cull)
{
    return cull == 7 ? reinterpret_cast<const void *>(&aov_kernel<7>) : reinterpret_cast<const void *>(&aov_kernel<0>);
}

hipError_t launch_aov(int cull, const KAov &k, uint32_t grid, hipStream_t stream)
{
    const size_t lds = (size_t)k.lds_units * 16u;
    void *args[] = {const_cast<KAov *>(&k)};
    return hipLaunchKernel(aov_ptr(cull), dim3(grid), dim3(256), args, lds, stream);
}

hipError_t occupancy_aov(int cull, int *blocks_per_cu, size_t lds)
{
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, aov_ptr(cull), 256, lds);
}

// the kernel's static LDS (the transposed tests' per-wave records; the scene blob comes on top)
hipError_t static_lds_aov(int cull, size_t *bytes)
{
    hipFuncAttributes a{};
    const hipError_t e = hipFuncGetAttributes(&a, aov_ptr(cull));
    if (e == hipSuccess) *bytes = a.sharedSizeBytes;
    return e;
}

} // namespace rt
