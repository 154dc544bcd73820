// rt_sky.hip — the sky kernel and its launcher, a translation unit of its own over
// rt_trace.h's vector math, RNG and pixel enumeration.
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
    const FrameConsts &fc = p.fc;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;  // the sky pixel
    const bool live = t < p.n_pix;
    uint32_t px, rr;
    pixel_of(fc, p.pos0 + (live ? t : 0u), px, rr, p.block_perm);
    const uint32_t py = fc.row_offset + rr * fc.row_stride;
    const uint64_t inc_data = ((uint64_t)fc.inc_data_hi << 32) | fc.inc_data_lo;
    const uint64_t inc_cam = ((uint64_t)fc.inc_cam_hi << 32) | fc.inc_cam_lo;
    const uint64_t key0 = (uint64_t)(py * fc.W + px) * fc.spp;
    const uint32_t spp = fc.spp, full_end = spp & ~3u;
    float fW = fc.fW, fH = fc.fH, rW = fc.rW, rH = fc.rH, lens = fc.lens;
    const bool dw = fc.div_fast & 1u, dh = fc.div_fast & 2u;
    f3 org = mk(fc.org[0], fc.org[1], fc.org[2]), llc = mk(fc.llc[0], fc.llc[1], fc.llc[2]);
    f3 hor = mk(fc.hor[0], fc.hor[1], fc.hor[2]), ver = mk(fc.ver[0], fc.ver[1], fc.ver[2]);
    // (a VALU operation reading an SGPR issues at half rate, scripts/ubench_int.hip)
    if (RT_SKY_VCONST >= 1) asm volatile("" : "+v"(fW), "+v"(fH), "+v"(rW), "+v"(rH), "+v"(lens));
    if (RT_SKY_VCONST >= 2) {
        asm volatile("" : "+v"(org.x), "+v"(org.y), "+v"(org.z), "+v"(llc.x), "+v"(llc.y), "+v"(llc.z));
        asm volatile("" : "+v"(hor.x), "+v"(hor.y), "+v"(hor.z), "+v"(ver.x), "+v"(ver.y), "+v"(ver.z));
    }
    // acc: the running sum; pa: the block's c0, then c2; pb: c0 + c1
    f3 acc = mk(0.f, 0.f, 0.f), pa = acc, pb = acc;
    // Sample s's streams (main.cxx:192-200, key = (y W + x) spp + s): pcg_seed(key, inc) =
    // key M + inc (M + 1), and the data stream's second state M (key M + inc (M + 1)) + inc; both
    // are key M and key M^2 plus wave-uniform terms, and the key steps by 1 from sample to sample,
    // so the two products step by M and M^2 (mod 2^64, exact): no multiply per sample
    const uint64_t cd1 = inc_data * (kPcgMul + 1u), cd2 = cd1 * kPcgMul + inc_data, cc = inc_cam * (kPcgMul + 1u);
    const uint64_t mm = kPcgMul * kPcgMul;
    uint64_t km = key0 * kPcgMul, kmm = km * kPcgMul;
    const float ux = div_const((float)px, fW, rW, dw), vy = div_const((float)py, fH, rH, dh);
    // the draw side: sd, the sample whose lens point the lane is drawing (a dead lane has none to
    // draw, and counts as having every point waiting); rc, the camera stream's state; kc, key M
    // of the sample after sd. The LCG multiplier's halves and the 2^-31 scale sit in VGPRs, as in
    // random_in_unit_sphere_capped.
    uint32_t sd = live ? 0u : spp;
    uint64_t rc = km + cc, kc = km + kPcgMul;
    uint32_t m_lo = (uint32_t)kPcgMul, m_hi = (uint32_t)(kPcgMul >> 32);
    float k31 = 0x1p-31f;
    asm volatile("" : "+v"(m_lo), "+v"(m_hi), "+v"(k31));
    const uint64_t mul = ((uint64_t)m_hi << 32) | m_lo;
    auto draw = [&]() {
        const uint64_t old = rc;
        rc = old * mul + inc_cam;
        return fmaf(fminf((float)pcg_out(old), 0x1.fffffep31f), k31, -1.f);  // canonical_pm1
    };
    // the colour side: sc, the wave's colour sample (uniform); a wave without a live lane leaves
    const uint32_t n_s = ballot(live) ? spp : 0u;
    const uint32_t tid = threadIdx.x;
    for (uint32_t sc = 0; sc < n_s;) {
        if (ballot(sd == sc)) {
            // some lane has no point waiting (sd >= sc always): an attempt round, camera.hxx:52
            const uint32_t room_end = min(spp, sc + (uint32_t)RT_SKY_RING);
            if (sd < room_end) {
                const float x = draw();
                const float y = draw();
                const float z = draw();
                if (!(x * x + y * y + z * z > 0x1.000002p+0f)) {
                    ring[sd & (RT_SKY_RING - 1u)][tid] = make_float2(x, y);
                    ++sd;
                    rc = kc + cc;
                    kc += kPcgMul;
                }
            }
        }
        // (a second if, not an else: the draw side's registers are then updated in place, where
        // the else form copied sd, rc and kc on every attempt round, 9 moves)
        if (!ballot(sd == sc)) {
            // every lane holds sample sc's point: a colour round for the whole wave
            const float2 r = ring[sc & (RT_SKY_RING - 1u)][tid];
            const float xu = fminf((float)pcg_out(km + cd1), 0x1.fffffep31f) * 0x1p-32f;  // canonical()
            const float xv = fminf((float)pcg_out(kmm + cd2), 0x1.fffffep31f) * 0x1p-32f;
            const float uu = ux + div_const(xu, fW, rW, dw);
            const float vv = vy + div_const(xv, fH, rH, dh);
            km += kPcgMul;
            kmm += mm;
            const f3 rd = mk(r.x * lens, r.y * lens, 0.f);                      // camera.hxx:46-57
            const f3 off = mk(uu * rd.x, vv * rd.y, 0.f);
            f3 d = ((llc + hor * uu) + ver * (1.f - vv)) - off;
            if (fc.corrected) d = d - org;
            // unit_direction(d).y (math.hxx:219-227): with |d|^2 in [2^-40, 2^40] the short
            // sqrt and division give its bits (render_body's sky)
            const float a = d.x * d.x + d.y * d.y + d.z * d.z;
            float uy;
            if (!ballot(!(a >= 0x1p-40f && a <= 0x1p40f))) {
                const float l = sqrt_scaled(a);
                const float y0 = __builtin_amdgcn_rcpf(l);
                uy = div_ray(d.y, RayDiv{l, fmaf(fmaf(-l, y0, 1.f), y0, y0), 1u});
            } else {
                uy = normalize(d).y;
            }
            const float tt = .5f * uy + 1.f;                                    // main.cxx:71
            const f3 col = mk(1.f, 1.f, 1.f) * (1.f - tt) + mk(.5f, .7f, 1.f) * tt;
            // the blocked sum, on scalar branches: c0 and c2 wait in pa, c0 + c1 in pb, and the
            // block's (c0 + c1) + (c2 + c3), or a tail colour, folds into acc
            const uint32_t j = sc & 3u;
            if (sc >= full_end) {
                acc = acc + col;
            } else if (j == 1u) {
                pb = pa + col;
            } else if (j == 3u) {
                acc = acc + (pb + (pa + col));
            } else {
                pa = col;
            }
            ++sc;
        }
    }
    if (live) {
        float *o = p.sums + 3u * (size_t)t;
        o[0] = acc.x;
        o[1] = acc.y;
        o[2] = acc.z;
    }
    if (p.segments) {
        const uint32_t n = lanes(live);
        if ((threadIdx.x & 63u) == 0u && n) atomicAdd(p.segments, (unsigned long long)n * spp);
    }
}

hipError_t launch_sky(const KSky &k, hipStream_t stream)
{
    if (!k.n_pix) return hipSuccess;
    hipLaunchKernelGGL(sky_kernel, dim3((k.n_pix + 255u) / 256u), dim3(256), 0, stream, k);
    return hipGetLastError();
}

} // namespace rt
