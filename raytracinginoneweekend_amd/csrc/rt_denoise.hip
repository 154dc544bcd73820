// rt_denoise.hip — the edge-avoiding à-trous denoiser over the first-hit feature buffers
// (rt_denoise_device; Dammertz et al. 2010 with a polynomial edge function). A
// translation unit of its own: the render and feature-buffer kernels' machine code does not depend
// on it.
//
// One launch filters one level: 25 taps of the 5x5 B3 spline at spacing `step`, each weighted by
// the edge functions of the terms that are on (include/rt_api.h states the arithmetic; every
// operation below is a separate binary32 operation, in the contract's order). Two kernels with the
// same arithmetic per pixel, hence the same bits:
//   denoise_direct  one lane per pixel, the taps read from global memory
//   denoise_tiled   the workgroup's 32 x 16 tile and its halo of 2 step pixels staged once into
//                   LDS (the colour demodulated on load), the taps read from LDS
// The terms that are off are compiled out (TERMS), as is the demodulation of the input (DEMOD_IN).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

#include "rt_device.h"

namespace rt {

enum : int { kDnColor = 1, kDnNormal = 2, kDnDepth = 4, kDnAlbedo = 8 };

constexpr float kDnAlbedoFloor = 0.0078125f;  // A' = max(albedo, 2^-7)
constexpr int kDnTileW = 32, kDnTileH = 16;    // the tiled kernel's tile: 256 lanes, 2 pixels each

__device__ __forceinline__ float dn_edge(float d2, float r)
{
    const float m = fmaxf(0.0f, 1.0f - d2 * r);
    return m * m;
}

__device__ __forceinline__ float dn_dist2(float ar, float ag, float ab, float br, float bg, float bb)
{
    const float dr = ar - br, dg = ag - bg, db = ab - bb;
    return (dr * dr + dg * dg) + db * db;
}

// the B3 spline's taps h[|i|]; the six products h[|i|] h[|j|] are exact
__device__ __forceinline__ float dn_h(int i)
{
    const int a = i < 0 ? -i : i;
    return a == 0 ? 0.375f : a == 1 ? 0.25f : 0.0625f;
}

template <int TERMS, bool DEMOD_IN>
__global__ __launch_bounds__(256) void denoise_direct(const KDenoise k)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    const int W = k.W, H = k.H, s = k.step;
    if (x >= W || y >= H) return;
    // C(q): the level's input, level 0 of a demodulated run: beauty / A'
    auto color = [&](size_t at, float &r, float &g, float &b) {
        r = k.in[3u * at];
        g = k.in[3u * at + 1u];
        b = k.in[3u * at + 2u];
        if (DEMOD_IN) {
            r = r / fmaxf(k.albedo[3u * at], kDnAlbedoFloor);
            g = g / fmaxf(k.albedo[3u * at + 1u], kDnAlbedoFloor);
            b = b / fmaxf(k.albedo[3u * at + 2u], kDnAlbedoFloor);
        }
    };
    const size_t p = (size_t)y * W + x;
    float cr, cg, cb, nx = 0.f, ny = 0.f, nz = 0.f, pz = 0.f, ar = 0.f, ag = 0.f, ab = 0.f;
    color(p, cr, cg, cb);
    if (TERMS & kDnNormal) nx = k.normal[3u * p], ny = k.normal[3u * p + 1u], nz = k.normal[3u * p + 2u];
    if (TERMS & kDnDepth) pz = k.depth[p];
    if (TERMS & kDnAlbedo) ar = k.albedo[3u * p], ag = k.albedo[3u * p + 1u], ab = k.albedo[3u * p + 2u];
    float sumw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
#pragma unroll
    for (int j = -2; j <= 2; ++j) {
        const int qy = y + j * s;
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const int qx = x + i * s;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;  // skipped: nothing is added
            const size_t q = (size_t)qy * W + qx;
            float w = dn_h(i) * dn_h(j);
            float qr, qg, qb;
            color(q, qr, qg, qb);
            if (TERMS & kDnColor) w = w * dn_edge(dn_dist2(qr, qg, qb, cr, cg, cb), k.r_c);
            if (TERMS & kDnNormal)
                w = w * dn_edge(dn_dist2(k.normal[3u * q], k.normal[3u * q + 1u], k.normal[3u * q + 2u], nx, ny, nz),
                                k.r_n);
            if (TERMS & kDnDepth) {
                const float dz = k.depth[q] - pz;
                w = w * dn_edge(dz * dz, k.r_z);
            }
            if (TERMS & kDnAlbedo)
                w = w * dn_edge(dn_dist2(k.albedo[3u * q], k.albedo[3u * q + 1u], k.albedo[3u * q + 2u], ar, ag, ab),
                                k.r_a);
            sumw = sumw + w;
            sr = sr + w * qr;
            sg = sg + w * qg;
            sb = sb + w * qb;
        }
    }
    float o0 = sr / sumw, o1 = sg / sumw, o2 = sb / sumw;
    if (k.demod_out) {
        o0 = o0 * fmaxf(k.albedo[3u * p], kDnAlbedoFloor);
        o1 = o1 * fmaxf(k.albedo[3u * p + 1u], kDnAlbedoFloor);
        o2 = o2 * fmaxf(k.albedo[3u * p + 2u], kDnAlbedoFloor);
    }
    k.out[3u * p] = o0;
    k.out[3u * p + 1u] = o1;
    k.out[3u * p + 2u] = o2;
}

// channels a staged pixel holds: the colour and the guides of the terms that are on
__host__ __device__ constexpr int dn_channels(int terms)
{
    return 3 + ((terms & kDnNormal) ? 3 : 0) + ((terms & kDnDepth) ? 1 : 0) + ((terms & kDnAlbedo) ? 3 : 0);
}

// The LDS image is one plane per channel, each (32 + 4 step) x (16 + 4 step) floats, row-major:
// the 32 lanes of a half-wave read 32 consecutive floats of one plane for every tap, whatever the
// step, so no read meets a bank conflict (an interleaved rgb image would put a stride of 3 floats
// between the lanes). Staged pixels outside the image are left unwritten: their taps are skipped.
template <int TERMS, bool DEMOD_IN>
__global__ __launch_bounds__(256) void denoise_tiled(const KDenoise k)
{
    extern __shared__ float dn_lds[];
    constexpr int NCH = dn_channels(TERMS);
    constexpr int CN = 3, CZ = CN + ((TERMS & kDnNormal) ? 3 : 0), CA = CZ + ((TERMS & kDnDepth) ? 1 : 0);
    const int W = k.W, H = k.H, s = k.step, halo = 2 * s;
    const int lw = kDnTileW + 2 * halo, lh = kDnTileH + 2 * halo, plane = lw * lh;
    const int x0 = blockIdx.x * kDnTileW - halo, y0 = blockIdx.y * kDnTileH - halo;
    const int tid = threadIdx.y * kDnTileW + threadIdx.x;
    for (int idx = tid; idx < plane; idx += 256) {
        const int lx = idx % lw, ly = idx / lw, gx = x0 + lx, gy = y0 + ly;
        if (gx < 0 || gx >= W || gy < 0 || gy >= H) continue;
        const size_t at = (size_t)gy * W + gx;
        float r = k.in[3u * at], g = k.in[3u * at + 1u], b = k.in[3u * at + 2u];
        if (DEMOD_IN || (TERMS & kDnAlbedo)) {
            const float a0 = k.albedo[3u * at], a1 = k.albedo[3u * at + 1u], a2 = k.albedo[3u * at + 2u];
            if (DEMOD_IN) {
                r = r / fmaxf(a0, kDnAlbedoFloor);
                g = g / fmaxf(a1, kDnAlbedoFloor);
                b = b / fmaxf(a2, kDnAlbedoFloor);
            }
            if (TERMS & kDnAlbedo) {
                dn_lds[CA * plane + idx] = a0;
                dn_lds[(CA + 1) * plane + idx] = a1;
                dn_lds[(CA + 2) * plane + idx] = a2;
            }
        }
        dn_lds[idx] = r;
        dn_lds[plane + idx] = g;
        dn_lds[2 * plane + idx] = b;
        if (TERMS & kDnNormal) {
            dn_lds[CN * plane + idx] = k.normal[3u * at];
            dn_lds[(CN + 1) * plane + idx] = k.normal[3u * at + 1u];
            dn_lds[(CN + 2) * plane + idx] = k.normal[3u * at + 2u];
        }
        if (TERMS & kDnDepth) dn_lds[CZ * plane + idx] = k.depth[at];
    }
    __syncthreads();
    static_assert(NCH == CA + ((TERMS & kDnAlbedo) ? 3 : 0), "plane order");
    const int x = blockIdx.x * kDnTileW + threadIdx.x;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int ty = threadIdx.y + 8 * half, y = blockIdx.y * kDnTileH + ty;
        if (x >= W || y >= H) continue;
        const int c = (ty + halo) * lw + threadIdx.x + halo;
        const float cr = dn_lds[c], cg = dn_lds[plane + c], cb = dn_lds[2 * plane + c];
        float nx = 0.f, ny = 0.f, nz = 0.f, pz = 0.f, ar = 0.f, ag = 0.f, ab = 0.f;
        if (TERMS & kDnNormal)
            nx = dn_lds[CN * plane + c], ny = dn_lds[(CN + 1) * plane + c], nz = dn_lds[(CN + 2) * plane + c];
        if (TERMS & kDnDepth) pz = dn_lds[CZ * plane + c];
        if (TERMS & kDnAlbedo)
            ar = dn_lds[CA * plane + c], ag = dn_lds[(CA + 1) * plane + c], ab = dn_lds[(CA + 2) * plane + c];
        float sumw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
#pragma unroll
        for (int j = -2; j <= 2; ++j) {
            const int qy = y + j * s;
#pragma unroll
            for (int i = -2; i <= 2; ++i) {
                const int qx = x + i * s;
                if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;  // skipped: nothing is added
                const int q = c + j * s * lw + i * s;
                float w = dn_h(i) * dn_h(j);
                const float qr = dn_lds[q], qg = dn_lds[plane + q], qb = dn_lds[2 * plane + q];
                if (TERMS & kDnColor) w = w * dn_edge(dn_dist2(qr, qg, qb, cr, cg, cb), k.r_c);
                if (TERMS & kDnNormal)
                    w = w * dn_edge(dn_dist2(dn_lds[CN * plane + q], dn_lds[(CN + 1) * plane + q],
                                             dn_lds[(CN + 2) * plane + q], nx, ny, nz),
                                    k.r_n);
                if (TERMS & kDnDepth) {
                    const float dz = dn_lds[CZ * plane + q] - pz;
                    w = w * dn_edge(dz * dz, k.r_z);
                }
                if (TERMS & kDnAlbedo)
                    w = w * dn_edge(dn_dist2(dn_lds[CA * plane + q], dn_lds[(CA + 1) * plane + q],
                                             dn_lds[(CA + 2) * plane + q], ar, ag, ab),
                                    k.r_a);
                sumw = sumw + w;
                sr = sr + w * qr;
                sg = sg + w * qg;
                sb = sb + w * qb;
            }
        }
        const size_t p = (size_t)y * W + x;
        float o0 = sr / sumw, o1 = sg / sumw, o2 = sb / sumw;
        if (k.demod_out) {
            o0 = o0 * fmaxf(k.albedo[3u * p], kDnAlbedoFloor);
            o1 = o1 * fmaxf(k.albedo[3u * p + 1u], kDnAlbedoFloor);
            o2 = o2 * fmaxf(k.albedo[3u * p + 2u], kDnAlbedoFloor);
        }
        k.out[3u * p] = o0;
        k.out[3u * p + 1u] = o1;
        k.out[3u * p + 2u] = o2;
    }
}

// instantiation v = TERMS | DEMOD_IN << 4
template <size_t... V>
static const void *direct_ptr(uint32_t v, std::index_sequence<V...>)
{
    static const void *const t[] = {reinterpret_cast<const void *>(&denoise_direct<int(V & 15u), (V >> 4) != 0u>)...};
    return t[v];
}
template <size_t... V>
static const void *tiled_ptr(uint32_t v, std::index_sequence<V...>)
{
    static const void *const t[] = {reinterpret_cast<const void *>(&denoise_tiled<int(V & 15u), (V >> 4) != 0u>)...};
    return t[v];
}

// LDS bytes of a tiled launch at this step with these terms
size_t denoise_tiled_lds(uint32_t terms, uint32_t step)
{
    const size_t lw = kDnTileW + 4u * step, lh = kDnTileH + 4u * step;
    return lw * lh * dn_channels(static_cast<int>(terms)) * sizeof(float);
}

hipError_t launch_denoise(const KDenoise &k, uint32_t terms, bool demod_in, bool tiled, hipStream_t stream)
{
    const uint32_t v = (terms & 15u) | (demod_in ? 16u : 0u);
    void *args[] = {const_cast<KDenoise *>(&k)};
    if (tiled) {
        const dim3 grid((k.W + kDnTileW - 1) / kDnTileW, (k.H + kDnTileH - 1) / kDnTileH);
        return hipLaunchKernel(tiled_ptr(v, std::make_index_sequence<32>{}), grid, dim3(kDnTileW, 8), args,
                               denoise_tiled_lds(terms, k.step), stream);
    }
    const dim3 grid((k.W + 63) / 64, (k.H + 3) / 4);
    return hipLaunchKernel(direct_ptr(v, std::make_index_sequence<32>{}), grid, dim3(64, 4), args, 0, stream);
}

// ---- the variance-guided level (rt_denoise_var_device) -------------------------
// denoise_direct's tap loop with two differences: the colour term's r_c is formed per pixel from the
// 3x3 prefiltered variance (clamped coordinates, spacing 1), and every tap also adds w^2 V(q) to the
// variance carried to the next level. One lane per pixel, 64 consecutive x per wave row (every plane
// is read with unit stride over the lanes); the terms are compiled out as above.
template <int TERMS>
__global__ __launch_bounds__(256) void denoise_var_direct(const KDenoiseVar kv)
{
    const KDenoise &k = kv.d;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    const int W = k.W, H = k.H, s = k.step;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    float r_c = 0.f;
    if (TERMS & kDnColor) {
        float g = 0.f;
#pragma unroll
        for (int j = -1; j <= 1; ++j) {
            const int qy = min(max(y + j, 0), H - 1);
#pragma unroll
            for (int i = -1; i <= 1; ++i) {
                const int qx = min(max(x + i, 0), W - 1);
                const float kk = (i == 0 && j == 0) ? 0.25f : (i == 0 || j == 0) ? 0.125f : 0.0625f;
                g = g + kk * kv.vin[(size_t)qy * W + qx];
            }
        }
        r_c = 1.0f / (kv.sc2 * g + kv.var_floor);
    }
    const float cr = k.in[3u * p], cg = k.in[3u * p + 1u], cb = k.in[3u * p + 2u];
    float nx = 0.f, ny = 0.f, nz = 0.f, pz = 0.f, ar = 0.f, ag = 0.f, ab = 0.f;
    if (TERMS & kDnNormal) nx = k.normal[3u * p], ny = k.normal[3u * p + 1u], nz = k.normal[3u * p + 2u];
    if (TERMS & kDnDepth) pz = k.depth[p];
    if (TERMS & kDnAlbedo) ar = k.albedo[3u * p], ag = k.albedo[3u * p + 1u], ab = k.albedo[3u * p + 2u];
    float sumw = 0.f, sumv = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
#pragma unroll
    for (int j = -2; j <= 2; ++j) {
        const int qy = y + j * s;
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const int qx = x + i * s;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;  // skipped: nothing is added
            const size_t q = (size_t)qy * W + qx;
            float w = dn_h(i) * dn_h(j);
            const float qr = k.in[3u * q], qg = k.in[3u * q + 1u], qb = k.in[3u * q + 2u];
            if (TERMS & kDnColor) w = w * dn_edge(dn_dist2(qr, qg, qb, cr, cg, cb), r_c);
            if (TERMS & kDnNormal)
                w = w * dn_edge(dn_dist2(k.normal[3u * q], k.normal[3u * q + 1u], k.normal[3u * q + 2u], nx, ny, nz),
                                k.r_n);
            if (TERMS & kDnDepth) {
                const float dz = k.depth[q] - pz;
                w = w * dn_edge(dz * dz, k.r_z);
            }
            if (TERMS & kDnAlbedo)
                w = w * dn_edge(dn_dist2(k.albedo[3u * q], k.albedo[3u * q + 1u], k.albedo[3u * q + 2u], ar, ag, ab),
                                k.r_a);
            sumw = sumw + w;
            sumv = sumv + (w * w) * kv.vin[q];
            sr = sr + w * qr;
            sg = sg + w * qg;
            sb = sb + w * qb;
        }
    }
    k.out[3u * p] = sr / sumw;
    k.out[3u * p + 1u] = sg / sumw;
    k.out[3u * p + 2u] = sb / sumw;
    if (kv.vout) kv.vout[p] = sumv / (sumw * sumw);
}

template <size_t... V>
static const void *var_ptr(uint32_t v, std::index_sequence<V...>)
{
    static const void *const t[] = {reinterpret_cast<const void *>(&denoise_var_direct<int(V)>)...};
    return t[v];
}

hipError_t launch_denoise_var(const KDenoiseVar &k, uint32_t terms, hipStream_t stream)
{
    void *args[] = {const_cast<KDenoiseVar *>(&k)};
    const dim3 grid((k.d.W + 63) / 64, (k.d.H + 3) / 4);
    return hipLaunchKernel(var_ptr(terms & 15u, std::make_index_sequence<16>{}), grid, dim3(64, 4), args, 0, stream);
}

} // namespace rt
