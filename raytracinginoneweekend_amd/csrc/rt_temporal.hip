// rt_temporal.hip — temporal accumulation: the previous frame's history reprojected into the
// current frame (rt_temporal_device; SVGF, Schied et al. 2017, §4.1). A translation
// unit of its own: the render, feature-buffer and denoise kernels' machine code does not depend on it.
//
// One launch, one lane per pixel, 64 x 4 workgroups as denoise_direct: a wave covers 64 consecutive
// pixels of a row, so every current-frame load and every store has unit stride over the lanes, and
// the four taps of neighbouring lanes fall in the same or adjacent cache lines under any smooth
// motion. No LDS tile: the tap positions are data-dependent, and the footprint of a tile's taps is
// not known before the projection is done. include/rt_api.h states the arithmetic; every operation
// below is a separate binary32 operation, in the contract's order. HISTORY = false is the frame
// without history: a copy.
//
// MOTION (rt_temporal_motion_device): a surface pixel's first hit is carried back by
// its sphere's motion m = C - C' before it is projected: the two table rows of the pixel's id are read
// from global memory, one 16-byte load each (the tables are small and stay in cache). A form whose
// workgroup first staged {m, same-radius flag} of every sphere in LDS was measured and was slower
// (31.5 against 23.4 us at 1280x720 with 486 spheres: every workgroup pays for the whole table, and 32
// KiB of LDS cost occupancy; profiles/motion/lds_form.diff keeps it). MOTION = false is the static stage:
// its machine code is what it was before the parameter existed.
//
// CLIP (rt_temporal_clip_device): the resampled history colour is clamped to the box
// mean +- gamma standard deviations of the current frame's colours around the pixel. Unlike the history
// taps, that window is a fixed rectangle of the current frame, so the workgroup stages its tile of
// {beauty, sphere_id} plus a halo of `radius` texels in LDS (one float4 per texel, the id's bits in w:
// a lane's tap reads the id and, if it is the pixel's, the colour of one 16-byte texel, and the lanes of a
// wave read consecutive texels), and every lane takes its window from there. Lanes outside the image help
// to stage and reach the barrier before they leave; halo texels outside the image are not read from memory
// (zeros are staged) and a lane skips them by their coordinates. CLIP = false is the stage without the
// clamp: its machine code is what it was before the parameter existed (no LDS, no barrier, the early
// return first), and it does not name the tile.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rt_device.h"

namespace rt {

__device__ __forceinline__ float tp_dot(const float *a, float x, float y, float z)
{
    return (a[0] * x + a[1] * y) + a[2] * z;
}

// The clip kernel's workgroup: RT_CLIP_BW x (256 / RT_CLIP_BW) lanes. 64 x 4 as the plain kernel; -DRT_CLIP_BW=32
// builds the 32 x 8 form, which reads a smaller halo (DESIGN.md §4.17 keeps both forms' figures).
#ifndef RT_CLIP_BW
#define RT_CLIP_BW 64
#endif
constexpr int kClipBW = RT_CLIP_BW, kClipBH = 256 / RT_CLIP_BW, kClipMaxRadius = 3;
constexpr int kClipTexels = (kClipBW + 2 * kClipMaxRadius) * (kClipBH + 2 * kClipMaxRadius);
static_assert(kClipBW * kClipBH == 256 && kClipBW % 32 == 0, "the clip kernel's workgroup is 256 lanes in whole half-waves");
// the staged tile at the largest radius (70 x 10 texels at 64 x 4: 11200 bytes); only the CLIP kernels name it
__shared__ float4 g_clip_tile[kClipTexels];

// The workgroup's tile of {beauty, id} and its halo of R texels into LDS, row-major, (kClipBW + 2 R) texels a
// row (a compile-time width: the texel's row and column cost no division). A texel outside the image is
// not read: zeros are staged.
template <int R>
__device__ __forceinline__ void stage_tile(float4 *tile, const float *beauty, const uint32_t *id, int W, int H)
{
    constexpr int TW = kClipBW + 2 * R, texels = TW * (kClipBH + 2 * R);
    const int x0 = (int)blockIdx.x * kClipBW - R, y0 = (int)blockIdx.y * kClipBH - R;
    for (int t = (int)threadIdx.y * kClipBW + (int)threadIdx.x; t < texels; t += 256) {
        const int ty = t / TW, gx = x0 + (t - ty * TW), gy = y0 + ty;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t g = (size_t)gy * W + gx;
            v = make_float4(beauty[3u * g], beauty[3u * g + 1u], beauty[3u * g + 2u], __uint_as_float(id[g]));
        }
        tile[t] = v;
    }
}

// Step 5b of the contract for the lane at (lx, ly) of the workgroup, pixel (x, y): the history colour
// (c0, c1, c2) clamped to the box of the (2 R + 1)^2 window, read from the staged tile.
template <int R>
__device__ __forceinline__ void clip_history(const float4 *tile, int lx, int ly, int x, int y, int W, int H, float br,
                                             float bg, float bb, uint32_t id, float gamma, float &c0, float &c1, float &c2)
{
    constexpr int TW = kClipBW + 2 * R;
    float n = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = -R; j <= R; ++j) {
        const bool row = y + j >= 0 && y + j < H;
#pragma unroll
        for (int i = -R; i <= R; ++i) {
            // (A form without these branches, a skipped tap adding +0.0f, lets the compiler issue the whole
            // window's LDS loads together: 226 VGPRs, 2 waves per SIMD, twice the time. DESIGN.md §4.17.)
            if (!row || x + i < 0 || x + i >= W) continue;  // skipped: nothing is added
            const float4 t = tile[(ly + R + j) * TW + (lx + R + i)];
            if (__float_as_uint(t.w) != id) continue;
            n = n + 1.0f;
            const float d0 = t.x - br, d1 = t.y - bg, d2 = t.z - bb;
            a0 = a0 + d0, a1 = a1 + d1, a2 = a2 + d2;
            s0 = s0 + d0 * d0, s1 = s1 + d1 * d1, s2 = s2 + d2 * d2;
        }
    }
    auto clamp = [&](float c, float b, float m1, float m2) {
        const float mean = m1 / n, ex2 = m2 / n;
        const float var = fmaxf(0.0f, ex2 - mean * mean);
        const float half = gamma * sqrtf(var);
        const float mu = b + mean;
        const float lo = mu - half, hi = mu + half;
        return fminf(fmaxf(c, lo), hi);
    };
    c0 = clamp(c0, br, a0, s0), c1 = clamp(c1, bg, a1, s1), c2 = clamp(c2, bb, a2, s2);
}

template <bool HISTORY, bool MOTION, bool CLIP>
__global__ __launch_bounds__(256) void temporal_accumulate(const KTemporal k)
{
    constexpr int BW = CLIP ? kClipBW : 64, BH = CLIP ? kClipBH : 4;
    const int x = blockIdx.x * BW + threadIdx.x, y = blockIdx.y * BH + threadIdx.y;
    const int W = k.W, H = k.H;
    if constexpr (CLIP) {  // (discarded, the tile's name with it, when CLIP is false)
        // every lane, also one outside the image (the host checks radius <= 3: any other value stages
        // and reads the radius-3 tile, so the tile's size holds whatever the record says)
        switch (k.clip_radius) {  // uniform over the grid
        case 1: stage_tile<1>(g_clip_tile, k.beauty, k.id, W, H); break;
        case 2: stage_tile<2>(g_clip_tile, k.beauty, k.id, W, H); break;
        default: stage_tile<3>(g_clip_tile, k.beauty, k.id, W, H); break;
        }
        __syncthreads();
    }
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float br = k.beauty[3u * p], bg = k.beauty[3u * p + 1u], bb = k.beauty[3u * p + 2u];
    const float var = k.variance[p];
    // no history: the current frame's bits, a history of one frame
    float o0 = br, o1 = bg, o2 = bb, ov = var, on = 1.0f;
    if (HISTORY) {
        const float al = k.alpha[p];
        const bool surface = al == 1.0f;
        if (surface || al == 0.0f) {
            const float fw = (float)W, fh = (float)H;
            const float u = ((float)x + 0.5f) / fw;
            const float m = 1.0f - ((float)y + 0.5f) / fh;
            const float dx = (k.a[0] + k.hor[0] * u) + k.ver[0] * m;
            const float dy = (k.a[1] + k.hor[1] * u) + k.ver[1] * m;
            const float dz = (k.a[2] + k.hor[2] * u) + k.ver[2] * m;
            float qx = dx, qy = dy, qz = dz;
            bool moved_ok = true;  // MOTION: the sphere is in the tables and kept its radius
            if (surface) {
                const float t = k.depth[p];
                if (MOTION) {
                    // an id outside the tables reads neither; a resized sphere restarts
                    const uint32_t sid = k.id[p];
                    float mx = 0.f, my = 0.f, mz = 0.f;
                    moved_ok = sid < k.n_spheres;
                    if (moved_ok) {
                        const float4 c = reinterpret_cast<const float4 *>(k.centres)[sid];
                        const float4 b = reinterpret_cast<const float4 *>(k.p_centres)[sid];
                        mx = c.x - b.x, my = c.y - b.y, mz = c.z - b.z;
                        moved_ok = __float_as_uint(c.w) == __float_as_uint(b.w);
                    }
                    qx = ((k.o[0] + t * dx) - mx) - k.basis[9];
                    qy = ((k.o[1] + t * dy) - my) - k.basis[10];
                    qz = ((k.o[2] + t * dz) - mz) - k.basis[11];
                } else {
                    qx = (k.o[0] + t * dx) - k.basis[9];
                    qy = (k.o[1] + t * dy) - k.basis[10];
                    qz = (k.o[2] + t * dz) - k.basis[11];
                }
            }
            const float pa = tp_dot(k.basis, qx, qy, qz);
            const float pb = tp_dot(k.basis + 3, qx, qy, qz);
            const float ga = tp_dot(k.basis + 6, qx, qy, qz);
            if (ga > 0.0f && (!MOTION || moved_ok)) {
                const float px = (pa / ga) * fw - 0.5f;
                const float py = (1.0f - pb / ga) * fh - 0.5f;
                if (px > -1.0f && px < fw && py > -1.0f && py < fh) {
                    // px in (-1, W), py in (-1, H): ix in [-1, W - 1], iy in [-1, H - 1]
                    const float fx = floorf(px), fy = floorf(py);
                    const float tx = px - fx, ty = py - fy;
                    const int ix = (int)fx, iy = (int)fy;
                    const uint32_t id = k.id[p];
                    const float nx = k.normal[3u * p], ny = k.normal[3u * p + 1u], nz = k.normal[3u * p + 2u];
                    const float ztol = k.depth_tol * ga;
                    float sumw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sumv = 0.f, sumn = 0.f;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int ty_ = iy + j;
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            const int tx_ = ix + i;
                            if (tx_ < 0 || tx_ >= W || ty_ < 0 || ty_ >= H) continue;  // skipped: nothing is added
                            const size_t t = (size_t)ty_ * W + tx_;
                            if (k.p_id[t] != id) continue;
                            const float ex = k.p_normal[3u * t] - nx, ey = k.p_normal[3u * t + 1u] - ny,
                                        ez = k.p_normal[3u * t + 2u] - nz;
                            if ((ex * ex + ey * ey) + ez * ez > k.normal_tol) continue;
                            if (surface && fabsf(k.p_depth[t] - ga) > ztol) continue;
                            const float wgt = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                            sumw = sumw + wgt;
                            sr = sr + wgt * k.p_color[3u * t];
                            sg = sg + wgt * k.p_color[3u * t + 1u];
                            sb = sb + wgt * k.p_color[3u * t + 2u];
                            sumv = sumv + (wgt * wgt) * k.p_variance[t];
                            sumn = sumn + wgt * k.p_history[t];
                        }
                    }
                    if (sumw >= 0.01f) {
                        const float n = fminf(sumn / sumw + 1.0f, k.max_history);
                        const float kk = fmaxf(1.0f / n, k.alpha_min), rest = 1.0f - kk;
                        if constexpr (CLIP) {
                            float c0 = sr / sumw, c1 = sg / sumw, c2 = sb / sumw;
                            const int lx = threadIdx.x, ly = threadIdx.y;
                            const float4 *const tile = g_clip_tile;
                            switch (k.clip_radius) {  // uniform over the grid
                            case 1: clip_history<1>(tile, lx, ly, x, y, W, H, br, bg, bb, id, k.clip_gamma, c0, c1, c2); break;
                            case 2: clip_history<2>(tile, lx, ly, x, y, W, H, br, bg, bb, id, k.clip_gamma, c0, c1, c2); break;
                            default: clip_history<3>(tile, lx, ly, x, y, W, H, br, bg, bb, id, k.clip_gamma, c0, c1, c2); break;
                            }
                            o0 = kk * br + rest * c0;
                            o1 = kk * bg + rest * c1;
                            o2 = kk * bb + rest * c2;
                        } else {  // (the statements as they were: the order of the divisions is part of the machine code)
                            o0 = kk * br + rest * (sr / sumw);
                            o1 = kk * bg + rest * (sg / sumw);
                            o2 = kk * bb + rest * (sb / sumw);
                        }
                        ov = (kk * kk) * var + (rest * rest) * (sumv / (sumw * sumw));
                        on = n;
                    }
                }
            }
        }
    }
    k.o_color[3u * p] = o0;
    k.o_color[3u * p + 1u] = o1;
    k.o_color[3u * p + 2u] = o2;
    k.o_variance[p] = ov;
    k.o_history[p] = on;
}

hipError_t launch_temporal(const KTemporal &k, hipStream_t stream)
{
    void *args[] = {const_cast<KTemporal *>(&k)};
    // the motion kernel from a table pointer, the clip kernel from a radius (without history: the copy)
    if (k.p_color && k.clip_radius) {
        const dim3 grid((k.W + kClipBW - 1) / kClipBW, (k.H + kClipBH - 1) / kClipBH);
        const void *fn = k.centres ? reinterpret_cast<const void *>(&temporal_accumulate<true, true, true>)
                                   : reinterpret_cast<const void *>(&temporal_accumulate<true, false, true>);
        return hipLaunchKernel(fn, grid, dim3(kClipBW, kClipBH), args, 0, stream);
    }
    const dim3 grid((k.W + 63) / 64, (k.H + 3) / 4);
    const void *fn = !k.p_color ? reinterpret_cast<const void *>(&temporal_accumulate<false, false, false>)
                     : k.centres ? reinterpret_cast<const void *>(&temporal_accumulate<true, true, false>)
                                 : reinterpret_cast<const void *>(&temporal_accumulate<true, false, false>);
    return hipLaunchKernel(fn, grid, dim3(64, 4), args, 0, stream);
}

} // namespace rt
