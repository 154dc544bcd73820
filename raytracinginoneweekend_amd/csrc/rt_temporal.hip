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
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rt_device.h"

namespace rt {

__device__ __forceinline__ float tp_dot(const float *a, float x, float y, float z)
{
    return (a[0] * x + a[1] * y) + a[2] * z;
}

template <bool HISTORY, bool MOTION>
__global__ __launch_bounds__(256) void temporal_accumulate(const KTemporal k)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    const int W = k.W, H = k.H;
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
                        o0 = kk * br + rest * (sr / sumw);
                        o1 = kk * bg + rest * (sg / sumw);
                        o2 = kk * bb + rest * (sb / sumw);
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
    const dim3 grid((k.W + 63) / 64, (k.H + 3) / 4);
    // the motion kernel from a table pointer
    const void *fn = !k.p_color ? reinterpret_cast<const void *>(&temporal_accumulate<false, false>)
                     : k.centres ? reinterpret_cast<const void *>(&temporal_accumulate<true, true>)
                                 : reinterpret_cast<const void *>(&temporal_accumulate<true, false>);
    return hipLaunchKernel(fn, grid, dim3(64, 4), args, 0, stream);
}

} // namespace rt
