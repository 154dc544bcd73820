// rt_upsample.hip — guided upsampling of a low-resolution frame (rt_upsample_device, DESIGN.md
// §4.15): a joint-bilateral upsample whose four bilinear taps are tested against first-hit guides of
// the output size. A translation unit of its own: the other kernels' machine code does not depend
// on it.
//
// One launch, one lane per output pixel, 64 x 4 workgroups as temporal_accumulate: a wave covers 64
// consecutive pixels of an output row, so every load of an output-size guide and every store has
// unit stride over the lanes. Unlike the temporal stage's, a workgroup's tap footprint is known
// before any load: a rectangle of at most 66 x 6 low-resolution pixels (lw <= w, lh <= h; the
// positions are monotone in x and y, so the block's first and last pixel bound it). The workgroup
// stages that rectangle of the five low-resolution planes in LDS (14 KiB) and the taps read it
// there: 0.91 of the direct-load form's time at 640x360 -> 1280x720 (profiles/upscale/ab_staged.txt,
// DESIGN.md §4.15); that form stays as the A/B build -DRT_UPSAMPLE_DIRECT (scripts/build_variant.sh).
// include/rt_api.h states the arithmetic; every operation below is a separate binary32 operation,
// in the contract's order, the same in both forms. VARIANCE = false is the call without the
// variance pair: the colour's operations are the same ones.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rt_device.h"

namespace rt {

#ifdef RT_UPSAMPLE_DIRECT
// A/B: every tap a direct load (neighbouring lanes share taps, so the reads hit cache).
template <bool VARIANCE>
__global__ __launch_bounds__(256) void upsample_guided(const KUpsample k)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    const int W = k.W, H = k.H, LW = k.LW, LH = k.LH;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const bool surface = k.alpha[p] == 1.0f;
    const uint32_t id = k.id[p];
    const float nx = k.normal[3u * p], ny = k.normal[3u * p + 1u], nz = k.normal[3u * p + 2u];
    const float z = k.depth[p];
    const float ztol = k.depth_tol * z;
    const float px = (((float)x + 0.5f) / (float)W) * (float)LW - 0.5f;
    const float py = (((float)y + 0.5f) / (float)H) * (float)LH - 0.5f;
    // px in (-0.5, LW - 0.5), py in (-0.5, LH - 0.5): ix in [-1, LW - 1], iy in [-1, LH - 1]
    const float fx = floorf(px), fy = floorf(py);
    const float tx = px - fx, ty = py - fy;
    const int ix = (int)fx, iy = (int)fy;
    float pw = 0.f, pr = 0.f, pg = 0.f, pb = 0.f, pv = 0.f;
    float gw = 0.f, gr = 0.f, gg = 0.f, gb = 0.f, gv = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ty_ = iy + j;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int tx_ = ix + i;
            if (tx_ < 0 || tx_ >= LW || ty_ < 0 || ty_ >= LH) continue;  // skipped: nothing is added
            const size_t t = (size_t)ty_ * LW + tx_;
            const float wgt = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
            const float cr = k.l_color[3u * t], cg = k.l_color[3u * t + 1u], cb = k.l_color[3u * t + 2u];
            const float wr = wgt * cr, wg = wgt * cg, wb = wgt * cb;
            float wv = 0.f;
            if (VARIANCE) wv = (wgt * wgt) * k.l_variance[t];
            pw = pw + wgt;
            pr = pr + wr;
            pg = pg + wg;
            pb = pb + wb;
            if (VARIANCE) pv = pv + wv;
            if (k.l_id[t] != id) continue;
            if (surface) {
                const float ex = k.l_normal[3u * t] - nx, ey = k.l_normal[3u * t + 1u] - ny,
                            ez = k.l_normal[3u * t + 2u] - nz;
                if ((ex * ex + ey * ey) + ez * ez > k.normal_tol) continue;
                if (fabsf(k.l_depth[t] - z) > ztol) continue;
            }
            gw = gw + wgt;
            gr = gr + wr;
            gg = gg + wg;
            gb = gb + wb;
            if (VARIANCE) gv = gv + wv;
        }
    }
    const bool guided = gw >= 0.01f;
    const float sw = guided ? gw : pw;
    k.o_color[3u * p] = (guided ? gr : pr) / sw;
    k.o_color[3u * p + 1u] = (guided ? gg : pg) / sw;
    k.o_color[3u * p + 2u] = (guided ? gb : pb) / sw;
    if (VARIANCE) k.o_variance[p] = (guided ? gv : pv) / (sw * sw);
}

#else
// The product's form: the tile is [tx0, tx1] x [ty0, ty1], clamped to the image and to 66 x 6; a
// tap inside the image that the tile does not hold (which the bound above excludes) is loaded
// directly, so no LDS index depends on that bound being right.
constexpr int kTileW = 66, kTileH = 6, kTilePx = kTileW * kTileH;

__device__ __forceinline__ int up_floor_pos(int x, int w, int lw)
{
    return (int)floorf((((float)x + 0.5f) / (float)w) * (float)lw - 0.5f);
}

template <bool VARIANCE>
__global__ __launch_bounds__(256) void upsample_guided(const KUpsample k)
{
    __shared__ float s_color[3 * kTilePx], s_normal[3 * kTilePx], s_depth[kTilePx], s_var[VARIANCE ? kTilePx : 1];
    __shared__ uint32_t s_id[kTilePx];
    const int W = k.W, H = k.H, LW = k.LW, LH = k.LH;
    const int bx0 = blockIdx.x * 64, by0 = blockIdx.y * 4;
    const int tx0 = max(up_floor_pos(bx0, W, LW), 0), ty0 = max(up_floor_pos(by0, H, LH), 0);
    const int tx1 = min(up_floor_pos(min(bx0 + 63, W - 1), W, LW) + 1, LW - 1);
    const int ty1 = min(up_floor_pos(min(by0 + 3, H - 1), H, LH) + 1, LH - 1);
    const int tw = max(min(tx1 - tx0 + 1, kTileW), 0), th = max(min(ty1 - ty0 + 1, kTileH), 0);
    for (int s = threadIdx.y * 64 + threadIdx.x; s < tw * th; s += 256) {
        const int r = s / tw, c = s - r * tw;
        const size_t t = (size_t)(ty0 + r) * LW + (tx0 + c);  // tx0 + c <= tx1 < LW, ty0 + r <= ty1 < LH
        const int d = r * kTileW + c;
        s_color[3 * d] = k.l_color[3u * t], s_color[3 * d + 1] = k.l_color[3u * t + 1u], s_color[3 * d + 2] = k.l_color[3u * t + 2u];
        s_normal[3 * d] = k.l_normal[3u * t], s_normal[3 * d + 1] = k.l_normal[3u * t + 1u], s_normal[3 * d + 2] = k.l_normal[3u * t + 2u];
        s_depth[d] = k.l_depth[t];
        s_id[d] = k.l_id[t];
        if (VARIANCE) s_var[d] = k.l_variance[t];
    }
    __syncthreads();
    const int x = bx0 + threadIdx.x, y = by0 + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const bool surface = k.alpha[p] == 1.0f;
    const uint32_t id = k.id[p];
    const float nx = k.normal[3u * p], ny = k.normal[3u * p + 1u], nz = k.normal[3u * p + 2u];
    const float z = k.depth[p];
    const float ztol = k.depth_tol * z;
    const float px = (((float)x + 0.5f) / (float)W) * (float)LW - 0.5f;
    const float py = (((float)y + 0.5f) / (float)H) * (float)LH - 0.5f;
    const float fx = floorf(px), fy = floorf(py);
    const float tx = px - fx, ty = py - fy;
    const int ix = (int)fx, iy = (int)fy;
    float pw = 0.f, pr = 0.f, pg = 0.f, pb = 0.f, pv = 0.f;
    float gw = 0.f, gr = 0.f, gg = 0.f, gb = 0.f, gv = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ty_ = iy + j;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int tx_ = ix + i;
            if (tx_ < 0 || tx_ >= LW || ty_ < 0 || ty_ >= LH) continue;  // skipped: nothing is added
            const size_t t = (size_t)ty_ * LW + tx_;
            const bool held = (unsigned)(tx_ - tx0) < (unsigned)tw && (unsigned)(ty_ - ty0) < (unsigned)th;
            const int d = held ? (ty_ - ty0) * kTileW + (tx_ - tx0) : 0;
            const float wgt = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
            float cr, cg, cb, tv = 0.f, en0, en1, en2, tz;
            uint32_t tid;
            if (held) {
                cr = s_color[3 * d], cg = s_color[3 * d + 1], cb = s_color[3 * d + 2];
                en0 = s_normal[3 * d], en1 = s_normal[3 * d + 1], en2 = s_normal[3 * d + 2];
                tz = s_depth[d], tid = s_id[d];
                if (VARIANCE) tv = s_var[d];
            } else {
                cr = k.l_color[3u * t], cg = k.l_color[3u * t + 1u], cb = k.l_color[3u * t + 2u];
                en0 = k.l_normal[3u * t], en1 = k.l_normal[3u * t + 1u], en2 = k.l_normal[3u * t + 2u];
                tz = k.l_depth[t], tid = k.l_id[t];
                if (VARIANCE) tv = k.l_variance[t];
            }
            const float wr = wgt * cr, wg = wgt * cg, wb = wgt * cb;
            float wv = 0.f;
            if (VARIANCE) wv = (wgt * wgt) * tv;
            pw = pw + wgt;
            pr = pr + wr;
            pg = pg + wg;
            pb = pb + wb;
            if (VARIANCE) pv = pv + wv;
            if (tid != id) continue;
            if (surface) {
                const float ex = en0 - nx, ey = en1 - ny, ez = en2 - nz;
                if ((ex * ex + ey * ey) + ez * ez > k.normal_tol) continue;
                if (fabsf(tz - z) > ztol) continue;
            }
            gw = gw + wgt;
            gr = gr + wr;
            gg = gg + wg;
            gb = gb + wb;
            if (VARIANCE) gv = gv + wv;
        }
    }
    const bool guided = gw >= 0.01f;
    const float sw = guided ? gw : pw;
    k.o_color[3u * p] = (guided ? gr : pr) / sw;
    k.o_color[3u * p + 1u] = (guided ? gg : pg) / sw;
    k.o_color[3u * p + 2u] = (guided ? gb : pb) / sw;
    if (VARIANCE) k.o_variance[p] = (guided ? gv : pv) / (sw * sw);
}
#endif

hipError_t launch_upsample(const KUpsample &k, hipStream_t stream)
{
    void *args[] = {const_cast<KUpsample *>(&k)};
    const dim3 grid((k.W + 63) / 64, (k.H + 3) / 4);
    const void *fn = k.o_variance ? reinterpret_cast<const void *>(&upsample_guided<true>)
                                  : reinterpret_cast<const void *>(&upsample_guided<false>);
    return hipLaunchKernel(fn, grid, dim3(64, 4), args, 0, stream);
}

} // namespace rt
