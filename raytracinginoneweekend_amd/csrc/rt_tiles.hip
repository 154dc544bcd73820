// rt_tiles.hip — the dealing order of a pass computed on the device:
// classify_tiles_kernel gives every 64-pixel block of the pass its class byte with the host's own
// beam arithmetic (rt_tiles.h: the same expression tree, so the same classes exactly), and
// order_blocks_kernel partitions the blocks by class into the permutation the render kernels read.
// A translation unit of its own: no other kernel's machine code depends on it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rt_tiles.h"

namespace rt {

// One lane per block, 64-lane workgroups (a tile over the scene costs a few dozen slab tests with
// binary64 divisions, a sky tile one: many small workgroups spread the dear rows over the CUs).
// The box and sphere records are indexed by loop counters that are the same in every lane, and
// nothing is stored before the last of them is read: they come in as scalar loads.
__global__ __launch_bounds__(64) void classify_tiles_kernel(const rttile::KTiles k)
{
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (t >= k.n_blocks) return;
    uint8_t c = 1;
    if (t < k.n_tiles) {
        const float *__restrict__ geom = k.geom;
        const rttile::geom_view g{k.has_root ? geom : nullptr,
                                  reinterpret_cast<const rt_sphere *>(geom + 6u + 6u * static_cast<size_t>(k.n_boxes)),
                                  k.n_always, geom + 6u, k.n_boxes, k.clus_pad};
        c = rttile::classify_tile(k.cam, k.pass, g, t, false);
    }
    k.cls[t] = c;
}

// The stable three-way partition of the class bytes: perm = the blocks of class 0 in ascending
// order, then those of class 1, then those of class 2 (the host's three passes over the classes),
// counts = {n_lead, n_sky}. One workgroup of 16 waves walks the blocks in chunks of 1024, twice:
// first to count the classes (where each one's part of perm starts), then to place every block at
// its class's running offset + the blocks of that class in the chunk's earlier waves (LDS) + those
// in the wave's earlier lanes (ballot). perm null: the counts alone.
constexpr uint32_t kOrderLanes = 1024, kOrderWaves = kOrderLanes / 64;

__global__ __launch_bounds__(kOrderLanes) void order_blocks_kernel(const uint8_t *__restrict__ cls, uint32_t n,
                                                                  uint32_t *__restrict__ perm, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t wsum[2][3][kOrderWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;

    uint32_t w0 = 0, w2 = 0;  // this wave's blocks of class 0 and 2 (the same in every lane)
    for (uint32_t base = 0; base < n; base += kOrderLanes) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t c = i < n ? cls[i] : 3u;
        w0 += static_cast<uint32_t>(__popcll(__ballot(c == 0u)));
        w2 += static_cast<uint32_t>(__popcll(__ballot(c == 2u)));
    }
    if (lane == 0) {
        wsum[0][0][wave] = w0;
        wsum[0][2][wave] = w2;
    }
    __syncthreads();
    uint32_t n_lead = 0, n_sky = 0;
    for (uint32_t w = 0; w < kOrderWaves; ++w) {
        n_lead += wsum[0][0][w];
        n_sky += wsum[0][2][w];
    }
    if (threadIdx.x == 0) {
        counts[0] = n_lead;
        counts[1] = n_sky;
    }
    if (!perm) return;
    __syncthreads();  // the totals are read: the first chunk may write wsum[0] again

    uint32_t run[3] = {0u, n_lead, n - n_sky};  // where the chunk's blocks of each class go
    uint32_t buf = 0;
    for (uint32_t base = 0; base < n; base += kOrderLanes, buf ^= 1u) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t c = i < n ? cls[i] : 3u;
        const unsigned long long m0 = __ballot(c == 0u), m1 = __ballot(c == 1u), m2 = __ballot(c == 2u);
        if (lane == 0) {
            wsum[buf][0][wave] = static_cast<uint32_t>(__popcll(m0));
            wsum[buf][1][wave] = static_cast<uint32_t>(__popcll(m1));
            wsum[buf][2][wave] = static_cast<uint32_t>(__popcll(m2));
        }
        // (one barrier per chunk: the chunk after the next writes this buffer again, and a wave
        // gets there only through the next chunk's barrier, after every wave has read this one)
        __syncthreads();
        uint32_t before[3] = {0u, 0u, 0u}, total[3] = {0u, 0u, 0u};
        for (uint32_t w = 0; w < kOrderWaves; ++w)
            for (uint32_t q = 0; q < 3u; ++q) {
                const uint32_t v = wsum[buf][q][w];
                before[q] += w < wave ? v : 0u;
                total[q] += v;
            }
        const unsigned long long mine = c == 0u ? m0 : c == 1u ? m1 : m2;
        const uint32_t at = (c == 0u ? run[0] + before[0] : c == 1u ? run[1] + before[1] : run[2] + before[2]) +
                            static_cast<uint32_t>(__popcll(mine & below));
        if (c < 3u && at < n) perm[at] = i;
        for (uint32_t q = 0; q < 3u; ++q) run[q] += total[q];
    }
}

hipError_t launch_classify_tiles(const rttile::KTiles &k, hipStream_t stream)
{
    if (!k.n_blocks) return hipSuccess;
    void *args[] = {const_cast<rttile::KTiles *>(&k)};
    return hipLaunchKernel(reinterpret_cast<const void *>(&classify_tiles_kernel), dim3((k.n_blocks + 63u) / 64u), dim3(64),
                           args, 0, stream);
}

hipError_t launch_order_blocks(const uint8_t *cls, uint32_t n_blocks, uint32_t *perm, uint32_t *counts, hipStream_t stream)
{
    void *args[] = {&cls, &n_blocks, &perm, &counts};
    return hipLaunchKernel(reinterpret_cast<const void *>(&order_blocks_kernel), dim3(1), dim3(kOrderLanes), args, 0, stream);
}

} // namespace rt
