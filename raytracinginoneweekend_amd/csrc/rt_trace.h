// rt_trace.h — the device functions every kernel family shares: the reference CPU path's vector
// math, RNG and closest hit, for gfx950 (CDNA4). Included by rt_kernel.hip (the megakernel),
// rt_sky.hip, rt_accum.hip (through rt_accum.h), rt_compat.hip, rt_wavefront.hip and rt_aov.hip;
// everything here is __forceinline__ or a template, so a unit holds only what its kernels use.
//
// Semantics are the reference CPU path, bit for bit in the exact variants:
//   app::color                      src/main.cxx:52-75
//   app::background_color / mix     src/main.cxx:47-50, src/math.hxx:325-329
//   raytracer::hit_world/intersect  src/raytracer.hxx:52-118
//   raytracer::apply_material       src/raytracer.hxx:120-199
//   raytracer::random_in_unit_sphere, schlick  src/raytracer.hxx:32-50
//   raytracer::camera::ray          src/camera.hxx:46-57
//   pixel/sample driver + reduce    src/main.cxx:185-207
// Every binary32 op is separately rounded in the reference's order: this file is compiled
// with -ffp-contract=off and without fast-math, so div/sqrt are the correctly rounded
// sequences and NaN semantics (total internal reflection, src/math.hxx:308) survive.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "rt_device.h"

namespace rt {

#define RT_TMIN 0.008f   // raytracer.hxx:98 kMIN
#define RT_TMAX FLT_MAX  // raytracer.hxx:97 kMAX

struct f3 { float x, y, z; };
__device__ __forceinline__ f3 mk(float x, float y, float z) { return {x, y, z}; }
__device__ __forceinline__ f3 operator+(f3 a, f3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ f3 operator-(f3 a, f3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ f3 operator*(f3 a, f3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
__device__ __forceinline__ f3 operator*(f3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ f3 operator/(f3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ f3 adds(f3 a, float s) { return {a.x + s, a.y + s, a.z + s}; }
__device__ __forceinline__ float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float length(f3 a) { return sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }
__device__ __forceinline__ f3 normalize(f3 a)                    // math.hxx:219-227
{
    float l = length(a);
    return fabsf(l) > FLT_MIN ? a / l : a;
}
__device__ __forceinline__ f3 reflect(f3 I, f3 N) { return I - (N * dot(N, I)) * 2.f; } // math.hxx:294-298
__device__ __forceinline__ float sqrt_scaled(float x);
__device__ __forceinline__ f3 refract(f3 I, f3 N, float eta)                          // math.hxx:300-309
{
    const float d = dot(N, I);
    const float k = 1.f - eta * eta * (1.f - d * d);
    return (I * eta - adds(N * sqrt_scaled(k), d * eta)) * (k >= 0.f ? 1.f : 0.f);  // k <= 1
}

// Diagnostic counters (STATS builds only; see rt_scene_debug_counters): per-lane tallies
// plus wave-level ones counted by the first active lane.
struct Dbg {
    uint32_t wave_blocks, lane_blocks, wave_roots, lane_roots, wave_member_blocks;
    uint32_t ev[kDbgEvents];  // executions of the code blocks below by the wave (rt_scene_debug_events)
};
__device__ __forceinline__ bool first_active_lane()
{
    return (threadIdx.x & 63u) == __builtin_amdgcn_readfirstlane(threadIdx.x & 63u);
}
// block-execution events (STATS builds): counted once per wave each time the block runs
enum DbgEvent : uint32_t {
    EV_ITER, EV_REFILL_TRIP, EV_FRESH, EV_REJECT_TRIP, EV_LENS_DONE, EV_SCATTER_DONE, EV_ROOT_GATE_PASS,
    EV_SUPER, EV_SUPER_PASS, EV_CLUSTER_REQ, EV_TRANSPOSED, EV_T_ROUND, EV_T_FAR, EV_PER_LANE_MEMBERS,
    EV_SKY, EV_HIT, EV_LAMBERT, EV_UNIT_DIR, EV_DIELECTRIC, EV_STORE, EV_METAL_ABSORB,
    EV_LIVE_LANES,  // live lanes summed over wave iterations
    EV_DRY_ITER,    // wave iterations after the item queues ran dry (the drain)
    EV_DRY_LANES,   // live lanes summed over those
    EV_ISO_LANES,   // lanes that skipped the cluster walk (isolated hint sphere), summed over iterations
    EV_WALK_SKIPPED,  // wave iterations with segments whose cluster walk no lane needed
    EV_WALK1, EV_WALK2, EV_WALK4, EV_WALK8,  // wave iterations whose walk 1, 2, 3-4, 5-8 lanes need
    EV_PAIR_SUM,   // (lanes) pair sums stored by the main launch (both samples ended there)
    EV_BOTH_MEET,  // (lanes) pair sums formed in the deep launch by the second of two queued samples
    EV_COUNT
};
static_assert(EV_COUNT <= kDbgEvents, "event counters");
#define RT_EV(e)                                          \
    do {                                                  \
        if (STATS && first_active_lane()) ++dbg.ev[(e)]; \
    } while (0)

// The lane mask of a predicate. Votes are taken on single compares only: the compiler turns the
// vote of a compare into one scalar AND with exec, but materialises any other predicate (an AND
// of compares, a value carried across blocks) as 0/1 in a VGPR and compares it again, two extra
// half-rate VALU operations; compound conditions are formed from masks instead.
__device__ __forceinline__ uint64_t ballot(bool x) { return __builtin_amdgcn_ballot_w64(x); }
__device__ __forceinline__ uint32_t lanes(bool x) { return (uint32_t)__popcll(ballot(x)); }

// Bounds check of the instrumented kernel (STATS; rt_device.h kDbgError): an index at or past its
// bound is recorded (the first one wins) and replaced by 0, so the diagnostic never makes the
// access it reports. The product kernels compile this to the index itself.
template <bool STATS>
__device__ __forceinline__ uint32_t checked(uint32_t i, uint32_t bound, uint32_t code, unsigned long long *dbg)
{
    if (STATS && i >= bound) {
        atomicCAS(dbg + kDbgError, 0ull, ((unsigned long long)code << 32) | i);
        return 0u;
    }
    return i;
}

// ---- RNG: PCG32 XSH-RR per (pixel, sample) stream; the increment is wave-uniform ---------
constexpr uint64_t kPcgMul = 6364136223846793005ULL;
__device__ __forceinline__ uint32_t pcg_out(uint64_t old)
{
    uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u);
    uint32_t rot = (uint32_t)(old >> 59u);
    return (xs >> rot) | (xs << ((0u - rot) & 31u));
}
__device__ __forceinline__ uint32_t pcg_next(uint64_t &state, uint64_t inc)
{
    uint64_t old = state;
    state = old * kPcgMul + inc;
    return pcg_out(old);
}
__device__ __forceinline__ uint64_t pcg_seed(uint64_t initstate, uint64_t inc)
{
    uint64_t st = inc;  // state = 0; next() -> 0 * M + inc
    st += initstate;
    return st * kPcgMul + inc;
}
// libstdc++ generate_canonical<float,24> over a 32-bit engine: float(x) / 2^32, kept < 1.
// float(x) rounds up to 2^32 for the top 128 words; clamping it to the largest float below,
// 2^32 - 256, before the exact scaling gives the same 0x1.fffffep-1.
__device__ __forceinline__ float canonical(uint64_t &st, uint64_t inc)
{
    return fminf((float)pcg_next(st, inc), 0x1.fffffep31f) * 0x1p-32f;
}
// canonical() * 2.f + -1.f (raytracer.hxx:35-37): the product is exact, so the result is the
// one rounding of clamp(float(x)) * 2^-31 - 1, i.e. a single FMA.
__device__ __forceinline__ float canonical_pm1(uint64_t &st, uint64_t inc)
{
    return fmaf(fminf((float)pcg_next(st, inc), 0x1.fffffep31f), 0x1p-31f, -1.f);
}
// RN(a / b) for a per-render divisor b (the image width or height): one reciprocal rb = RN(1/b)
// and one FMA correction (Markstein) when the host has checked, for this b, that the sequence
// reproduces the IEEE quotient for every float mantissa (rt_host_build.cpp exact_by_reciprocal: the
// result then holds for every normal a >= 0, the scaling by powers of two being exact);
// otherwise the IEEE division.
__device__ __forceinline__ float div_const(float a, float b, float rb, bool fast)
{
    if (fast) {
        const float q0 = a * rb;
        const float r = fmaf(-q0, b, a);
        return fmaf(r, rb, q0);
    }
    return a / b;
}
// raytracer.hxx:32-43. `length(p) > 1` is evaluated as `norm(p) > 1 + 2^-23`: with a
// correctly rounded sqrt the two agree for every non-negative float (checked exhaustively,
// tests/test_numerics_cpu.py), and the loop runs as long as its slowest lane.
__device__ __forceinline__ f3 random_in_unit_sphere(uint64_t &st, uint64_t inc)
{
    f3 p;
    do {
        float x = canonical_pm1(st, inc);
        float y = canonical_pm1(st, inc);
        float z = canonical_pm1(st, inc);
        p = mk(x, y, z);
    } while (p.x * p.x + p.y * p.y + p.z * p.z > 0x1.000002p+0f);
    return p;
}

// At most RT_REJECT_CAP attempts of raytracer.hxx:32-43 in this call: `got` tells whether one
// was accepted; if not, st is left after the failed attempts' draws and the caller resumes the
// same sequence next time. The wave runs this as long as its unluckiest lane, up to the cap.
#ifndef RT_REJECT_CAP
#define RT_REJECT_CAP 4  // 0: unbounded (the loop runs until every lane accepts)
#endif
template <bool STATS, int CAP = RT_REJECT_CAP>
__device__ __forceinline__ f3 random_in_unit_sphere_capped(uint64_t &st, uint64_t inc, bool &got, Dbg &dbg)
{
    if (CAP == 0) {
        got = true;
        return random_in_unit_sphere(st, inc);
    }
    // p is written on every attempt a lane makes: a lane that accepted has left the loop, so
    // later attempts do not touch its p, and no per-attempt select is needed (p of a lane that
    // did not accept is not used)
    // The LCG multiplier's halves and the 2^-31 scale sit in VGPRs for the loop (three moves
    // of literals): on gfx950 a VALU operation reading an SGPR issues at half rate
    // (scripts/ubench_int.hip), and the compiler would keep these uniform constants in SGPRs.
    uint32_t m_lo = (uint32_t)kPcgMul, m_hi = (uint32_t)(kPcgMul >> 32);
    float k31 = 0x1p-31f;
    asm volatile("" : "+v"(m_lo), "+v"(m_hi), "+v"(k31));
    const uint64_t mul = ((uint64_t)m_hi << 32) | m_lo;
    auto draw = [&]() {
        const uint64_t old = st;
        st = old * mul + inc;
        return fmaf(fminf((float)pcg_out(old), 0x1.fffffep31f), k31, -1.f);  // canonical_pm1
    };
    f3 p;
    got = false;
#pragma unroll
    for (int k = 0; k < (CAP > 0 ? CAP : 1); ++k) {
        RT_EV(EV_REJECT_TRIP);
        p.x = draw();
        p.y = draw();
        p.z = draw();
        if (!(p.x * p.x + p.y * p.y + p.z * p.z > 0x1.000002p+0f)) {
            got = true;
            break;
        }
    }
    return p;
}

// raytracer.hxx:45-50. std::pow(float,int) promotes to double: r0 = x^2 is exact in double;
// (1-cos)^5 is formed as y^4 * y with y^4 = y^2*y^2 split exactly by an FMA, so the double
// product is within a few 1e-17 relative of glibc's pow before the final cast to float.
// xf = (1 - ri) / (1 + ri) in binary32 (per sphere and side, from the host).
__device__ __forceinline__ float schlick_x(float xf, float c)
{
    double x = (double)xf;
    double r0 = x * x;
    double y = (double)(1.f - c);
    double y2 = y * y;                  // exact (24-bit * 24-bit)
    double y4 = y2 * y2;
    double y4lo = fma(y2, y2, -y4);     // exact residual
    double y5 = fma(y4, y, y4lo * y);
    return (float)(r0 + (1.0 - r0) * y5);
}
__device__ __forceinline__ float schlick(float ri, float c) { return schlick_x((1.f - ri) / (1.f + ri), c); }

// ---- work decomposition ----------------------------------------------------------------
template <class UD>
__device__ __forceinline__ uint32_t udiv(uint32_t n, const UD &u)
{
    const uint32_t t = __umulhi(n, u.m);
    return (t + ((n - t) >> u.s1)) >> u.s2;
}

// pixel (x, packed row rr) of enumeration position i; perm: the pass's block permutation
// (KParams::block_perm) or null
#ifndef RT_PERM_SCALAR
#define RT_PERM_SCALAR 1  // A/B build switch: the block permutation read through the scalar cache
#endif
template <class FC>
__device__ __forceinline__ void pixel_of(const FC &fc, uint32_t i, uint32_t &x, uint32_t &rr, const uint32_t *perm)
{
    if (perm) {
        // the active lanes' positions lie in one or two blocks nearly always (fresh lanes take
        // consecutive items of one tile at one sample): the first lane's block through a scalar
        // load, vector loads only for lanes in another block
        const uint32_t b = i >> 6;
        uint32_t nb;
        if (RT_PERM_SCALAR) {
            const uint32_t b0 = __builtin_amdgcn_readfirstlane(b);
            nb = perm[b0];
            if (b != b0) nb = perm[b];
        } else {
            nb = perm[b];
        }
        i = (nb << 6) | (i & 63u);
    }
    const uint32_t W = fc.W, tiled_rows = fc.tiled_rows, tiles_x = fc.tiles_x;
    const uint32_t tiled_px = tiled_rows * W;
    if (i < tiled_px) {
        uint32_t t = i >> 6, w = i & 63u;
        uint32_t ty = udiv(t, fc.div_tiles_x), tx = t - ty * tiles_x;
        const uint32_t lw = fc.tile_lw;
        x = (tx << lw) + (w & ((1u << lw) - 1u));
        rr = (ty << (6u - lw)) + (w >> lw);
    } else {
        uint32_t j = i - tiled_px;
        rr = udiv(j, fc.div_W);
        x = j - rr * W;
        rr += tiled_rows;
    }
}

// ---- closest hit (raytracer.hxx:94-118) -------------------------------------------------
// The reference tests every sphere on (kMIN, kMAX) and keeps the first minimum in index
// order (stable_partition + min_element with a strict '<'). Here every sphere that is
// tested yields the reference's per-sphere candidate (near root if in range, else far root,
// raytracer.hxx:62-90) and candidates are compared on (t, original index) lexicographically
// — the same minimum whatever order spheres are visited in, so the scene may be reordered
// into spatial clusters. Spheres come 8 at a time: 8 discriminants, one
// max reduction (NaN never wins) and the root work only when some lane needs it.
struct Hit {  // the closest candidate so far as hit_key(t, original index); ~0 = none
    uint64_t key;
    __device__ float t() const { return __uint_as_float((uint32_t)(key >> 32)); }
    __device__ uint32_t id() const { return (uint32_t)key; }
};
constexpr uint64_t kNoHit = 0x7f7fffffffffffffull;  // t = kMAX, index = none
// kNoHit made in VGPRs where it is used: left to itself the allocator keeps the constant in a
// VGPR pair for the whole kernel, and at 7 waves per SIMD (72 VGPRs) spills it to scratch
__device__ __forceinline__ uint64_t no_hit()
{
    uint32_t lo = 0xffffffffu, hi = 0x7f7fffffu;
    asm volatile("" : "+v"(lo), "+v"(hi));
    return ((uint64_t)hi << 32) | lo;
}
// this lane's slot of a per-thread LDS array: the wave's first slot (a scalar) plus the lane
// id, recomputed at each use (keeping threadIdx.x * 16 live across the loop costs a VGPR,
// which at 7 waves per SIMD is spilled to scratch)
__device__ __forceinline__ uint32_t thread_slot(uint32_t wave_base)
{
    uint32_t l;  // the lane id, formed here (the builtins' result is hoisted and kept live)
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return wave_base + l;
}

// Work counters of one wave (wave-uniform, scalar registers): segments traced and the
// lane-level ray-sphere and cluster-box tests executed, summed from ballots in uniform control
// flow (a test the wave runs for k requesting lanes counts k).
// Only the counting instantiation (COUNT, used when the caller asks for the counters) keeps them.
template <bool COUNT>
struct WaveTally {
    uint64_t seg = 0, sph = 0, box = 0;
    __device__ __forceinline__ void add_seg(uint32_t n) { if (COUNT) seg += n; }
    __device__ __forceinline__ void add_sph(uint64_t n) { if (COUNT) sph += n; }
    __device__ __forceinline__ void add_box(uint32_t n) { if (COUNT) box += n; }
};
// t in (kMIN, kMAX), the reference's test (raytracer.hxx:63-64,76-77): positive binary32 values
// are ordered as their bit patterns, and as unsigned integers every negative value and every
// NaN lies outside the open interval of patterns, so one subtract and one compare decide it.
__device__ __forceinline__ bool in_range(float t)
{
    constexpr uint32_t lo = 0x3c03126fu;  // bits of RT_TMIN (0.008f)
    constexpr uint32_t hi = 0x7f7fffffu;  // bits of RT_TMAX (FLT_MAX)
    return __float_as_uint(t) - (lo + 1u) < hi - lo - 1u;
}
// A candidate as a 64-bit key, bits(t) << 32 | original index: for t > 0 (or NaN, which loses to
// every valid t) the unsigned key order is the (t, index) order of closest_hit.
__device__ __forceinline__ uint64_t hit_key(float t, uint32_t id)
{
    return ((uint64_t)__float_as_uint(t) << 32) | id;
}

// ---- the root of a candidate (raytracer.hxx:62-90) -----------------------------------------
// The IEEE forms of sqrtf and of division, as the compiler expands them, scale operands whose
// exponents are extreme and fix up special values; when neither can occur they reduce to shorter
// exact sequences. Per ray segment the divisor a = |d|^2 gets its refined reciprocal once (the
// divisor-only head of the division sequence). fd (wave-uniform) says the short forms give the
// IEEE bits for every lane: the scene lies within 2^19 of the origin (KParams::fast_roots: then
// |oc| <= 2^21 and every in-range root is below 2^43) and every active lane has a in
// [2^-40, 2^40], so no root division needs scaling (quotient exponents stay 96 below the
// numerator's) and every discriminant is below 2^96.
struct RayDiv {
    float a, y;  // divisor |d|^2 and its refined reciprocal
    uint32_t fd; // wave-uniform (a scalar, not a lane predicate): the short forms are exact for every lane
};
__device__ __forceinline__ RayDiv ray_div(float a, uint64_t active, uint32_t fast_roots)
{
    const float y0 = __builtin_amdgcn_rcpf(a);
    const float y = fmaf(fmaf(-a, y0, 1.f), y0, y0);
    const uint64_t ok = ballot(a >= 0x1p-40f) & ballot(a <= 0x1p40f);  // NaN: neither
    return {a, y, (uint32_t)__builtin_amdgcn_readfirstlane((fast_roots != 0u && !(active & ~ok)) ? 1u : 0u)};
}
// n / a: the IEEE sequence (v_div_scale, rcp + refinement, two FMA corrections, v_div_fmas,
// v_div_fixup) with no scaling and no special value, i.e. its two corrections
__device__ __forceinline__ float div_ray(float n, const RayDiv &r)
{
    const float q0 = n * r.y;
    const float q1 = fmaf(fmaf(-r.a, q0, n), r.y, q0);
    return fmaf(fmaf(-r.a, q1, n), r.y, q1);
}
// correctly rounded sqrt for 0 < x < 2^96: the compiler's IEEE expansion (v_sqrt_f32, then the
// one-ulp neighbours checked by FMA residuals) always run on x * 2^32 and scaled back by 2^-16,
// both exact, so the result is that of the expansion's own small-input path for every such x
__device__ __forceinline__ float sqrt_scaled(float x)
{
    const float xs = x * 0x1p32f;
    const float s = __builtin_amdgcn_sqrtf(xs);
    const float sdn = __uint_as_float(__float_as_uint(s) - 1u);
    const float sup = __uint_as_float(__float_as_uint(s) + 1u);
    float r = fmaf(-sdn, s, xs) <= 0.f ? sdn : s;
    r = fmaf(-sup, s, xs) > 0.f ? sup : r;
    return r * 0x1p-16f;
}
// r.fd, re-read as a scalar at each use: left to itself the compiler hoists `fd != 0` out of the
// sphere loops as a lane predicate and rebuilds its negation per use with two VALU operations
__device__ __forceinline__ bool fast_div(const RayDiv &r)
{
    uint32_t f = r.fd;  // uniform by construction (ray_div): an SGPR, no readfirstlane here
    asm volatile("" : "+s"(f));
    return f != 0u;
}
// n / r for the three components of n by the short form, with r's refined reciprocal formed once.
// The caller has checked that no operand takes the IEEE sequence's scaling or fix-up paths:
// |r| in [2^-40, 2^20], of either sign (the hollow ball's radius is negative), every |n_i| in
// [2^-100, 2^21] (so no zero, whose sign the short form can lose, and no quotient below 2^-126).
__device__ __forceinline__ f3 div3_short(f3 n, float r)
{
    const float y0 = __builtin_amdgcn_rcpf(r);
    const RayDiv rr{r, fmaf(fmaf(-r, y0, 1.f), y0, y0), 1u};
    return mk(div_ray(n.x, rr), div_ray(n.y, rr), div_ray(n.z, rr));
}
// every active lane's |n_i| >= 2^-100 (a wave-uniform answer; one min3 and one compare per lane).
// The minimum is IEEE 754-2019's (v_minimum3_f32): a NaN component stays NaN and fails the
// compare, where fminf would drop it and let the lane pass.
__device__ __forceinline__ bool all_lanes_min_abs_ok(f3 n)
{
    const float m = __builtin_elementwise_minimum(__builtin_elementwise_minimum(fabsf(n.x), fabsf(n.y)), fabsf(n.z));
    return !ballot(!(m >= 0x1p-100f));
}
// the near root (-b - sqrt(disc)) / a and its sqrt, raytracer.hxx:62-63; FD: 1 the short forms
// (the caller has branched on fast_div), 0 the IEEE forms, -1 a branch on fast_div here
template <int FD = -1>
__device__ __forceinline__ float near_root(float b, float disc, const RayDiv &r, float &q)
{
    if (FD == 1 || (FD < 0 && fast_div(r))) {
        q = sqrt_scaled(disc);
        return div_ray(-b - q, r);
    }
    q = sqrtf(disc);
    return (-b - q) / r.a;
}
// the far root (-b + sqrt(disc)) / a, raytracer.hxx:76
template <int FD = -1>
__device__ __forceinline__ float far_root(float b, float q, const RayDiv &r)
{
    return (FD == 1 || (FD < 0 && fast_div(r))) ? div_ray(-b + q, r) : (-b + q) / r.a;
}
template <int B> struct IntC { static constexpr int value = B; };

#ifndef RT_GROUND1
#define RT_GROUND1 1
#endif
#ifndef RT_ROOT_HOIST
#define RT_ROOT_HOIST 5  // bit 0: blocks of 8, bit 1: of 4, bit 2: single spheres (8 and 4 together spill)
#endif
template <bool FAST, bool STATS, int N = 8>
__device__ __forceinline__ void test_block8(const float4 *__restrict__ geo, const uint32_t *__restrict__ sidx, uint32_t i,
                                            f3 o, f3 d, const RayDiv &rd, Hit &h, Dbg &dbg)
{
    const float a = rd.a;
    float bq[N], dq[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float4 s = geo[i + k];
        const float ocx = o.x - s.x, ocy = o.y - s.y, ocz = o.z - s.z;       // raytracer.hxx:55
        float b, c;
        if (FAST) {  // contracted: 11 VALU per sphere
            b = fmaf(ocx, d.x, fmaf(ocy, d.y, ocz * d.z));
            c = fmaf(ocx, ocx, fmaf(ocy, ocy, fmaf(ocz, ocz, -s.w)));
            dq[k] = fmaf(b, b, -(a * c));
        } else {     // the reference's rounding, op by op: 17 VALU per sphere
            b = ocx * d.x + ocy * d.y + ocz * d.z;                           // :57
            c = ocx * ocx + ocy * ocy + ocz * ocz - s.w;                     // :58
            dq[k] = b * b - a * c;                                           // :60
        }
        bq[k] = b;
        if (N == 1) {
            // The always-tested spheres (the ground): a ray leaving the sphere (b > 0) from
            // outside it (c >= 0) has no candidate unless rounding makes the far root reach
            // kMIN: with a c >= 0 the discriminant is at most RN(b^2), so its correctly rounded
            // root q is at most b + ulp(b), the near root is negative and the far root
            // RN((q - b) / a) <= RN(ulp(b) / a) < kMIN when b 2^-22 < kMIN a. Such lanes need
            // no root work: their discriminant is set to -1 (no candidate, as computed), and a
            // wave of them (upward rays from above the ground: the sky) skips it.
            if (b > 0.f && c >= 0.f && b * 0x1p-22f < RT_TMIN * a) dq[k] = -1.f;
        }
    }
    // pairwise max tree (NaN never wins)
    float mq[N];
#pragma unroll
    for (int k = 0; k < N; ++k) mq[k] = dq[k];
#pragma unroll
    for (int w = N / 2; w >= 1; w /= 2)
#pragma unroll
        for (int k = 0; k < w; ++k) mq[k] = fmaxf(mq[k], mq[k + w]);
    // Wave-uniform branches (ballots) around the root work, lane selects inside: a masked
    // lane costs the same issue slots as a computing one, and uniform branches need no
    // exec-mask save/restore. Lanes without a positive discriminant take the root of -1
    // (NaN), so their candidate is NaN, whose key never wins (NaN bits order above every
    // finite t): no predicate is carried to the key update, which is selected by the key
    // compare alone. (Formed as `pos && kt < h.key`, the mask would be ANDed into VCC by a
    // scalar op, and a VALU read of a VCC that a scalar op wrote stalls ~20 cycles on gfx950,
    // scripts/ubench_int.hip.)
    // The root form is chosen once for the block's roots (one uniform branch, not one per root)
    auto roots = [&](auto fdc) {
        constexpr int FD = decltype(fdc)::value;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const bool pos = dq[k] > 0.f;                                    // :62
            const uint64_t posm = ballot(pos);
            if (posm) {
                if (STATS) { dbg.lane_roots += pos; if (first_active_lane()) ++dbg.wave_roots; }
                const float dk = pos ? dq[k] : -1.f;
                float q;
                float t = near_root<FD>(bq[k], dk, rd, q);                   // :63
                const bool ok = in_range(t);
                if (posm & ~ballot(ok)) {
                    const float t2 = far_root<FD>(bq[k], q, rd);             // :76
                    t = ok ? t : (in_range(t2) ? t2 : __builtin_nanf(""));
                } else {
                    t = ok ? t : __builtin_nanf("");
                }
                const uint64_t kt = hit_key(t, sidx[i + k]);
                if (kt < h.key) h.key = kt;
            }
        }
    };
    if (ballot(mq[0] > 0.f)) {
        if (STATS) { ++dbg.lane_blocks; if (first_active_lane()) ++dbg.wave_blocks; }
        constexpr bool hoist = (RT_ROOT_HOIST >> (N == 8 ? 0 : N == 4 ? 1 : 2)) & 1;
        if (hoist && fast_div(rd)) roots(IntC<1>{});
        else roots(IntC<hoist ? 0 : -1>{});
    }
}

// Cluster culling: a lane tests a cluster's spheres only if its ray segment (kMIN, t_best]
// can reach the cluster's AABB grown by a pad that dominates every float error involved
// (1e-3 x (|o|_1 + max_c(|C|_1 + |e|_1)) against errors below 3e-4 of that),
// so a culled cluster never holds a sphere whose exact candidate could win: same bits.
#define RT_PAD_REL 1e-3f

// a list of spheres: blocks of 8, then 4, then single spheres (cluster member counts are
// multiples of 4; the always-tested list has its exact count, e.g. 1 for the ground)
template <bool FAST, bool STATS>
__device__ __forceinline__ void run_members(const float4 *__restrict__ geo, const uint32_t *__restrict__ sidx,
                                            uint32_t start, uint32_t cnt, f3 o, f3 d, const RayDiv &rd, Hit &h,
                                            Dbg &dbg)
{
    const uint32_t end = start + cnt;
    uint32_t i = start;
    for (; i + 8 <= end; i += 8) test_block8<FAST, STATS>(geo, sidx, i, o, d, rd, h, dbg);
    if (i + 4 <= end) { test_block8<FAST, STATS, 4>(geo, sidx, i, o, d, rd, h, dbg); i += 4; }
    for (; i < end; ++i) test_block8<FAST, STATS, 1>(geo, sidx, i, o, d, rd, h, dbg);
}

struct RayBox {  // per-segment constants of the padded slab test
    float ix, iy, iz, oix, oiy, oiz, aix, aiy, aiz, px, py, pz;
};
__device__ __forceinline__ bool box_pass(const RayBox &r, float4 c0, float4 c1, float t_lo, float t_hi)
{
    const float hx = fmaf(c0.w, r.aix, r.px), hy = fmaf(c1.x, r.aiy, r.py), hz = fmaf(c1.y, r.aiz, r.pz);
    const float tcx = fmaf(c0.x, r.ix, -r.oix), tcy = fmaf(c0.y, r.iy, -r.oiy), tcz = fmaf(c0.z, r.iz, -r.oiz);
    // tin <= tout && tout >= t_lo && tin <= t_hi, with t_lo < t_hi (no NaN arises: every
    // operand is finite or an infinity of one sign)
    const float tin = fmaxf(fmaxf(fmaxf(tcx - hx, tcy - hy), tcz - hz), t_lo);
    const float tout = fminf(fminf(fminf(tcx + hx, tcy + hy), tcz + hz), t_hi);
    return tin <= tout;
}

// Structure 7: the members of a passing cluster, tested transposed. A wave walks the union of
// its lanes' passing clusters, and in structure 5 every lane then runs the cluster's 16 tests
// while only the lanes whose segment reaches the cluster keep the results (20% of the lanes on
// config 3). Here, when at most kTransposeMax lanes request a cluster, all 64 lanes of the wave
// test (requesting ray, member) pairs instead — 4 rays x 16 members per round — and each
// ray's minimum over its 16 lanes comes back to its lane. Every pair yields the reference's
// per-sphere candidate (near root if in range, else far root, raytracer.hxx:62-90), and the
// candidates are combined by the (t, original index) minimum as key = bits(t) << 32 | index
// (t > 0, so the u64 order is that order): the same hit, in any order. Whole-wave code.
#ifndef RT_TRANSPOSE_LDS
#define RT_TRANSPOSE_LDS 16  // rays per transposed cluster the per-wave LDS holds
#endif
constexpr uint32_t kTransposeMax = RT_TRANSPOSE_LDS;  // KParams::transpose_max is clamped to this
// unsigned minimum over each row of 16 lanes: xor 1, xor 2 (quad permutes), then the half-row
// mirror and the row mirror leave every lane of a row with the row's minimum
// (the DPP moves carry the identity of min as their old value, so the compiler folds each into
// its v_min_u32 as a DPP operand)
__device__ __forceinline__ uint32_t min16_u32(uint32_t v)
{
#define RT_DPP_MIN(ctrl) v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, ctrl, 0xf, 0xf, false))
    RT_DPP_MIN(0xB1);
    RT_DPP_MIN(0x4E);
    RT_DPP_MIN(0x141);
    RT_DPP_MIN(0x140);
#undef RT_DPP_MIN
    return v;
}
// minimum key over each row of 16 lanes, in two 32-bit passes: the smallest t (as bits), then the
// smallest index among the lanes holding that t
__device__ __forceinline__ uint64_t min16_key(uint64_t k)
{
    const uint32_t tb = (uint32_t)(k >> 32);
    const uint32_t tm = min16_u32(tb);
    const uint32_t im = min16_u32(tb == tm ? (uint32_t)k : 0xffffffffu);
    return ((uint64_t)tm << 32) | im;
}
// per-wave LDS of the transposed tests: the requesting rays by rank; a ray's minimum key comes
// back in the last two words of its first record once its round is done (the round's rows read
// their rays before any row writes a key, and later rounds read other rays)
#ifndef RT_TKEY_SEPARATE
#define RT_TKEY_SEPARATE 0  // A/B build switch: the rows' keys in an array of their own (512 B more per workgroup)
#endif
struct TransposeLds {
    float4 ray[kTransposeMax][2];   // {o.x, o.y, o.z | key lo, a | key hi}, {d.x, d.y, d.z, refined 1/a}
#if RT_TKEY_SEPARATE
    uint64_t key[kTransposeMax];
#endif
};
template <bool FAST, bool STATS>
__device__ __forceinline__ void members_transposed(const float4 *__restrict__ geo, const uint32_t *__restrict__ sidx,
                                                   uint32_t start, uint32_t cnt, uint64_t M, bool req,
                                                   TransposeLds *tw, f3 o, f3 d, const RayDiv &rd, Hit &h,
                                                   Dbg &dbg)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t m = (uint32_t)__popcll(M);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(M >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)M, 0u));
    if (req) {
        tw->ray[rank][0] = make_float4(o.x, o.y, o.z, rd.a);
        tw->ray[rank][1] = make_float4(d.x, d.y, d.z, rd.y);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t k = lane & 15u;          // member slot (slots >= cnt read beyond: masked)
    const float kth = k < cnt ? 0.f : __builtin_inff();  // slots past the cluster never test positive
    const float4 s = geo[start + k];
    const uint32_t sid = sidx[start + k];
    for (uint32_t r0 = 0; r0 < m; r0 += 4u) {
        RT_EV(EV_T_ROUND);
        const uint32_t r = r0 + (lane >> 4);
        const uint32_t rr = min(r, m - 1u);  // rows r >= m repeat ray m - 1; their keys are not stored
        const float4 q0 = tw->ray[rr][0], q1 = tw->ray[rr][1];
        const float ra = q0.w;                                              // |d|^2, as closest_hit
        const RayDiv rdr{ra, q1.w, rd.fd};
        const float ocx = q0.x - s.x, ocy = q0.y - s.y, ocz = q0.z - s.z;  // raytracer.hxx:55
        float b, disc;
        if (FAST) {
            b = fmaf(ocx, q1.x, fmaf(ocy, q1.y, ocz * q1.z));
            const float c = fmaf(ocx, ocx, fmaf(ocy, ocy, fmaf(ocz, ocz, -s.w)));
            disc = fmaf(b, b, -(ra * c));
        } else {
            b = ocx * q1.x + ocy * q1.y + ocz * q1.z;                     // :57
            const float c = ocx * ocx + ocy * ocy + ocz * ocz - s.w;     // :58
            disc = b * b - ra * c;                                         // :60
        }
        const bool pos = disc > kth;                                       // :62
        const uint64_t posm = ballot(pos);
        uint64_t key = ~0ull;
        if (posm) {
            const float dk = pos ? disc : -1.f;  // NaN candidate without a positive discriminant
            float q;
            float t = near_root(b, dk, rdr, q);                            // :63
            const bool ok = in_range(t);
            if (posm & ~ballot(ok)) {
                RT_EV(EV_T_FAR);
                const float t2 = far_root(b, q, rdr);                      // :76
                t = ok ? t : (in_range(t2) ? t2 : __builtin_nanf(""));
            } else {
                t = ok ? t : __builtin_nanf("");
            }
            // NaN keys (no candidate) lose to every valid key in the row minimum and in the
            // owner's update, like ~0 (test_block8)
            key = hit_key(t, sid);
        }
        key = min16_key(key);
        if (k == 0u && r < m) {
#if RT_TKEY_SEPARATE
            tw->key[r] = key;
#else
            tw->ray[r][0].z = __uint_as_float((uint32_t)key);
            tw->ray[r][0].w = __uint_as_float((uint32_t)(key >> 32));
#endif
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (req) {
#if RT_TKEY_SEPARATE
        const uint64_t kk = tw->key[rank];
#else
        const float4 q = tw->ray[rank][0];
        const uint64_t kk = ((uint64_t)__float_as_uint(q.w) << 32) | __float_as_uint(q.z);
#endif
        if (kk < h.key) h.key = kk;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <bool FAST, bool STATS, bool COUNT>
__device__ __forceinline__ void cluster_members7(bool req, uint64_t M, uint32_t scu_lane, const float4 *__restrict__ geo,
                                                 const uint32_t *__restrict__ sidx, TransposeLds *tw, uint32_t tmax,
                                                 f3 o, f3 d, const RayDiv &rd, Hit &h, Dbg &dbg, WaveTally<COUNT> &wt)
{
    // req: this lane's segment reaches the cluster box; M: the wave's mask of such lanes
    if (!M) return;
    RT_EV(EV_CLUSTER_REQ);
    const uint32_t scu = __builtin_amdgcn_readfirstlane(scu_lane);
    const uint32_t start = scu & 0xffffu, cnt = scu >> 16;
    wt.add_sph((uint64_t)__popcll(M) * cnt);
    if ((uint32_t)__popcll(M) <= min(tmax, kTransposeMax) && cnt <= 16u) {
        RT_EV(EV_TRANSPOSED);
        members_transposed<FAST, STATS>(geo, sidx, start, cnt, M, req, tw, o, d, rd, h, dbg);
    } else if (req) {
        RT_EV(EV_PER_LANE_MEMBERS);
        if (STATS && first_active_lane()) dbg.wave_member_blocks += (cnt + 7) / 8;
        run_members<FAST, STATS>(geo, sidx, start, cnt, o, d, rd, h, dbg);
    }
}

// One sphere's candidate for this lane's segment (raytracer.hxx:55-90, the op sequence of
// test_block8 on its geo entry {C, fl(r r)}) as a key, no_hit() without one. want: this lane
// asks (the others compute along and get no_hit()); t: the candidate's t when the key is valid.
template <bool FAST>
__device__ __forceinline__ uint64_t sphere_key(bool want, float4 s, uint32_t id, f3 o, f3 d, const RayDiv &rd, float &t)
{
    const float a = rd.a;
    const float ocx = o.x - s.x, ocy = o.y - s.y, ocz = o.z - s.z;            // raytracer.hxx:55
    float b, disc;
    if (FAST) {
        b = fmaf(ocx, d.x, fmaf(ocy, d.y, ocz * d.z));
        const float c = fmaf(ocx, ocx, fmaf(ocy, ocy, fmaf(ocz, ocz, -s.w)));
        disc = fmaf(b, b, -(a * c));
    } else {
        b = ocx * d.x + ocy * d.y + ocz * d.z;                               // :57
        const float c = ocx * ocx + ocy * ocy + ocz * ocz - s.w;             // :58
        disc = b * b - a * c;                                                // :60
    }
    const bool pos = want && disc > 0.f;                                     // :62
    const uint64_t posm = ballot(pos);
    t = 0.f;
    if (!posm) return no_hit();
    const float dk = pos ? disc : -1.f;  // NaN candidate without a positive discriminant
    float q;
    t = near_root(b, dk, rd, q);                                             // :63
    const bool ok = in_range(t);
    if (posm & ~ballot(ok)) {
        const float t2 = far_root(b, q, rd);                                 // :76
        t = ok ? t : (in_range(t2) ? t2 : __builtin_nanf(""));
    } else {
        t = ok ? t : __builtin_nanf("");
    }
    const uint64_t kt = hit_key(t, id);
    const uint64_t none = no_hit();
    return kt < none ? kt : none;  // a NaN key (no candidate) orders above kNoHit: none then
}

// The sphere a path last refracted into or reflected off inside (a dielectric hit), tested
// first: a ray trapped in a small glass sphere (the reference's refract, raytracer.hxx:158-194,
// keeps 0.17% of the samples bouncing up to max_depth, nearly all inside small dielectric
// spheres) then starts the walk with t_best at that sphere's far wall, and the padded boxes of
// every cluster its short segment does not reach are culled. The candidate is the reference's,
// so the (t, index) minimum is unchanged when the walk meets the sphere again. hint: this lane's
// last hit was a dielectric sphere, whose geo entry, original index (hid; kShortcut: the sphere
// has a shortcut word) and shortcut word (nbw) wait in the lane's LDS slots.
//
// The shortcut (rt_host_build.cpp shortcut_words; KParams::iso): when the segment (0, 1.002 t] up to
// the sphere's own candidate t lies in the ball |p - C|^2 <= fl(r r) kIsoR2Grow (both ends
// checked; the ball is convex), the host has shown that it misses the padded box of every
// clustered sphere but the sphere's at most two neighbours (none: "isolated"), whose slots nbw
// holds: the lane tests them here and needs no walk (`skip`; the always-tested spheres are still
// tested). A ray trapped in a small glass ball takes this path for every bounce.
//
// The neighbour slots of a lane that does not test a neighbour are 0, not its word's: a lane's
// word may be stale (left by an earlier path) or, before the lane's first dielectric hit, whatever
// the LDS held — bounded by that lane's own `skip` since fd383c3. The instrumented kernel (STATS)
// checks the slot against n_geo, starts every lane's word at 0x3fffffff (slots past any blob, no list), and
// with `unbounded` (KParams::diag_unbounded_nb) forms it the old way, so the check fires
// (tests/test_gpu_parity.py test_neighbour_slots_are_bounded).
template <bool FAST, bool STATS>
__device__ __forceinline__ uint64_t hint_candidate(bool hint, float4 s, uint32_t hid, uint32_t nbw,
                                                   const float4 *__restrict__ geo, const uint32_t *__restrict__ sidx,
                                                   f3 o, f3 d, const RayDiv &rd, uint32_t iso, bool &skip,
                                                   uint32_t n_geo, uint32_t unbounded, unsigned long long *dbg)
{
    skip = false;
    float t;
    uint64_t key = sphere_key<FAST>(hint, s, hid & 0x7fffffffu, o, d, rd, t);
    if (iso && ballot(key < no_hit() && (int32_t)hid < 0)) {
        // a valid key implies hint; t then is finite and in range
        const float ocx = o.x - s.x, ocy = o.y - s.y, ocz = o.z - s.z;
        const float tq = t * 1.002f;  // the walk's bound, h.t() * 1.002f
        const float qx = fmaf(tq, d.x, ocx), qy = fmaf(tq, d.y, ocy), qz = fmaf(tq, d.z, ocz);
        const float r2k = s.w * kIsoR2Grow;
        const float o2 = ocx * ocx + ocy * ocy + ocz * ocz;
        const float q2 = qx * qx + qy * qy + qz * qz;
        skip = (int32_t)hid < 0 && key < no_hit() && o2 <= r2k && q2 <= r2k;
        // the neighbours (geo slots + 1 in nbw), tested by the lanes that skip the walk
        const uint32_t n0 = nbw & 0x7fffu, n1 = (nbw >> 15) & 0x7fffu;
        // (lanes that do not test a neighbour read slot 0: their word may be stale)
        if (ballot(skip && n0 != 0u)) {
            uint32_t g = (STATS && unbounded) ? (n0 ? n0 - 1u : 0u) : (skip && n0 ? n0 - 1u : 0u);
            g = checked<STATS>(g, n_geo, BC_HINT_NB, dbg);
            const uint64_t k = sphere_key<FAST>(skip && n0 != 0u, geo[g], sidx[g], o, d, rd, t);
            if (k < key) key = k;
        }
        if (ballot(skip && n1 != 0u)) {
            uint32_t g = (STATS && unbounded) ? (n1 ? n1 - 1u : 0u) : (skip && n1 ? n1 - 1u : 0u);
            g = checked<STATS>(g, n_geo, BC_HINT_NB, dbg);
            const uint64_t k = sphere_key<FAST>(skip && n1 != 0u, geo[g], sidx[g], o, d, rd, t);
            if (k < key) key = k;
        }
    }
    return key;
}

template <bool FAST, int CULL, bool STATS, bool COUNT, class KP>
__device__ __forceinline__ Hit closest_hit(const KP &p, const float4 *__restrict__ geo,
                                           const uint32_t *__restrict__ sidx, const float4 *__restrict__ clus, f3 o,
                                           f3 d, const RayDiv &rd, Dbg &dbg, WaveTally<COUNT> &wt, bool active,
                                           uint64_t am, TransposeLds *tw, uint64_t key0)
{
    // active: this lane traces a segment; am: the wave's mask of such lanes; key0: a candidate
    // already found for this segment (hint_candidate) or no_hit()
    Hit h{key0};
    // one always-tested sphere (the ground of the reference's scenes): its block without the
    // list's loop control
    if (RT_GROUND1 && p.n_always == 1u) test_block8<FAST, STATS, 1>(geo, sidx, 0, o, d, rd, h, dbg);
    else run_members<FAST, STATS>(geo, sidx, 0, p.n_always, o, d, rd, h, dbg);
    if (CULL) {
        // 1/x with its magnitude clamped to 1e30 (one med3; |x| < 1e-30 behaves as 1e-30 of
        // the same sign, zeros included): products with coordinates stay finite
        auto safe_rcp = [](float x) { return __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(x), -1e30f, 1e30f); };
        const float ix = safe_rcp(d.x), iy = safe_rcp(d.y), iz = safe_rcp(d.z);
        const float oix = o.x * ix, oiy = o.y * iy, oiz = o.z * iz;
        const float aix = fabsf(ix), aiy = fabsf(iy), aiz = fabsf(iz);
        const float pad = fmaf(RT_PAD_REL, fabsf(o.x) + fabsf(o.y) + fabsf(o.z), p.clus_pad);
        const float px = pad * aix, py = pad * aiy, pz = pad * aiz;
        const float t_lo = 0.5f * RT_TMIN;
        // Two levels under a root box, with whole-wave control (lanes predicated by `active`) so
        // that every lane can take part in a cluster's transposed member tests: the level-3 box
        // over every cluster gates the walk (a ray that misses the padded union box misses every
        // padded box inside it), a level-2 box covers kSuperClusters (8) consecutive clusters, and a passing
        // level-2 box's cluster boxes are tested in pairs against the current t_best.
        const RayBox rb{ix, iy, iz, oix, oiy, oiz, aix, aiy, aiz, px, py, pz};
        const float4 *sup = clus + (p.supers_offset - p.clus_offset);
        uint32_t n_supers = p.n_supers;
        if (!am) {
            n_supers = 0;  // every lane's segment is settled (isolated hint spheres)
        } else if (p.use_root) {
            wt.add_box(lanes(active));
            if (!(ballot(box_pass(rb, sup[2 * p.n_supers], sup[2 * p.n_supers + 1], t_lo, h.t() * 1.002f)) & am))
                n_supers = 0;
        }
        if (n_supers) RT_EV(EV_ROOT_GATE_PASS);
        for (uint32_t g = 0; g < n_supers; ++g) {
            RT_EV(EV_SUPER);
            const float4 s0 = sup[2 * g], s1 = sup[2 * g + 1];
            wt.add_box(lanes(active));
            const bool bs = box_pass(rb, s0, s1, t_lo, h.t() * 1.002f);
            const uint64_t spm = ballot(bs) & am;
            if (!spm) continue;
            const bool sp = bs & active;
            RT_EV(EV_SUPER_PASS);
            // its first cluster and the count the walk tests (up to its last non-empty one)
            const uint32_t sw = __builtin_amdgcn_readfirstlane(__float_as_uint(s1.w)), c0i = sw & 0xffffu, cn = sw >> 16;
            wt.add_box(cn * (uint32_t)__popcll(spm));
            for (uint32_t c = c0i; c < c0i + cn; c += 2) {
                const float tb_now = h.t() * 1.002f;
                const float4 a0 = clus[2 * c], a1 = clus[2 * c + 1], b0 = clus[2 * c + 2], b1 = clus[2 * c + 3];
                const bool ba = box_pass(rb, a0, a1, t_lo, tb_now), bb = box_pass(rb, b0, b1, t_lo, tb_now);
                const uint64_t pam = ballot(ba) & spm, pbm = ballot(bb) & spm;
                cluster_members7<FAST, STATS, COUNT>(ba & sp, pam, __float_as_uint(a1.w), geo, sidx, tw, p.transpose_max, o,
                                                     d, rd, h, dbg, wt);
                cluster_members7<FAST, STATS, COUNT>(bb & sp, pbm, __float_as_uint(b1.w), geo, sidx, tw, p.transpose_max, o,
                                                     d, rd, h, dbg, wt);
            }
        }
    }
    return h;
}

// p[i] read from global memory, named as such (a float4 load from address space 1)
__device__ __forceinline__ float4 gld4(const float4 *p, uint32_t i)
{
    const __attribute__((address_space(1))) float *g = (const __attribute__((address_space(1))) float *)(p + i);
    return make_float4(g[0], g[1], g[2], g[3]);
}

} // namespace rt
