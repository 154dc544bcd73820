// TEST INFRASTRUCTURE ONLY: one small kernel per device function of rt_trace.h, so that the suite
// can run the product's own short exact forms by themselves on the device
// (tests/test_primitives_gpu.py through tests/tools/probe.py). Nothing here restates a function:
// every kernel instantiates rt_trace.h's. Built by csrc/Makefile (target `probe`) with the
// product's flags, -ffp-contract=off included, into tests/device/librt_probe.so.
//
// Every probe has one shape: rt_probe_<name>(in, out, n, arg, stream) launches n / 64 whole waves
// (n a positive multiple of 64, else hipErrorInvalidValue and no launch) on `stream` and returns
// hipGetLastError(). in and out are device arrays of 32-bit words, laid out as planes [plane][n]
// (element i of plane p at p * n + i; a 64-bit value takes two planes, low word first); lane i of
// the grid reads and writes element i of every plane and nothing else. The caller owns the
// arrays: no allocation and no synchronisation here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_trace.h"
#include "rt_host_build.h"

using namespace rt;

namespace {

struct Io {
    const uint32_t *in;
    uint32_t *out;
    uint32_t n, i;
    __device__ uint32_t u(uint32_t p) const { return in[(size_t)p * n + i]; }
    __device__ float f(uint32_t p) const { return __uint_as_float(u(p)); }
    __device__ uint64_t u64(uint32_t p) const { return ((uint64_t)u(p + 1) << 32) | u(p); }
    __device__ f3 v(uint32_t p) const { return mk(f(p), f(p + 1), f(p + 2)); }
    __device__ void u(uint32_t p, uint32_t x) const { out[(size_t)p * n + i] = x; }
    __device__ void f(uint32_t p, float x) const { u(p, __float_as_uint(x)); }
    __device__ void u64(uint32_t p, uint64_t x) const { u(p, (uint32_t)x); u(p + 1, (uint32_t)(x >> 32)); }
    __device__ void v(uint32_t p, f3 x) const { f(p, x.x); f(p + 1, x.y); f(p + 2, x.z); }
};

} // namespace

// the kernel k_<name>(io, arg) and its launcher rt_probe_<name>; one wave per workgroup
#define RT_PROBE(name)                                                                                      \
    __device__ __forceinline__ void body_##name(const Io &io, uint32_t arg);                                \
    __global__ __launch_bounds__(64) void k_##name(const uint32_t *in, uint32_t *out, uint32_t n, uint32_t arg) \
    {                                                                                                       \
        const uint32_t i = blockIdx.x * 64u + threadIdx.x;                                                  \
        if (i < n) body_##name(Io{in, out, n, i}, arg); /* n is a multiple of 64: a wave is whole or absent */ \
    }                                                                                                       \
    extern "C" int rt_probe_##name(const void *in, void *out, uint32_t n, uint32_t arg, void *stream)       \
    {                                                                                                       \
        if (!in || !out || n == 0u || n % 64u != 0u) return (int)hipErrorInvalidValue;                      \
        hipLaunchKernelGGL(k_##name, dim3(n / 64u), dim3(64u), 0, static_cast<hipStream_t>(stream),         \
                           static_cast<const uint32_t *>(in), static_cast<uint32_t *>(out), n, arg);       \
        return (int)hipGetLastError();                                                                      \
    }                                                                                                       \
    __device__ __forceinline__ void body_##name(const Io &io, uint32_t arg)

// in: x | out: sqrt_scaled(x)
RT_PROBE(sqrt_scaled) { io.f(0, sqrt_scaled(io.f(0))); }

// in: a, active (0 / 1), n | arg: fast_roots | out: fd, div_ray(n, rd), rd.y of rd = ray_div(a, mask of active, arg)
RT_PROBE(ray_div)
{
    const RayDiv rd = ray_div(io.f(0), ballot(io.u(1) != 0u), arg);
    io.u(0, rd.fd);
    io.f(1, div_ray(io.f(2), rd));
    io.f(2, rd.y);
}

// in: b, disc, a | out: near_root<1>, its q, far_root<1>, near_root<0>, its q, far_root<0>
RT_PROBE(roots)
{
    const float b = io.f(0), disc = io.f(1);
    const RayDiv rd = ray_div(io.f(2), ~0ull, 1u);
    float q1, q0;
    const float n1 = near_root<1>(b, disc, rd, q1);
    const float n0 = near_root<0>(b, disc, rd, q0);
    io.f(0, n1); io.f(1, q1); io.f(2, far_root<1>(b, q1, rd));
    io.f(3, n0); io.f(4, q0); io.f(5, far_root<0>(b, q0, rd));
}

// in: n.xyz, r, active (0 / 1) | arg: 1 = the divisor is sqrt_scaled(r) (the kernel's d / |d|)
// out: all_lanes_min_abs_ok(n) as the active lanes see it (2 in an inactive lane), div3_short(n, r)
RT_PROBE(div3)
{
    const f3 n = io.v(0);
    uint32_t vote = 2u;
    f3 s = mk(0.f, 0.f, 0.f);
    if (io.u(4) != 0u) {
        vote = all_lanes_min_abs_ok(n) ? 1u : 0u;
        s = div3_short(n, arg ? sqrt_scaled(io.f(3)) : io.f(3));
    }
    io.u(0, vote);
    io.v(1, s);
}

// in: a, b, rb, fast (0 / 1) | out: div_const(a, b, rb, fast)
RT_PROBE(div_const) { io.f(0, div_const(io.f(0), io.f(1), io.f(2), io.u(3) != 0u)); }

// in: want (0 / 1), s.xyzw, id, o.xyz, d.xyz | arg: fast_roots | out: sphere_key<false> (2 words), fd
RT_PROBE(sphere_key)
{
    const f3 d = io.v(9);
    const float a = d.x * d.x + d.y * d.y + d.z * d.z;  // as the render loop forms it
    const RayDiv rd = ray_div(a, ~0ull, arg);
    float t;
    const uint64_t k = sphere_key<false>(io.u(0) != 0u, make_float4(io.f(1), io.f(2), io.f(3), io.f(4)), io.u(5),
                                         io.v(6), d, rd, t);
    io.u64(0, k);
    io.u(2, rd.fd);
}

// in: bits of t, id | out: in_range(t), hit_key(t, id) (2 words)
RT_PROBE(in_range)
{
    io.u(0, in_range(io.f(0)) ? 1u : 0u);
    io.u64(1, hit_key(io.f(0), io.u(1)));
}

// in: key (2 words) | out: min16_key(key) (2 words)
RT_PROBE(min16_key) { io.u64(0, min16_key(io.u64(0))); }

// in: initstate (2), inc (2) | arg: draws m <= 16 | out: m words of pcg_next from pcg_seed, then the state (2)
RT_PROBE(pcg_stream)
{
    const uint64_t inc = io.u64(2);
    const uint32_t m = arg < 16u ? arg : 16u;  // out has m + 2 planes
    uint64_t st = pcg_seed(io.u64(0), inc);
    for (uint32_t j = 0; j < m; ++j) io.u(j, pcg_next(st, inc));
    io.u64(m, st);
}

// in: state (2), inc (2) | arg: 0 canonical, 1 canonical_pm1 | out: the draw, the state after it (2)
RT_PROBE(canonical)
{
    uint64_t st = io.u64(0);
    const uint64_t inc = io.u64(2);
    io.f(0, arg ? canonical_pm1(st, inc) : canonical(st, inc));
    io.u64(1, st);
}

// in: state (2), inc (2) | out: random_in_unit_sphere_capped<false, 4> resumed call after call until it
// accepts (at most 8 calls): p.xyz, state (2), calls; then random_in_unit_sphere: p.xyz, state (2)
RT_PROBE(unit_sphere)
{
    const uint64_t inc = io.u64(2);
    uint64_t st = io.u64(0);
    Dbg dbg{};
    bool got = false;
    uint32_t calls = 0;
    f3 p = mk(0.f, 0.f, 0.f);
    while (!got && calls < 8u) {
        p = random_in_unit_sphere_capped<false, 4>(st, inc, got, dbg);
        ++calls;
    }
    io.v(0, p);
    io.u64(3, st);
    io.u(5, got ? calls : 0u);
    uint64_t su = io.u64(0);
    io.v(6, random_in_unit_sphere(su, inc));
    io.u64(9, su);
}

// in: I.xyz, N.xyz, eta | out: refract(I, N, eta)
RT_PROBE(refract) { io.v(0, refract(io.v(0), io.v(3), io.f(6))); }

// in: v.xyz | out: normalize(v)
RT_PROBE(normalize) { io.v(0, normalize(io.v(0))); }

// in: xf, c | out: schlick_x(xf, c)
RT_PROBE(schlick_x) { io.f(0, schlick_x(io.f(0), io.f(1))); }

// in: n, then the divisor's UDiv {m, s1, s2} | out: udiv(n, u)
RT_PROBE(udiv)
{
    const UDiv u{io.u(1), io.u(2), io.u(3)};
    io.u(0, udiv(io.u(0), u));
}

// the host's side of div_const and udiv (rt_host_build.cpp)
extern "C" int rt_probe_exact_by_reciprocal(float b) { return rthost::exact_by_reciprocal(b) ? 1 : 0; }
extern "C" void rt_probe_make_udiv(uint32_t d, uint32_t *m, uint32_t *s1, uint32_t *s2)
{
    const UDiv u = rthost::make_udiv(d);
    *m = u.m;
    *s1 = u.s1;
    *s2 = u.s2;
}
