// TEST INFRASTRUCTURE ONLY: host restatements of rt_trace.h's short exact sequences, op for op with
// std::fma, for tests/test_primitives_cpu.py (built on first use by tests/tools/probe_cases.py with
// g++ -ffp-contract=off -mfma). Where the device sequence starts from a hardware approximation
// (v_rcp_f32, v_sqrt_f32: 1 ulp promised, no value), `off` picks the seed: the correctly rounded
// value (0) or its neighbour one ulp below (-1) or above (+1), so that a proof checked here does not
// rest on which of them the hardware returns.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace {
float ulps(float x, int off)
{
    uint32_t b;
    std::memcpy(&b, &x, 4);
    b += static_cast<uint32_t>(off);
    std::memcpy(&x, &b, 4);
    return x;
}
} // namespace

extern "C" {

// ray_div's refined reciprocal
void ph_rcp(const float *a, size_t cnt, int off, float *out)
{
    for (size_t i = 0; i < cnt; ++i) {
        const float y0 = ulps(1.f / a[i], off);
        out[i] = std::fma(std::fma(-a[i], y0, 1.f), y0, y0);
    }
}

// ray_div's refined reciprocal and div_ray's two corrections (also div3_short), the gate ignored
void ph_div(const float *n, const float *a, size_t cnt, int off, float *out)
{
    for (size_t i = 0; i < cnt; ++i) {
        const float y0 = ulps(1.f / a[i], off);
        const float y = std::fma(std::fma(-a[i], y0, 1.f), y0, y0);
        const float q0 = n[i] * y;
        const float q1 = std::fma(std::fma(-a[i], q0, n[i]), y, q0);
        out[i] = std::fma(std::fma(-a[i], q1, n[i]), y, q1);
    }
}

// the same with div_ray's second correction left out: what the tables must tell from ph_div
void ph_div_one_correction(const float *n, const float *a, size_t cnt, int off, float *out)
{
    for (size_t i = 0; i < cnt; ++i) {
        const float y0 = ulps(1.f / a[i], off);
        const float y = std::fma(std::fma(-a[i], y0, 1.f), y0, y0);
        const float q0 = n[i] * y;
        out[i] = std::fma(std::fma(-a[i], q0, n[i]), y, q0);
    }
}

void ph_sqrt(const float *x, size_t cnt, int off, float *out)
{
    for (size_t i = 0; i < cnt; ++i) {
        const float xs = x[i] * 0x1p32f;
        const float s = ulps(std::sqrt(xs), off);
        const float sdn = ulps(s, -1), sup = ulps(s, 1);
        float r = std::fma(-sdn, s, xs) <= 0.f ? sdn : s;
        r = std::fma(-sup, s, xs) > 0.f ? sup : r;
        out[i] = r * 0x1p-16f;
    }
}

void ph_div_const(const float *a, const float *b, const float *rb, size_t cnt, float *out)
{
    for (size_t i = 0; i < cnt; ++i) {
        const float q0 = a[i] * rb[i];
        out[i] = std::fma(std::fma(-q0, b[i], a[i]), rb[i], q0);
    }
}

void ph_schlick(const float *xf, const float *c, size_t cnt, float *out)
{
    for (size_t i = 0; i < cnt; ++i) {
        const double x = xf[i], r0 = x * x, y = static_cast<double>(1.f - c[i]);
        const double y2 = y * y, y4 = y2 * y2, y4lo = std::fma(y2, y2, -y4);
        const double y5 = std::fma(y4, y, y4lo * y);
        out[i] = static_cast<float>(r0 + (1.0 - r0) * y5);
    }
}

// the reference's own form, with the C library's pow
void ph_schlick_pow(const float *xf, const float *c, size_t cnt, float *out)
{
    for (size_t i = 0; i < cnt; ++i) {
        const double r0 = std::pow(static_cast<double>(xf[i]), 2);
        out[i] = static_cast<float>(r0 + (1.0 - r0) * std::pow(static_cast<double>(1.f - c[i]), 5));
    }
}

void ph_canonical(const uint32_t *w, size_t cnt, float *c, float *pm1)
{
    for (size_t i = 0; i < cnt; ++i) {
        const float f = std::fmin(static_cast<float>(w[i]), 0x1.fffffep31f);
        c[i] = f * 0x1p-32f;
        pm1[i] = std::fma(f, 0x1p-31f, -1.f);
    }
}

void ph_in_range(const uint32_t *t, size_t cnt, uint32_t *out)
{
    const uint32_t lo = 0x3c03126fu, hi = 0x7f7fffffu;
    for (size_t i = 0; i < cnt; ++i) out[i] = t[i] - (lo + 1u) < hi - lo - 1u;
}

void ph_udiv(const uint32_t *n, const uint32_t *m, const uint32_t *s1, const uint32_t *s2, size_t cnt, uint32_t *out)
{
    for (size_t i = 0; i < cnt; ++i) {
        const uint32_t t = static_cast<uint32_t>((static_cast<uint64_t>(n[i]) * m[i]) >> 32);
        out[i] = (t + ((n[i] - t) >> s1[i])) >> s2[i];
    }
}

} // extern "C"
