// rt_tiles.h — the beam arithmetic of the tile classes, stated once for
// the host (rt_host_build.cpp classify_tiles, built with -x c++ and by tests/sanitize) and for the
// device (rt_tiles.hip classify_tiles_kernel). Both sides are built with -ffp-contract=off
// -fno-fast-math and evaluate the same expression tree of binary64 +, -, *, / and comparisons
// (the device's division is the IEEE sequence), so a tile's class is the same on both, exactly.
// Minimum, maximum and magnitude are explicit comparisons in the operand order std::min, std::max
// and std::fabs had here before: lo(a, b) = b < a ? b : a, hi(a, b) = a < b ? b : a. The magnitude
// x < 0 ? -x : x differs from fabs only in the sign of a zero (and of a NaN), which no comparison
// sees and which never reaches a divisor: those are tested > 0 or < 0 first.
#pragma once
#include <cstdint>

#include "../../include/rt_api.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define RT_TILE_FN __host__ __device__ inline
#else
#define RT_TILE_FN inline
#endif

namespace rttile {

// What the classifier reads of a culled scene (rthost::scene_geom, or its copy on the device):
// the box over all clusters (null: none), the always-tested spheres, the non-empty clusters'
// boxes {C[3], E[3]} and the kernel's pad.
struct geom_view {
    const float *root;
    const rt_sphere *always;
    uint32_t n_always;
    const float *boxes;
    uint32_t n_boxes;
    float clus_pad;
};

// The tiled part of a pass: tiles of tw x th pixels, tiles_x per tile row, rows y = row_offset +
// i st of a W x H image.
struct pass_view {
    uint32_t W, H, row_offset, st, tw, th, tiles_x;
};

// closed intervals in double: every operation's result contains every value its operands can take
struct iv {
    double lo, hi;
};
RT_TILE_FN double lo2(double a, double b) { return b < a ? b : a; }
RT_TILE_FN double hi2(double a, double b) { return a < b ? b : a; }
RT_TILE_FN double absd(double x) { return x < 0 ? -x : x; }
RT_TILE_FN iv operator+(iv a, iv b) { return {a.lo + b.lo, a.hi + b.hi}; }
RT_TILE_FN iv operator-(iv a, iv b) { return {a.lo - b.hi, a.hi - b.lo}; }
RT_TILE_FN iv operator-(iv a, double c) { return {a.lo - c, a.hi - c}; }
RT_TILE_FN iv operator*(iv a, iv b)
{
    const double p0 = a.lo * b.lo, p1 = a.lo * b.hi, p2 = a.hi * b.lo, p3 = a.hi * b.hi;
    return {lo2(lo2(p0, p1), lo2(p2, p3)), hi2(hi2(p0, p1), hi2(p2, p3))};
}
RT_TILE_FN iv operator*(double c, iv a) { return c >= 0 ? iv{c * a.lo, c * a.hi} : iv{c * a.hi, c * a.lo}; }
RT_TILE_FN iv sq(iv a)
{
    if (a.lo >= 0) return {a.lo * a.lo, a.hi * a.hi};
    if (a.hi <= 0) return {a.hi * a.hi, a.lo * a.lo};
    return {0.0, hi2(a.lo * a.lo, a.hi * a.hi)};
}
RT_TILE_FN iv grow(iv a, double e) { return {a.lo - e, a.hi + e}; }
RT_TILE_FN double mag(iv a) { return hi2(absd(a.lo), absd(a.hi)); }

// Every ray o + t d (t >= 0) with o in the box o[], d in the box d[] misses the box [lo, hi]:
// the t for which a coordinate of some ray of the beam can lie in the slab form one interval
// per axis (o_lo + t d_lo <= hi and o_hi + t d_hi >= lo), which contains each single ray's
// slab interval; if the three have no common t >= 0, no ray of the beam meets the box.
RT_TILE_FN bool beam_misses(const iv o[3], const iv d[3], const double lo[3], const double hi[3])
{
    double t0 = 0.0, t1 = __builtin_huge_val();
    for (int k = 0; k < 3; ++k) {
        const double a = hi[k] - o[k].lo;  // t d_lo <= a
        if (d[k].lo > 0) t1 = lo2(t1, a / d[k].lo);
        else if (d[k].lo < 0) t0 = hi2(t0, a / d[k].lo);
        else if (a < 0) return true;
        const double b = lo[k] - o[k].hi;  // t d_hi >= b
        if (d[k].hi > 0) t0 = hi2(t0, b / d[k].hi);
        else if (d[k].hi < 0) t1 = lo2(t1, b / d[k].hi);
        else if (b > 0) return true;
    }
    // empty with a relative margin far above the double divisions' rounding
    return t1 < 0 || t0 > t1 * (1 + 1e-9) + 1e-12;
}

// No ray of the beam gets a candidate from sphere S in the kernel's binary32 test
// (raytracer.hxx:52-92 as rt_trace.h test_block8 evaluates it), proven in exact arithmetic
// with margins of 1e-5 of the terms' magnitudes, where the binary32 evaluation errs by < 2^-21:
// either the discriminant b^2 - a c is negative for every ray, or every ray starts outside S
// (c > 0) moving away from it (b > 0) with b 2^-22 < kMIN a / 2, so that both roots are negative
// and the rounded far root stays below kMIN (the kernel's own shortcut for the ground, whose
// condition the float values then meet too).
RT_TILE_FN bool sphere_missed(const iv o[3], const iv d[3], const rt_sphere &S)
{
    const iv oc[3] = {o[0] - static_cast<double>(S.center[0]), o[1] - static_cast<double>(S.center[1]),
                      o[2] - static_cast<double>(S.center[2])};
    const double r2 = static_cast<double>(S.radius) * S.radius;
    const iv a = sq(d[0]) + sq(d[1]) + sq(d[2]);
    const iv b = oc[0] * d[0] + oc[1] * d[1] + oc[2] * d[2];
    const iv c = (sq(oc[0]) + sq(oc[1]) + sq(oc[2])) - r2;
    const double bm = mag(oc[0]) * mag(d[0]) + mag(oc[1]) * mag(d[1]) + mag(oc[2]) * mag(d[2]);
    const double cm = mag(oc[0]) * mag(oc[0]) + mag(oc[1]) * mag(oc[1]) + mag(oc[2]) * mag(oc[2]) + r2;
    const iv disc = sq(b) - a * c;
    if (disc.hi < -1e-5 * (bm * bm + a.hi * cm)) return true;
    return b.lo > 1e-5 * bm && c.lo > 1e-5 * cm && b.hi * 0x1p-22 < 0.5 * 0.008 * a.lo;
}

// The beam of a tile (every primary ray of its pixels: origins o[], directions d[]) misses the
// box r = {C[3], E[3]} grown by pad.
RT_TILE_FN bool box_missed(const iv o[3], const iv d[3], double pad, const float *r)
{
    double lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = static_cast<double>(r[k]) - r[3 + k] - pad;
        hi[k] = static_cast<double>(r[k]) + r[3 + k] + pad;
    }
    return beam_misses(o, d, lo, hi);
}

// The class of tile t of the pass: 0 lead (a primary ray can meet a cluster's padded box), 1 other,
// 2 sky (every primary ray proven to meet no sphere). sky_only: 1 for every tile that is not sky.
RT_TILE_FN uint8_t classify_tile(const rt_camera &cam, const pass_view &p, const geom_view &g, uint32_t t, bool sky_only)
{
    const uint32_t W = p.W, H = p.H, row_offset = p.row_offset, st = p.st, tw = p.tw, th = p.th, tiles_x = p.tiles_x;
    const double lens = absd(static_cast<double>(cam.lens_radius));
    const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
    const double x0 = static_cast<double>(tx) * tw, x1 = x0 + tw;  // x in [x0, x1), jitter < 1
    const double y0 = row_offset + static_cast<double>(ty) * th * st, y1 = y0 + static_cast<double>(th - 1) * st + 1;
    // uu = x/W + U/W, vv = y/H + U/H in binary32 (a few ulps around the exact values)
    const iv uu = grow({x0 / W, x1 / W}, 1e-6 * (x1 / W) + 1e-12);
    const iv vv = grow({y0 / H, y1 / H}, 1e-6 * (y1 / H) + 1e-12);
    const iv omv = iv{1.0, 1.0} - vv;
    // lens offset {uu rd.x, vv rd.y, 0}, |rd_k| <= lens (camera.hxx:52-54)
    const double ox = lens * mag(uu), oy = lens * mag(vv);
    const iv off[3] = {{-ox, ox}, {-oy, oy}, {0.0, 0.0}};
    iv o[3], d[3];
    for (int k = 0; k < 3; ++k) {
        const double org = cam.origin[k], llc = cam.lower_left_corner[k], hor = cam.horizontal[k], ver = cam.vertical[k];
        o[k] = grow(iv{org, org} + off[k], 1e-6 * (absd(org) + mag(off[k])) + 1e-30);
        // camera.hxx:56: llc + hor u + ver (1 - v) - offset (- origin in the corrected mode)
        iv dk = ((iv{llc, llc} + hor * uu) + ver * omv) - off[k];
        double m = absd(llc) + absd(hor) * mag(uu) + absd(ver) * mag(omv) + mag(off[k]);
        if (cam.mode == RT_CAMERA_CORRECTED) {
            dk = dk - org;
            m += absd(org);
        }
        d[k] = grow(dk, 1e-5 * m + 1e-30);
    }
    const double o1 = mag(o[0]) + mag(o[1]) + mag(o[2]);
    // twice the kernel's per-ray pad (rt_trace.h closest_hit: 1e-3 |o|_1 + clus_pad)
    const double pad = 2.0 * (1e-3 * o1 + g.clus_pad) + 1e-6;
    bool sky = !g.root || box_missed(o, d, pad, g.root);
    for (uint32_t i = 0; sky && i < g.n_always; ++i) sky = sphere_missed(o, d, g.always[i]);
    if (sky) return 2;
    if (sky_only) return 1;
    for (uint32_t c = 0; c < g.n_boxes; ++c)
        if (!box_missed(o, d, pad, g.boxes + 6u * c)) return 0;
    return 1;
}

// classify_tiles_kernel's record (rt_tiles.hip): the camera, the pass, the scene's geometry on the
// device as rt_scene_create laid it out ([root box: 6 floats][boxes: 6 floats each][always-tested
// spheres: rt_sphere records]) and the class byte of each of the pass's n_blocks 64-pixel blocks:
// blocks [0, n_tiles) are the 8x8 tiles, the others (rows left over) get class 1.
struct KTiles {
    rt_camera cam;
    pass_view pass;
    uint32_t n_tiles, n_blocks;
    const float *geom;
    uint32_t has_root, n_boxes, n_always;
    float clus_pad;
    uint8_t *cls;
};

} // namespace rttile
