// rt_ground.hip — the ground kernel and its launcher, a translation unit of its
// own over rt_trace.h's vector math, RNG, pixel enumeration and sphere tests.
#include "rt_trace.h"

namespace rt {

// ---- the ground kernel ---------------------------------------------------
// The pixels of the ground tiles: tiled blocks whose beam of primary rays misses every cluster's
// padded box (rt_tiles.h classify_tile, class 1), so the primary's closest hit is the always-tested
// list's alone. One thread per pixel, the pass's samples in order; per sample the operations of
// render_body for the only two paths these tiles take almost always:
//   primary misses the list                                   -> the sky's colour (as sky_kernel)
//   primary hits a (lambert) sphere of the list, the scattered ray misses the list and fails
//   closest_hit's root gate (it meets no cluster)             -> the sky's colour times the albedo
// Every other sample (the scattered ray hits the list again, or passes the gate) is punted: the
// lane writes no slot and appends the sample's item word (its slot index) to the pass's redo
// list, which render_list_kernel renders from scratch. A thread takes KGround::spt consecutive
// samples of its pixel (a pass's samples are cut into such parts, one wave per part and 64 pixels:
// a thread with all 128 samples of a lone pass is a chain that outlasts a row share's whole frame).
// Same draws per stream in the same order,
// same operations per sample, same bits; the host takes the kernel only when every sphere of the
// list is lambert and max_depth >= 2.
// As in sky_kernel the draws run ahead of the colours through per-lane rings in LDS, here for two
// streams: the camera stream's lens points, and the data stream's scatter points (the stream's
// state after the sample's two jitter draws is key M^3 plus a wave-uniform term, so it is known per
// sample by addition; a point drawn for a sample whose primary then misses is dropped). A colour
// round runs when every lane holds both points of the wave's sample sc. Slots are cursor &
// (RT_GROUND_RING - 1): every index is in the arrays whatever the cursors hold (§4.6).
#ifndef RT_GROUND_RING
#define RT_GROUND_RING 8
#endif
static_assert(RT_GROUND_RING >= 2 && (RT_GROUND_RING & (RT_GROUND_RING - 1)) == 0, "ring depth: a power of two");
constexpr uint32_t kGroundAlways = 8;  // the always-tested list the kernel stages (the host checks)

// main.cxx:71 as render_body forms it: background(.5 unit_direction(d).y + 1), a = |d|^2
__device__ __forceinline__ f3 sky_colour(f3 d, float a, uint32_t fd)
{
    float uy;
    if (fd != 0u) {
        const float l = sqrt_scaled(a);
        const float y0 = __builtin_amdgcn_rcpf(l);
        uy = div_ray(d.y, RayDiv{l, fmaf(fmaf(-l, y0, 1.f), y0, y0), 1u});
    } else {
        uy = normalize(d).y;
    }
    const float tt = .5f * uy + 1.f;
    return mk(1.f, 1.f, 1.f) * (1.f - tt) + mk(.5f, .7f, 1.f) * tt;
}

template <bool FAST, bool STATS, bool COUNT>
__global__ __launch_bounds__(64) void ground_kernel(const KGround p)
{
    constexpr uint32_t R = RT_GROUND_RING;
    __shared__ float2 ring_c[R][64];
    __shared__ float ring_d[3][R][64];
    // the always-tested list: geo entries {C, fl(r r)}, original indices, shading records
    __shared__ float4 s_geo[kGroundAlways], s_sf[kGroundAlways], s_md[kGroundAlways], s_root[2];
    __shared__ uint32_t s_sidx[kGroundAlways];
    const uint32_t lane = threadIdx.x;
    const uint32_t n_always = min(p.n_always, kGroundAlways);
    if (lane < kGroundAlways) {
        float4 g = make_float4(0.f, 0.f, 0.f, -__builtin_inff()), sf = g, md = g;  // padding never hits
        uint32_t id = 0xffffffffu;
        if (lane < n_always) {
            g = p.blob[lane];
            id = reinterpret_cast<const uint32_t *>(p.blob + p.n_geo)[lane];
            const uint32_t ib = checked<STATS>(id, p.n_spheres, BC_SHADE, p.dbg);
            sf = p.blob[p.shade_offset + 2u * ib];
            md = p.blob[p.shade_offset + 2u * ib + 1u];
        }
        s_geo[lane] = g;
        s_sidx[lane] = id;
        s_sf[lane] = sf;
        s_md[lane] = md;
    } else if (lane < kGroundAlways + 2u) {
        // the box over all clusters follows the n_supers level-2 boxes (closest_hit's root gate)
        s_root[lane - kGroundAlways] = p.blob[p.supers_offset + 2u * p.n_supers + (lane - kGroundAlways)];
    }
    __syncthreads();

    const FrameConsts &fc = p.fc;
    const uint32_t part = blockIdx.x / p.n_wg;
    const uint32_t t = (blockIdx.x - part * p.n_wg) * 64u + lane;  // the ground pixel
    const uint32_t s_lo = part * p.spt;                            // its first sample of the pass here
    const bool live = t < p.n_pix;
    const uint32_t pos = p.pos0 + (live ? t : 0u);
    uint32_t px, rr;
    pixel_of(fc, pos, px, rr, p.block_perm);
    const uint32_t py = fc.row_offset + rr * fc.row_stride;
    const uint64_t inc_data = ((uint64_t)fc.inc_data_hi << 32) | fc.inc_data_lo;
    const uint64_t inc_cam = ((uint64_t)fc.inc_cam_hi << 32) | fc.inc_cam_lo;
    const uint64_t key0 = (uint64_t)(py * fc.W + px) * fc.spp + fc.sample_begin + s_lo;
    const uint32_t n_samp = min(p.spt, p.n_samp - min(s_lo, p.n_samp));  // this thread's samples
    const float fW = fc.fW, fH = fc.fH, rW = fc.rW, rH = fc.rH, lens = fc.lens;
    const bool dw = fc.div_fast & 1u, dh = fc.div_fast & 2u;
    const f3 org = mk(fc.org[0], fc.org[1], fc.org[2]), llc = mk(fc.llc[0], fc.llc[1], fc.llc[2]);
    const f3 hor = mk(fc.hor[0], fc.hor[1], fc.hor[2]), ver = mk(fc.ver[0], fc.ver[1], fc.ver[2]);
    // Sample s's streams (sky_kernel): the camera stream starts at key M + cc; the data stream gives
    // the two jitters from key M + cd1 and key M^2 + cd2 and stands at key M^3 + cd3 after them. The
    // key steps by 1 from sample to sample, so the three products step by M, M^2 and M^3.
    const uint64_t cd1 = inc_data * (kPcgMul + 1u), cd2 = cd1 * kPcgMul + inc_data, cd3 = cd2 * kPcgMul + inc_data;
    const uint64_t cc = inc_cam * (kPcgMul + 1u);
    const uint64_t m2 = kPcgMul * kPcgMul, m3 = m2 * kPcgMul;
    uint64_t km = key0 * kPcgMul, kmm = km * kPcgMul;
    const float ux = div_const((float)px, fW, rW, dw), vy = div_const((float)py, fH, rH, dh);
    // the draw sides: sdc / sdd, the sample whose lens / scatter point the lane is drawing (a dead
    // lane has none to draw); rc / rs, the streams' states; kc / ks, key M and key M^3 of the
    // sample after it
    uint32_t sdc = live ? 0u : n_samp, sdd = sdc;
    uint64_t rc = km + cc, kc = km + kPcgMul;
    uint64_t ks = kmm * kPcgMul, rs = ks + cd3;
    ks += m3;
    uint32_t m_lo = (uint32_t)kPcgMul, m_hi = (uint32_t)(kPcgMul >> 32);
    float k31 = 0x1p-31f;
    asm volatile("" : "+v"(m_lo), "+v"(m_hi), "+v"(k31));
    const uint64_t mul = ((uint64_t)m_hi << 32) | m_lo;
    auto draw = [&](uint64_t &st, uint64_t inc) {
        const uint64_t old = st;
        st = old * mul + inc;
        return fmaf(fminf((float)pcg_out(old), 0x1.fffffep31f), k31, -1.f);  // canonical_pm1
    };
    Dbg dbg{};
    auto always_list = [&](f3 o, f3 d, const RayDiv &rd, Hit &h) {  // closest_hit's first step
        if (RT_GROUND1 && n_always == 1u) test_block8<FAST, false, 1>(s_geo, s_sidx, 0, o, d, rd, h, dbg);
        else run_members<FAST, false>(s_geo, s_sidx, 0, n_always, o, d, rd, h, dbg);
    };
    uint32_t n_seg = 0, n_box = 0;  // COUNT: the non-punted samples' segments and box tests (wave-uniform)
    const uint32_t n_s = ballot(live) ? n_samp : 0u;
    for (uint32_t sc = 0; sc < n_s;) {
        if (ballot(sdc == sc) | ballot(sdd == sc)) {
            // some lane lacks a point of sample sc (sdc, sdd >= sc always): an attempt round,
            // one attempt of raytracer.hxx:32-43 per stream for the lanes with room in that ring
            const uint32_t room_end = min(n_samp, sc + R);
            if (sdc < room_end) {
                const float x = draw(rc, inc_cam);
                const float y = draw(rc, inc_cam);
                const float z = draw(rc, inc_cam);
                if (!(x * x + y * y + z * z > 0x1.000002p+0f)) {
                    ring_c[sdc & (R - 1u)][lane] = make_float2(x, y);
                    ++sdc;
                    rc = kc + cc;
                    kc += kPcgMul;
                }
            }
            if (sdd < room_end) {
                const float x = draw(rs, inc_data);
                const float y = draw(rs, inc_data);
                const float z = draw(rs, inc_data);
                if (!(x * x + y * y + z * z > 0x1.000002p+0f)) {
                    const uint32_t w = sdd & (R - 1u);
                    ring_d[0][w][lane] = x;
                    ring_d[1][w][lane] = y;
                    ring_d[2][w][lane] = z;
                    ++sdd;
                    rs = ks + cd3;
                    ks += m3;
                }
            }
        }
        if (!(ballot(sdc == sc) | ballot(sdd == sc))) {
            // every lane holds sample sc's two points: a colour round for the whole wave
            const uint32_t w = sc & (R - 1u);
            const float2 r = ring_c[w][lane];
            const float xu = fminf((float)pcg_out(km + cd1), 0x1.fffffep31f) * 0x1p-32f;  // canonical()
            const float xv = fminf((float)pcg_out(kmm + cd2), 0x1.fffffep31f) * 0x1p-32f;
            const float uu = ux + div_const(xu, fW, rW, dw);
            const float vv = vy + div_const(xv, fH, rH, dh);
            km += kPcgMul;
            kmm += m2;
            const f3 rl = mk(r.x * lens, r.y * lens, 0.f);                          // camera.hxx:46-57
            const f3 off = mk(uu * rl.x, vv * rl.y, 0.f);
            const f3 o = org + off;
            f3 d = ((llc + hor * uu) + ver * (1.f - vv)) - off;
            if (fc.corrected) d = d - org;
            // the primary's closest hit: the always-tested list alone (the tile's proof)
            const float a = d.x * d.x + d.y * d.y + d.z * d.z;
            const RayDiv rd = ray_div(a, ballot(true), p.fast_roots);
            Hit h{no_hit()};
            always_list(o, d, rd, h);
            const bool hit = h.id() != 0xffffffffu;
            const uint64_t hm = ballot(hit);  // the lanes of the second segment
            f3 col;
            bool punt = false;
            if (!hit) {
                col = sky_colour(d, a, rd.fd);  // main.cxx:71, attenuation 1
            } else {
                // the lambert branch of render_body (raytracer.hxx:132-141), then the second segment
                uint32_t k = 0;
                for (uint32_t j = 1; j < n_always; ++j) k = s_sidx[j] == h.id() ? j : k;
                const float4 sf = s_sf[k], md = s_md[k];
                const f3 hp = o + d * h.t();                                        // math.hxx:353
                const f3 dv = hp - mk(sf.x, sf.y, sf.z);                            // raytracer.hxx:71
                f3 hn;
                if (p.fast_roots && all_lanes_min_abs_ok(dv)) hn = div3_short(dv, sf.w);
                else hn = dv / sf.w;
                const f3 att = mk(1.f, 1.f, 1.f) * mk(md.x, md.y, md.z);            // main.cxx:65
                const f3 q = mk(ring_d[0][w][lane], ring_d[1][w][lane], ring_d[2][w][lane]);
                const f3 d2 = ((hp + hn) + q) - hp;                                 // :135
                const float a2 = d2.x * d2.x + d2.y * d2.y + d2.z * d2.z;
                const RayDiv rd2 = ray_div(a2, hm, p.fast_roots);
                Hit h2{no_hit()};
                always_list(hp, d2, rd2, h2);
                // closest_hit's root gate: a ray that fails it meets no cluster's padded box
                auto safe_rcp = [](float x) { return __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(x), -1e30f, 1e30f); };
                const float ix = safe_rcp(d2.x), iy = safe_rcp(d2.y), iz = safe_rcp(d2.z);
                const float aix = fabsf(ix), aiy = fabsf(iy), aiz = fabsf(iz);
                const float pad = fmaf(RT_PAD_REL, fabsf(hp.x) + fabsf(hp.y) + fabsf(hp.z), p.clus_pad);
                const RayBox rb{ix, iy, iz, hp.x * ix, hp.y * iy, hp.z * iz, aix, aiy, aiz, pad * aix, pad * aiy, pad * aiz};
                const bool gate = box_pass(rb, s_root[0], s_root[1], 0.5f * RT_TMIN, h2.t() * 1.002f);
                punt = h2.id() != 0xffffffffu || gate;
                col = sky_colour(d2, a2, rd2.fd) * att;
            }
            const uint32_t slot = (s_lo + sc) * fc.n_pixels + pos;  // [sample][position]
            if (live && !punt) {
                float *dst = p.slots + (size_t)checked<STATS>(slot, p.n_slots, BC_SLOT, p.dbg) * 3u;
                dst[0] = col.x;
                dst[1] = col.y;
                dst[2] = col.z;
            }
            const uint64_t pm = ballot(live && punt);
            if (pm) {
                // one atomic per wave; the list holds every ground sample of the pass, and an
                // index past it (never: the host sizes it) is dropped, and recorded under STATS
                uint32_t base = 0;
                if (lane == (uint32_t)__builtin_ctzll(pm)) base = atomicAdd(p.redo.ctr + kRedoCount, (uint32_t)__popcll(pm));
                base = (uint32_t)__builtin_amdgcn_readlane((int)base, (int)__builtin_ctzll(pm));
                const uint32_t at = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(pm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pm, 0u));
                if (live && punt) {
                    if (at < p.redo.cap) p.redo.items[at] = slot;
                    else (void)checked<STATS>(at, p.redo.cap, BC_REDO_APPEND, p.dbg);
                }
            }
            if (COUNT) {
                const uint32_t n1 = lanes(live && !hit), n2 = lanes(live && hit && !punt);
                n_seg += n1 + 2u * n2;
                n_box += n2;
            }
            ++sc;
        }
    }
    if (COUNT && p.segments && lane == 0 && n_seg) {
        atomicAdd(p.segments + 0, (unsigned long long)n_seg);
        atomicAdd(p.segments + 1, (unsigned long long)n_seg * n_always);
        atomicAdd(p.segments + 2, (unsigned long long)n_box);
    }
}

hipError_t launch_ground(int variant, const KGround &k, hipStream_t stream)
{
    if (!k.n_pix || !k.n_samp || !k.spt || !k.n_wg) return hipSuccess;
    const bool count = k.segments != nullptr;
    const void *fn = nullptr;
    switch (variant) {
    case V_EXACT_LDS:
        fn = count ? reinterpret_cast<const void *>(&ground_kernel<false, false, true>)
                   : reinterpret_cast<const void *>(&ground_kernel<false, false, false>);
        break;
    case V_FAST_LDS:
        fn = count ? reinterpret_cast<const void *>(&ground_kernel<true, false, true>)
                   : reinterpret_cast<const void *>(&ground_kernel<true, false, false>);
        break;
    case V_STATS_LDS: fn = reinterpret_cast<const void *>(&ground_kernel<false, true, true>); break;
    default: return hipErrorInvalidValue;
    }
    void *args[] = {const_cast<KGround *>(&k)};
    return hipLaunchKernel(fn, dim3(k.n_wg * ((k.n_samp + k.spt - 1u) / k.spt)), dim3(64), args, 0, stream);
}

} // namespace rt
