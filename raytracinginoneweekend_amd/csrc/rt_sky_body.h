// rt_sky_body.h — the body of the sky kernels (rt_sky.hip: the loop is described there), included
// inside each kernel's braces so that both are the same statements: a device function inlined into
// sky_kernel compiles to other machine code than the body written in the kernel (the record then
// reaches it through a generic pointer, not as kernel arguments). The including kernel defines:
//   constexpr bool MOMENTS;  const KSky &p;  const KSkyMoments *q (MOMENTS: its record, else null);
//   __shared__ float2 ring[RT_SKY_RING][256].
// No include guard: it is included once per kernel.
    const FrameConsts &fc = p.fc;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;  // the sky pixel
    const bool live = t < p.n_pix;
    uint32_t px, rr;
    pixel_of(fc, p.pos0 + (live ? t : 0u), px, rr, p.block_perm);
    const uint32_t py = fc.row_offset + rr * fc.row_stride;
    const uint64_t inc_data = ((uint64_t)fc.inc_data_hi << 32) | fc.inc_data_lo;
    const uint64_t inc_cam = ((uint64_t)fc.inc_cam_hi << 32) | fc.inc_cam_lo;
    const uint64_t key0 = (uint64_t)(py * fc.W + px) * fc.spp;
    const uint32_t spp = fc.spp, full_end = spp & ~3u;
    const uint32_t s_a = MOMENTS ? q->s_a : 0u, s_b = MOMENTS ? q->s_b : spp;  // the call's samples
    float fW = fc.fW, fH = fc.fH, rW = fc.rW, rH = fc.rH, lens = fc.lens;
    const bool dw = fc.div_fast & 1u, dh = fc.div_fast & 2u;
    f3 org = mk(fc.org[0], fc.org[1], fc.org[2]), llc = mk(fc.llc[0], fc.llc[1], fc.llc[2]);
    f3 hor = mk(fc.hor[0], fc.hor[1], fc.hor[2]), ver = mk(fc.ver[0], fc.ver[1], fc.ver[2]);
    // (a VALU operation reading an SGPR issues at half rate, scripts/ubench_int.hip)
    if (RT_SKY_VCONST >= 1) asm volatile("" : "+v"(fW), "+v"(fH), "+v"(rW), "+v"(rH), "+v"(lens));
    if (RT_SKY_VCONST >= 2) {
        asm volatile("" : "+v"(org.x), "+v"(org.y), "+v"(org.z), "+v"(llc.x), "+v"(llc.y), "+v"(llc.z));
        asm volatile("" : "+v"(hor.x), "+v"(hor.y), "+v"(hor.z), "+v"(ver.x), "+v"(ver.y), "+v"(ver.z));
    }
    // acc: the running sum; pa: the block's c0, then c2; pb: c0 + c1
    f3 acc = mk(0.f, 0.f, 0.f), pa = acc, pb = acc;
    // MOMENTS: L_0 and the shifted sums, and where the pixel's sum and moments are carried: at its
    // natural index in a session's planes, at its sky position in a one-shot frame's two slot rows
    float l0 = 0.f, m1 = 0.f, m2 = 0.f;
    (void)l0; (void)m1; (void)m2;
    size_t at = 0;
    (void)at;
    if (MOMENTS) {
        const uint32_t pos = p.pos0 + (live ? t : 0u);
        at = 3u * (size_t)(!q->natural ? t : p.block_perm ? (p.block_perm[pos >> 6] << 6) | (pos & 63u) : pos);
        if (live && s_a > 0u) {
            acc = mk(q->acc[at], q->acc[at + 1], q->acc[at + 2]);
            l0 = q->mom[at], m1 = q->mom[at + 1], m2 = q->mom[at + 2];
        }
    }
    // Sample s's streams (main.cxx:192-200, key = (y W + x) spp + s): pcg_seed(key, inc) =
    // key M + inc (M + 1), and the data stream's second state M (key M + inc (M + 1)) + inc; both
    // are key M and key M^2 plus wave-uniform terms, and the key steps by 1 from sample to sample,
    // so the two products step by M and M^2 (mod 2^64, exact): no multiply per sample
    const uint64_t cd1 = inc_data * (kPcgMul + 1u), cd2 = cd1 * kPcgMul + inc_data, cc = inc_cam * (kPcgMul + 1u);
    const uint64_t mm = kPcgMul * kPcgMul;
    uint64_t km = (key0 + s_a) * kPcgMul, kmm = km * kPcgMul;
    const float ux = div_const((float)px, fW, rW, dw), vy = div_const((float)py, fH, rH, dh);
    // the draw side: sd, the sample whose lens point the lane is drawing (a dead lane has none to
    // draw, and counts as having every point waiting); rc, the camera stream's state; kc, key M
    // of the sample after sd. The LCG multiplier's halves and the 2^-31 scale sit in VGPRs, as in
    // random_in_unit_sphere_capped.
    uint32_t sd = live ? s_a : s_b;
    uint64_t rc = km + cc, kc = km + kPcgMul;
    uint32_t m_lo = (uint32_t)kPcgMul, m_hi = (uint32_t)(kPcgMul >> 32);
    float k31 = 0x1p-31f;
    asm volatile("" : "+v"(m_lo), "+v"(m_hi), "+v"(k31));
    const uint64_t mul = ((uint64_t)m_hi << 32) | m_lo;
    auto draw = [&]() {
        const uint64_t old = rc;
        rc = old * mul + inc_cam;
        return fmaf(fminf((float)pcg_out(old), 0x1.fffffep31f), k31, -1.f);  // canonical_pm1
    };
    // the colour side: sc, the wave's colour sample (uniform); a wave without a live lane leaves
    const uint32_t n_s = ballot(live) ? s_b : 0u;
    const uint32_t tid = threadIdx.x;
    for (uint32_t sc = s_a; sc < n_s;) {
        if (ballot(sd == sc)) {
            // some lane has no point waiting (sd >= sc always): an attempt round, camera.hxx:52
            const uint32_t room_end = min(s_b, sc + (uint32_t)RT_SKY_RING);
            if (sd < room_end) {
                const float x = draw();
                const float y = draw();
                const float z = draw();
                if (!(x * x + y * y + z * z > 0x1.000002p+0f)) {
                    ring[sd & (RT_SKY_RING - 1u)][tid] = make_float2(x, y);
                    ++sd;
                    rc = kc + cc;
                    kc += kPcgMul;
                }
            }
        }
        // (a second if, not an else: the draw side's registers are then updated in place, where
        // the else form copied sd, rc and kc on every attempt round, 9 moves)
        if (!ballot(sd == sc)) {
            // every lane holds sample sc's point: a colour round for the whole wave
            const float2 r = ring[sc & (RT_SKY_RING - 1u)][tid];
            const float xu = fminf((float)pcg_out(km + cd1), 0x1.fffffep31f) * 0x1p-32f;  // canonical()
            const float xv = fminf((float)pcg_out(kmm + cd2), 0x1.fffffep31f) * 0x1p-32f;
            const float uu = ux + div_const(xu, fW, rW, dw);
            const float vv = vy + div_const(xv, fH, rH, dh);
            km += kPcgMul;
            kmm += mm;
            const f3 rd = mk(r.x * lens, r.y * lens, 0.f);                      // camera.hxx:46-57
            const f3 off = mk(uu * rd.x, vv * rd.y, 0.f);
            f3 d = ((llc + hor * uu) + ver * (1.f - vv)) - off;
            if (fc.corrected) d = d - org;
            // unit_direction(d).y (math.hxx:219-227): with |d|^2 in [2^-40, 2^40] the short
            // sqrt and division give its bits (render_body's sky)
            const float a = d.x * d.x + d.y * d.y + d.z * d.z;
            float uy;
            if (!ballot(!(a >= 0x1p-40f && a <= 0x1p40f))) {
                const float l = sqrt_scaled(a);
                const float y0 = __builtin_amdgcn_rcpf(l);
                uy = div_ray(d.y, RayDiv{l, fmaf(fmaf(-l, y0, 1.f), y0, y0), 1u});
            } else {
                uy = normalize(d).y;
            }
            const float tt = .5f * uy + 1.f;                                    // main.cxx:71
            const f3 col = mk(1.f, 1.f, 1.f) * (1.f - tt) + mk(.5f, .7f, 1.f) * tt;
            // the blocked sum, on scalar branches: c0 and c2 wait in pa, c0 + c1 in pb, and the
            // block's (c0 + c1) + (c2 + c3), or a tail colour, folds into acc
            const uint32_t j = sc & 3u;
            if (sc >= full_end) {
                acc = acc + col;
            } else if (j == 1u) {
                pb = pa + col;
            } else if (j == 3u) {
                acc = acc + (pb + (pa + col));
            } else {
                pa = col;
            }
            if (MOMENTS) fold_luminance(col, sc == 0u, l0, m1, m2);
            ++sc;
        }
    }
    if (MOMENTS) {
        if (live) {
            q->acc[at] = acc.x, q->acc[at + 1] = acc.y, q->acc[at + 2] = acc.z;
            q->mom[at] = l0, q->mom[at + 1] = m1, q->mom[at + 2] = m2;
        }
    } else if (live) {
        float *o = p.sums + 3u * (size_t)t;
        o[0] = acc.x;
        o[1] = acc.y;
        o[2] = acc.z;
    }
    if (p.segments) {
        const uint32_t n = lanes(live);
        if ((threadIdx.x & 63u) == 0u && n) atomicAdd(p.segments, (unsigned long long)n * (s_b - s_a));
    }
