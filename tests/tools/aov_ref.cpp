// TEST INFRASTRUCTURE: the per-sample reference of the first-hit feature buffers
// (rt_render_aov_device). Builds on the CPU restatement (oracle/rt_oracle.cpp,
// included): every sample is started like oracle_render_f32's (rng_mode 0, the GPU contract)
// with camera_ray, its first hit found with intersect over every sphere (hit_world's rule, kept
// with the sphere's index), the miss colour formed with background as color() does, and the
// planes reduced with reduce_samples and divs. Used by tests/test_aov_cpu.py and test_aov_gpu.py.
#include "../../oracle/rt_oracle.cpp"

namespace {
// hit_world (raytracer.hxx:94-118) that also says which sphere: the first with the smallest time
inline hit hit_world_index(const scene &sc, const ray &r, std::uint32_t &index)
{
    hit best{}; best.ok = false;
    index = 0xffffffffu;
    for (std::uint32_t i = 0; i < sc.n; ++i) {
        hit h;
        if (intersect(r, sc.s[i], .008f, FLT_MAX, h) && (!best.ok || h.t < best.t)) {
            best = h;
            index = i;
        }
    }
    return best;
}
} // namespace

// Planes laid out as rt_params says (packed rows or RT_FLAG_FULL_FRAME), each optional; rows not
// rendered are left alone. sample_ids (optional): [rendered row][x][sample] first-hit sphere per
// sample, 0xffffffff on a miss. samples = 0: params->spp.
extern "C" int aov_ref(const rt_sphere *spheres, uint32_t n, const rt_material *mats, uint32_t nm,
                       const rt_camera *camera, const rt_params *params, uint32_t samples, float *albedo, float *normal,
                       float *depth, float *alpha, uint32_t *sphere_id, uint32_t *sample_ids)
{
    if (!spheres || !mats || !camera || !params || params->spp == 0 || samples > params->spp) return RT_ERR_INVALID;
    const rt_params p = *params;
    if (!samples) samples = p.spp;
    const scene sc{spheres, n, mats, nm};
    const cam c = to_cam(camera);
    const std::uint32_t nrows = rows_of(p), stride = p.row_stride ? p.row_stride : 1;
    const bool full = p.flags & RT_FLAG_FULL_FRAME;
    std::vector<v3> al(samples), nr(samples), da(samples);  // da: {depth, alpha, 0}
    pcg32 gd, gc;
    for (std::uint32_t i = 0; i < nrows; ++i) {
        const std::uint32_t y = p.row_offset + i * stride;
        const float v = static_cast<float>(y) / static_cast<float>(p.height);      // main.cxx:192
        for (std::uint32_t x = 0; x < p.width; ++x) {
            const float u = static_cast<float>(x) / static_cast<float>(p.width);     // main.cxx:195
            std::uint32_t id0 = 0xffffffffu;
            for (std::uint32_t s = 0; s < samples; ++s) {
                // the beauty's sample s: key over the frame's spp (oracle_render_f32, rng_mode 0)
                const std::uint64_t key = (static_cast<std::uint64_t>(y) * p.width + x) * p.spp + s;
                gd.seed(key, 2u * p.seed);
                gc.seed(key, 2u * p.seed + 1u);
                const float uu = u + canonical(gd) / static_cast<float>(p.width);
                const float vv = v + canonical(gd) / static_cast<float>(p.height);
                const ray r = camera_ray(c, gc, uu, vv);
                std::uint32_t id;
                const hit h = hit_world_index(sc, r, id);
                if (h.ok) {
                    const rt_material &m = sc.m[h.mat];
                    al[s] = mk(m.albedo[0], m.albedo[1], m.albedo[2]);
                    nr[s] = h.n;
                    da[s] = mk(h.t, 1.f, 0.f);
                } else {
                    // color()'s miss with the attenuation still 1 (main.cxx:71)
                    al[s] = mulv(background(.5f * normalize(r.d).y + 1.f), mk(1.f, 1.f, 1.f));
                    nr[s] = mk(0.f, 0.f, 0.f);
                    da[s] = mk(0.f, 0.f, 0.f);
                }
                if (s == 0) id0 = id;
                if (sample_ids) sample_ids[(static_cast<std::size_t>(i) * p.width + x) * samples + s] = id;
            }
            const float fs = static_cast<float>(samples);
            const v3 a = divs(reduce_samples(al), fs), nn = divs(reduce_samples(nr), fs), dd = divs(reduce_samples(da), fs);
            const std::size_t at = static_cast<std::size_t>(full ? y : i) * p.width + x;
            if (albedo) { albedo[3 * at] = a.x; albedo[3 * at + 1] = a.y; albedo[3 * at + 2] = a.z; }
            if (normal) { normal[3 * at] = nn.x; normal[3 * at + 1] = nn.y; normal[3 * at + 2] = nn.z; }
            if (depth) depth[at] = dd.x;
            if (alpha) alpha[at] = dd.y;
            if (sphere_id) sphere_id[at] = id0;
        }
    }
    return RT_OK;
}
