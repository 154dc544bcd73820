// TEST INFRASTRUCTURE: the per-sample colours of a pass, for the reference of rt_render_var's
// variance plane. Builds on the CPU restatement (oracle/rt_oracle.cpp, included):
// every sample is started exactly as oracle_render_f32 starts it in rng_mode 0 (the GPU contract)
// and traced with color(); the pixel's colour is formed with reduce_samples and divs. The variance
// itself is formed in numpy (tests/tools/moments_ref.py), line by line from the contract.
#include "../../oracle/rt_oracle.cpp"

// samples: [rendered row][x][s][3], packed rows in render order. rgb (optional): laid out as
// rt_params says (packed rows or RT_FLAG_FULL_FRAME); rows not rendered are left alone.
extern "C" int moments_ref(const rt_sphere *spheres, uint32_t n, const rt_material *mats, uint32_t nm,
                           const rt_camera *camera, const rt_params *params, float *samples, float *rgb)
{
    if (!spheres || !mats || !camera || !params || !samples || params->spp == 0) return RT_ERR_INVALID;
    const rt_params p = *params;
    const scene sc{spheres, n, mats, nm};
    const cam c = to_cam(camera);
    const std::uint32_t nrows = rows_of(p), stride = p.row_stride ? p.row_stride : 1;
    const bool full = p.flags & RT_FLAG_FULL_FRAME;
    std::vector<v3> cs(p.spp);
    pcg32 gd, gc;
    std::uint64_t seg = 0;
    for (std::uint32_t i = 0; i < nrows; ++i) {
        const std::uint32_t y = p.row_offset + i * stride;
        const float v = static_cast<float>(y) / static_cast<float>(p.height);      // main.cxx:192
        for (std::uint32_t x = 0; x < p.width; ++x) {
            const float u = static_cast<float>(x) / static_cast<float>(p.width);     // main.cxx:195
            float *o = samples + (static_cast<std::size_t>(i) * p.width + x) * p.spp * 3u;
            for (std::uint32_t s = 0; s < p.spp; ++s) {
                const std::uint64_t key = (static_cast<std::uint64_t>(y) * p.width + x) * p.spp + s;
                gd.seed(key, 2u * p.seed);
                gc.seed(key, 2u * p.seed + 1u);
                const float uu = u + canonical(gd) / static_cast<float>(p.width);
                const float vv = v + canonical(gd) / static_cast<float>(p.height);
                cs[s] = color(sc, gd, camera_ray(c, gc, uu, vv), p.max_depth, seg);
                o[3 * s] = cs[s].x; o[3 * s + 1] = cs[s].y; o[3 * s + 2] = cs[s].z;
            }
            if (rgb) {
                const v3 col = divs(reduce_samples(cs), static_cast<float>(p.spp));  // main.cxx:205-207
                float *d = rgb + (static_cast<std::size_t>(full ? y : i) * p.width + x) * 3u;
                d[0] = col.x; d[1] = col.y; d[2] = col.z;
            }
        }
    }
    return RT_OK;
}
