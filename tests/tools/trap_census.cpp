// TEST INFRASTRUCTURE: the proof check of the trap windows.
// Builds on the CPU restatement (oracle/rt_oracle.cpp, included) and on the library's own host
// routine rthost::trap_windows (raytracinginoneweekend_amd/csrc/rt_host_build.cpp, linked as
// tests/sanitize/host_check.cpp links it). Every path is traced in full with brute-force
// hit_world; wherever the kernels' trigger would fire (a dielectric hit from inside, on the
// total-reflection branch, cosine in the sphere's window, before the last segment) the rest of the
// trace must stay on that sphere, inside, on that branch, use up max_depth and return exactly 0.
//   trap_census frame W H spp corrected threads     the huge scene (seed 1234), every sample
//   trap_census adversarial                         states built on the window ends, single balls
// Prints key=value lines (tests/test_trap_cpu.py reads them); exit status 1 on a violation.
#include "../../oracle/rt_oracle.cpp"
#include "../../raytracinginoneweekend_amd/csrc/rt_host_build.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace {

struct tally {
    std::uint64_t paths = 0, segments = 0, maxdepth_paths = 0, fired = 0, fired_maxdepth = 0, violations = 0,
                  saved = 0, tir_runs = 0, tir_run_ends = 0;
    double drift = 0.0, drift_scaled = 0.0;  // largest max - min of the cosine over one run; / the margin's scale
    void operator+=(const tally &o)
    {
        paths += o.paths; segments += o.segments; maxdepth_paths += o.maxdepth_paths; fired += o.fired;
        fired_maxdepth += o.fired_maxdepth; violations += o.violations; saved += o.saved; tir_runs += o.tir_runs;
        tir_run_ends += o.tir_run_ends;
        drift = std::max(drift, o.drift);
        drift_scaled = std::max(drift_scaled, o.drift_scaled);
    }
};

// hit_world (raytracer.hxx:94-118) that also names the sphere
inline hit hit_world_index(const scene &sc, const ray &r, std::uint32_t &index)
{
    hit best{}; best.ok = false;
    for (std::uint32_t i = 0; i < sc.n; ++i) {
        hit h;
        if (intersect(r, sc.s[i], .008f, FLT_MAX, h) && (!best.ok || h.t < best.t)) { best = h; index = i; }
    }
    return best;
}

// the scale of a sphere's drift margin (rt_host_build.cpp trap_windows) without the factor K
inline double margin_scale(const rt_sphere &s)
{
    const double c = std::max(std::fabs(s.center[0]), std::max(std::fabs(s.center[1]), std::fabs(s.center[2])));
    return rt::kTrapDepth * 0x1p-23 * (c + std::fabs(s.radius)) / static_cast<double>(0.008f);
}

// app::color (main.cxx:52-75) with the trigger's claim checked along the way
template <class G> v3 color_checked(const scene &sc, const std::vector<float> &win, G &g, ray r, std::uint32_t depth, tally &t)
{
    v3 atten = mk(1.f, 1.f, 1.f), result = mk(0.f, 0.f, 0.f);
    std::uint32_t seg = 0, fired_at = 0, fired_sphere = 0;
    std::uint32_t run_sphere = ~0u, run_len = 0;  // the unbroken run of same-sphere inside hits on the TIR branch
    float run_min = 0.f, run_max = 0.f;
    bool broke = false, used_up = true;
    auto end_run = [&] {
        if (run_len >= 2) {
            ++t.tir_runs;
            const double d = static_cast<double>(run_max) - run_min;
            t.drift = std::max(t.drift, d);
            t.drift_scaled = std::max(t.drift_scaled, d / margin_scale(sc.s[run_sphere]));
        }
        run_len = 0;
        run_sphere = ~0u;
    };
    for (std::uint32_t b = 0; b < depth; ++b) {
        ++seg;
        std::uint32_t idx = ~0u;
        hit h = hit_world_index(sc, r, idx);
        bool trapped_hit = false;
        float cosv = 0.f;
        if (h.ok && sc.m[h.mat].kind == RT_DIELECTRIC) {
            // the quantities of apply_material's dielectric branch (raytracer.hxx:158-194)
            const v3 ud = normalize(r.d);
            cosv = dot(ud, h.n);
            if (cosv > 0.f) {
                const v3 refr = refract(ud, neg(h.n), sc.m[h.mat].param);
                trapped_hit = refr.x != refr.x;  // NaN: k < 0, reflected with probability 1
            }
        }
        if (fired_at && !(trapped_hit && idx == fired_sphere)) broke = true;
        if (trapped_hit && idx == run_sphere) {
            ++run_len;
            run_min = std::min(run_min, cosv);
            run_max = std::max(run_max, cosv);
        } else {
            end_run();
            if (trapped_hit) {
                run_sphere = idx;
                run_len = 1;
                run_min = run_max = cosv;
            }
        }
        // the trigger: a hit that would be shaded (seg < depth), ordered compares
        if (!fired_at && trapped_hit && seg < depth && depth <= rt::kTrapDepth && cosv >= win[2 * idx] &&
            cosv <= win[2 * idx + 1]) {
            fired_at = seg;
            fired_sphere = idx;
        }
        if (!h.ok) {
            result = mulv(background(.5f * normalize(r.d).y + 1.f), atten);
            used_up = false;
            break;
        }
        ray nr; v3 e;
        if (!apply_material(sc, g, r, h, nr, e)) {
            used_up = false;
            break;
        }
        r = nr;
        atten = mulv(atten, e);
    }
    if (run_len) {
        if (used_up) ++t.tir_run_ends;
        end_run();
    }
    ++t.paths;
    t.segments += seg;
    if (used_up) ++t.maxdepth_paths;
    if (fired_at) {
        ++t.fired;
        t.saved += depth - fired_at;
        const bool zero = result.x == 0.f && result.y == 0.f && result.z == 0.f;
        if (broke || !used_up || seg != depth || !zero) ++t.violations;
        else ++t.fired_maxdepth;
    }
    return result;
}

void print(const char *tag, const tally &t)
{
    std::printf("%s paths=%llu segments=%llu maxdepth_paths=%llu tir_run_ends=%llu fired=%llu fired_maxdepth=%llu "
                "violations=%llu saved=%llu tir_runs=%llu drift=%.9g drift_scaled=%.9g\n",
                tag, (unsigned long long)t.paths, (unsigned long long)t.segments, (unsigned long long)t.maxdepth_paths,
                (unsigned long long)t.tir_run_ends, (unsigned long long)t.fired, (unsigned long long)t.fired_maxdepth,
                (unsigned long long)t.violations, (unsigned long long)t.saved, (unsigned long long)t.tir_runs, t.drift,
                t.drift_scaled);
}

int frame(std::uint32_t W, std::uint32_t H, std::uint32_t spp, bool corrected, int threads)
{
    std::uint32_t ns = 0, nm = 0;
    rt_scene_huge(1234, nullptr, 0, &ns, nullptr, 0, &nm);
    std::vector<rt_sphere> s(ns);
    std::vector<rt_material> m(nm);
    if (rt_scene_huge(1234, s.data(), ns, &ns, m.data(), nm, &nm) != RT_OK) return 2;
    const std::vector<float> win = rthost::trap_windows(s.data(), ns, m.data());
    std::uint32_t n_glass = 0, n_win = 0;
    float lo_min = 1.f, hi_max = 0.f, lo_max = 0.f, hi_min = 1.f;
    for (std::uint32_t i = 0; i < ns; ++i) {
        if (m[s[i].material].kind == RT_DIELECTRIC) ++n_glass;
        if (win[2 * i] <= win[2 * i + 1]) {
            ++n_win;
            lo_min = std::min(lo_min, win[2 * i]); lo_max = std::max(lo_max, win[2 * i]);
            hi_min = std::min(hi_min, win[2 * i + 1]); hi_max = std::max(hi_max, win[2 * i + 1]);
        }
    }
    std::printf("scene spheres=%u glass=%u windows=%u cos_lo=%.6f..%.6f cos_hi=%.6f..%.6f drift_k=%g\n", ns, n_glass, n_win,
                lo_min, lo_max, hi_min, hi_max, rt::kTrapDriftK);
    rt_camera camera;
    if (rt_camera_default(W, H, corrected ? RT_CAMERA_CORRECTED : RT_CAMERA_REFERENCE, &camera) != RT_OK) return 2;
    const cam c = to_cam(&camera);
    const scene sc{s.data(), ns, m.data(), nm};
    const std::uint32_t depth = 64;
    const std::uint64_t seed = 1234;
    if (threads < 1) threads = 1;
    std::vector<tally> part(threads);
    auto worker = [&](int tid) {
        pcg32 gd, gc;
        tally t;
        for (std::uint32_t y = tid; y < H; y += threads) {
            const float v = static_cast<float>(y) / static_cast<float>(H);
            for (std::uint32_t x = 0; x < W; ++x) {
                const float u = static_cast<float>(x) / static_cast<float>(W);
                for (std::uint32_t k = 0; k < spp; ++k) {
                    const std::uint64_t key = (static_cast<std::uint64_t>(y) * W + x) * spp + k;
                    gd.seed(key, 2u * seed);
                    gc.seed(key, 2u * seed + 1u);
                    const float uu = u + canonical(gd) / static_cast<float>(W);
                    const float vv = v + canonical(gd) / static_cast<float>(H);
                    color_checked(sc, win, gd, camera_ray(c, gc, uu, vv), depth, t);
                }
            }
        }
        part[tid] = t;
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; ++t) pool.emplace_back(worker, t);
    worker(0);
    for (auto &t : pool) t.join();
    tally all;
    for (const tally &t : part) all += t;
    print("frame", all);
    return all.violations ? 1 : 0;
}

// a float moved by k units in the last place
inline float ulps(float x, int k)
{
    for (; k > 0; --k) x = std::nextafter(x, FLT_MAX);
    for (; k < 0; ++k) x = std::nextafter(x, -FLT_MAX);
    return x;
}

// Single balls over a far ground, rays started on the ball a few ulp off its surface with the
// cosine to the inward normal set on, just inside and just outside both window ends and across
// the window. A ball whose window is empty fires nowhere; its rays are still traced.
int adversarial()
{
    const float iors[2] = {1.33f, 1.5f};
    const float radii[3] = {0.1f, 0.2f, 1.0f};
    const float centres[3][3] = {{0.f, 0.f, 0.f}, {3.1f, 0.2f, -7.3f}, {500.f, 0.2f, -300.f}};
    int rc = 0;
    for (float ior : iors)
        for (float rad : radii)
            for (const auto &C : centres) {
                rt_material m[2] = {{RT_LAMBERT, {.5f, .5f, .5f}, 0.f}, {RT_DIELECTRIC, {1.f, 1.f, 1.f}, ior}};
                rt_sphere s[2] = {{{C[0], C[1] - rad - 0.05f * rad - 1000.f, C[2]}, 1000.f, 0}, {{C[0], C[1], C[2]}, rad, 1}};
                const std::vector<float> win = rthost::trap_windows(s, 2, m);
                const bool empty = !(win[2] <= win[3]);
                const scene sc{s, 2, m, 2};
                tally t;
                pcg32 g;
                g.seed(static_cast<std::uint64_t>(ior * 1000.f) * 7919u + static_cast<std::uint64_t>(rad * 100.f), 77);
                // the cosines tried: the ends, a few ulp and 1e-4 either side of them, the margin's
                // width outside them, and the span of the window (of a default one when it is empty)
                const float lo = empty ? 0.05f : win[2], hi = empty ? 0.7f : win[3];
                std::vector<float> cs;
                for (float e : {lo, hi})
                    for (int k : {-64, -4, -1, 0, 1, 4, 64}) cs.push_back(ulps(e, k));
                for (float e : {lo, hi})
                    for (float dlt : {-1e-2f, -1e-3f, -1e-4f, 1e-4f, 1e-3f, 1e-2f}) cs.push_back(e + dlt);
                for (int k = 0; k <= 24; ++k) cs.push_back(lo + (hi - lo) * static_cast<float>(k) / 24.f);
                const int per = 4096 / static_cast<int>(cs.size()) + 1;
                for (float c : cs) {
                    if (!(c > 0.f && c < 1.f)) continue;
                    for (int k = 0; k < per; ++k) {
                        // a point of the ball, a few ulp off its surface in every coordinate
                        const v3 n = normalize(random_in_unit_sphere(g));
                        v3 p = add(mk(C[0], C[1], C[2]), muls(n, rad));
                        p.x = ulps(p.x, static_cast<int>(g.next() % 7u) - 3);
                        p.y = ulps(p.y, static_cast<int>(g.next() % 7u) - 3);
                        p.z = ulps(p.z, static_cast<int>(g.next() % 7u) - 3);
                        // a unit tangent, then the direction at cosine c to the inward normal
                        v3 tg = cross(n, normalize(random_in_unit_sphere(g)));
                        if (!(length(tg) > 1e-3f)) continue;
                        tg = normalize(tg);
                        const v3 d = add(muls(n, -c), muls(tg, std::sqrt(1.f - c * c)));
                        color_checked(sc, win, g, ray{p, d}, 64, t);
                    }
                }
                char tag[128];
                std::snprintf(tag, sizeof tag, "ball ior=%.2f r=%.1f c=%.0f window=%.6f..%.6f", ior, rad, C[0], win[2], win[3]);
                print(tag, t);
                if (t.violations) rc = 1;
            }
    return rc;
}

} // namespace

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "frame" && argc == 7)
        return frame(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]) != 0, std::atoi(argv[6]));
    if (mode == "adversarial") return adversarial();
    std::fprintf(stderr, "usage: trap_census frame W H spp corrected threads | trap_census adversarial\n");
    return 2;
}
