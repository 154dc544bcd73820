// TEST INFRASTRUCTURE ONLY (tests/test_sanitize_cpu.py): drives the host-only half of the
// library (raytracinginoneweekend_amd/csrc/rt_host_build.cpp and rt_plan.cpp, compiled from the same source
// with -fsanitize=address,undefined or -fsanitize=thread by tests/sanitize/Makefile) and the CPU
// restatement (oracle/rt_oracle.cpp) through their real inputs, and checks the results against
// the reference's fixtures in tests/golden. Any sanitizer report fails the run (halt on error).
//
//   host_check host <golden dir>        scene generators vs the reference's scene dumps, camera
//                                       vs the restatement, cluster/neighbour-list builder on the
//                                       huge scene and adversarial scenes, the scene derivation bit
//                                       for bit (derive_scene), exact-division checks,
//                                       the synchronous calls' plane layout, the pass planner's cuts,
//                                       options parser (fixed and random strings), PPM writer
//   host_check render <scene.bin> <golden.f32> W H spp depth seed row0 stride rows mode threads
//                                       the restatement's render vs a golden frame, bit for bit
//   host_check threads <scene.bin>      (TSan) the restatement on 1 and 4 threads, the exact-division
//                                       cache and the options defaults from several threads
#include <cmath>
#include <cstdint>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

#include "../../raytracinginoneweekend_amd/csrc/rt_host_build.h"
#include "../../raytracinginoneweekend_amd/csrc/rt_plan.h"

extern "C" {
int oracle_render_f32(const rt_sphere *, uint32_t, const rt_material *, uint32_t, const rt_camera *, const rt_params *,
                      int rng_mode, int threads, float *out, uint64_t *segments_out);
int oracle_camera_default(uint32_t width, uint32_t height, uint32_t mode, rt_camera *out);
}

namespace {

int g_fail = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                                         \
        }                                                                     \
    } while (0)

std::vector<char> read_file(const std::string &p)
{
    std::ifstream f(p, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// RTSC v1 scene file (raytracinginoneweekend_amd/_abi.py save_scene_file)
bool load_scene(const std::string &p, std::vector<rt_sphere> &s, std::vector<rt_material> &m)
{
    const std::vector<char> b = read_file(p);
    if (b.size() < 16) return false;
    uint32_t h[4];
    std::memcpy(h, b.data(), 16);
    if (h[0] != 0x43535452u || h[1] != 1u || b.size() != 16u + 20u * (h[2] + h[3])) return false;
    s.resize(h[2]);
    m.resize(h[3]);
    std::memcpy(s.data(), b.data() + 16, 20u * h[2]);
    std::memcpy(m.data(), b.data() + 16 + 20u * h[2], 20u * h[3]);
    return true;
}

void check_scene_generators(const std::string &golden)
{
    std::vector<rt_sphere> gs, s(1024);
    std::vector<rt_material> gm, m(1024);
    uint32_t ns = 0, nm = 0;
    CHECK(load_scene(golden + "/scene_huge_1234.bin", gs, gm));
    CHECK(rt_scene_huge(1234, s.data(), 1024, &ns, m.data(), 1024, &nm) == RT_OK);
    CHECK(ns == gs.size() && nm == gm.size());
    CHECK(ns == gs.size() && std::memcmp(s.data(), gs.data(), ns * sizeof(rt_sphere)) == 0);
    CHECK(nm == gm.size() && std::memcmp(m.data(), gm.data(), nm * sizeof(rt_material)) == 0);
    CHECK(rt_scene_huge(1234, s.data(), 10, &ns, m.data(), 1024, &nm) == RT_ERR_CAPACITY);
    CHECK(rt_scene_huge(1234, nullptr, 0, &ns, nullptr, 0, &nm) == RT_OK && ns == gs.size());
    for (uint32_t seed : {0u, 1u, 7u, 0xffffffffu}) CHECK(rt_scene_huge(seed, s.data(), 1024, &ns, m.data(), 1024, &nm) == RT_OK);
    CHECK(load_scene(golden + "/scene_simple.bin", gs, gm));
    CHECK(rt_scene_simple(s.data(), 1024, &ns, m.data(), 1024, &nm) == RT_OK);
    CHECK(ns == gs.size() && std::memcmp(s.data(), gs.data(), ns * sizeof(rt_sphere)) == 0);
    CHECK(rt_scene_cuda(s.data(), 1024, &ns, m.data(), 1024, &nm) == RT_OK && ns == 5 && nm == 4);
}

void check_cameras()
{
    for (uint32_t W : {1u, 64u, 200u, 1280u, 3840u})
        for (uint32_t H : {1u, 36u, 100u, 720u, 2160u})
            for (uint32_t mode : {0u, 1u}) {
                rt_camera a{}, b{};
                CHECK(rt_camera_default(W, H, mode, &a) == RT_OK);
                CHECK(oracle_camera_default(W, H, mode, &b) == RT_OK);
                CHECK(std::memcmp(&a, &b, sizeof a) == 0);
            }
    rt_camera c{};
    CHECK(rt_camera_default(0, 10, 0, &c) == RT_ERR_INVALID);
    CHECK(rt_camera_cuda(64, 36, &c) == RT_OK);
    const float p[3] = {1, 2, 3};
    CHECK(rt_camera_init(p, p, p, 1.f, 90.f, 0.f, 1.f, 2u, &c) == RT_ERR_INVALID);
    CHECK(rt_camera_init(nullptr, p, p, 1.f, 90.f, 0.f, 1.f, 0u, &c) == RT_ERR_INVALID);
}

// every sphere appears exactly once: in the always-tested list or in one cluster's members
void check_blob(const std::vector<rt_sphere> &s, const std::vector<rt_material> &m, bool clustered, uint32_t csize)
{
    const uint32_t n = static_cast<uint32_t>(s.size());
    const rthost::blob_t b = rthost::build_blob(s.data(), n, clustered, csize);
    CHECK(b.n_geo % 4 == 0 && b.data.size() % 4 == 0);
    CHECK(b.clus_offset * 4u <= b.data.size() && b.supers_offset * 4u <= b.data.size());
    std::vector<int> seen(n, 0);
    for (uint32_t g = 0; g < b.n_geo; ++g) {
        uint32_t id;
        std::memcpy(&id, &b.data[4u * b.n_geo + g], 4);
        if (id != 0xffffffffu) {
            CHECK(id < n);
            if (id < n) ++seen[id];
        }
    }
    for (uint32_t i = 0; i < n; ++i) CHECK(seen[i] == 1);
    // cluster records: members inside the geo list, at most the cluster size
    for (uint32_t c = 0; c < b.n_clusters; ++c) {
        uint32_t packed;
        std::memcpy(&packed, &b.data[4u * (b.clus_offset + 2u * c) + 7u], 4);
        const uint32_t start = packed & 0xffffu, cnt = packed >> 16;
        CHECK(cnt <= ((csize + 3u) & ~3u) && start + cnt <= b.n_geo);
    }
    const std::vector<uint32_t> w = rthost::shortcut_words(s.data(), n, m.data(), b, false);
    const std::vector<uint32_t> w0 = rthost::shortcut_words(s.data(), n, m.data(), b, true);
    CHECK(w.size() == n && w0.size() == n);
    for (uint32_t i = 0; i < n; ++i) {
        if (!(w[i] & rt::kShortcut)) continue;
        CHECK(m[s[i].material].kind == RT_DIELECTRIC);
        const uint32_t n0 = w[i] & 0x7fffu, n1 = (w[i] >> 15) & 0x7fffu;
        CHECK(n0 <= b.n_geo && n1 <= b.n_geo);
        CHECK(!w0[i] || (w0[i] == rt::kShortcut && !n0));  // isolated only without neighbours
    }
}

void check_builders(const std::string &golden)
{
    std::vector<rt_sphere> s;
    std::vector<rt_material> m;
    CHECK(load_scene(golden + "/scene_huge_1234.bin", s, m));
    for (uint32_t cs = 4; cs <= 64; cs += 4) check_blob(s, m, true, cs);
    check_blob(s, m, false, 16);
    {   // the huge scene's walk shortcut (155 of its 157 glass balls)
        const rthost::blob_t b = rthost::build_blob(s.data(), static_cast<uint32_t>(s.size()), true, 16);
        const std::vector<uint32_t> w = rthost::shortcut_words(s.data(), static_cast<uint32_t>(s.size()), m.data(), b, false);
        uint32_t k = 0;
        for (uint32_t x : w) k += (x & rt::kShortcut) ? 1u : 0u;
        CHECK(k >= 150 && k <= 157);
    }
    // adversarial scenes: duplicates, zero / negative / huge radii, non-finite and far centres,
    // touching glass balls, fewer spheres than a cluster
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> U(-20.f, 20.f);
    for (uint32_t n : {0u, 1u, 5u, 31u, 32u, 33u, 300u, 2000u}) {
        std::vector<rt_sphere> t(n);
        std::vector<rt_material> mm = {{RT_LAMBERT, {.5f, .5f, .5f}, 0.f}, {RT_DIELECTRIC, {1, 1, 1}, 1.5f},
                                       {RT_METAL, {.7f, .6f, .5f}, .2f}};
        for (uint32_t i = 0; i < n; ++i) {
            t[i] = {{U(rng), std::fabs(U(rng)) * .05f, U(rng)}, .2f, i % 3u};
            if (i % 17 == 3 && i) t[i] = t[i - 1];                       // duplicate
            if (i % 29 == 5) t[i].radius = -.15f;                       // bubble
            if (i % 41 == 7) t[i].radius = 0.f;
            if (i % 53 == 11) t[i].center[0] = 7e5f;                    // far from the origin
            if (i % 97 == 13) t[i].center[1] = INFINITY;                // non-finite
            if (i % 89 == 17) t[i].radius = 3000.f;                     // huge (always tested)
        }
        check_blob(t, mm, true, 16);
        check_blob(t, mm, true, 4);
        check_blob(t, mm, false, 16);
    }
}

// 64-bit FNV-1a over the bytes of an array
template <class T> uint64_t fnv1a(const std::vector<T> &v)
{
    uint64_t h = 14695981039346656037ull;
    const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

struct DeriveCase {
    std::vector<rt_sphere> s;
    std::vector<rt_material> m;
};

// the huge scene, the simple scene, an adversarial scene (a negative radius, a centre beyond 2^19,
// a radius below 2^-40, glass of several indices of refraction, touching and nested balls) and
// the scene without spheres
std::vector<DeriveCase> derive_cases(const std::string &golden)
{
    std::vector<DeriveCase> c(4);
    CHECK(load_scene(golden + "/scene_huge_1234.bin", c[0].s, c[0].m));
    c[1].s.resize(1024);
    c[1].m.resize(1024);
    uint32_t ns = 0, nm = 0;
    CHECK(rt_scene_simple(c[1].s.data(), 1024, &ns, c[1].m.data(), 1024, &nm) == RT_OK);
    c[1].s.resize(ns);
    c[1].m.resize(nm);
    c[2].m = {{RT_LAMBERT, {.5f, .5f, .5f}, 0.f},   {RT_DIELECTRIC, {1, 1, 1}, 1.5f}, {RT_METAL, {.7f, .6f, .5f}, .2f},
              {RT_DIELECTRIC, {1, 1, 1}, 1.33f},    {RT_DIELECTRIC, {1, 1, 1}, 2.4f}, {RT_DIELECTRIC, {1, 1, 1}, 1.f},
              {RT_DIELECTRIC, {1, 1, 1}, 0.75f}};
    c[2].s = {{{0.f, -1000.f, 0.f}, 1000.f, 0u}, {{0.f, 1.f, 0.f}, 1.f, 1u},      {{0.f, 1.f, 0.f}, -.9f, 1u},
              {{4.f, 1.f, 0.f}, 1.f, 2u},        {{-4.f, 1.f, 0.f}, 1.f, 3u},     {{600000.f, 1.f, 2.f}, .5f, 4u},
              {{2.f, .2f, 2.f}, 0x1p-41f, 5u},   {{-2.f, .2f, 2.f}, .2f, 6u},     {{-2.f, .2f, 2.4f}, .2f, 4u},
              {{1.f, .2f, -3.f}, .2f, 0u},       {{1.5f, .2f, -3.f}, .2f, 3u},    {{7.f, .3f, 7.f}, .3f, 1u}};
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> U(-11.f, 11.f);
    for (uint32_t i = 0; i < 60; ++i) c[2].s.push_back({{U(rng), .2f, U(rng)}, .2f, i % 7u});
    c[3].m = {{RT_LAMBERT, {.5f, .5f, .5f}, 0.f}};
    return c;
}

// What a scene derives from its records (rthost::derive_scene), bit for bit: every derived array's
// hash and the three flags, per scene under the default options and under RT_DIAG_NO_TRAP_END |
// RT_DIAG_NO_NEIGHBOURS. The constants are those of derive_scene as it stood in rt_host.cpp at
// 152caca, before it moved to rt_host_build.cpp (profiles/hostsplit/derive_words.txt says how they
// were obtained): the device scenes, and so the golden frames, depend on these bits.
void check_derive(const std::string &golden)
{
    static const struct {
        uint64_t blob0, blob1, trap, geom_words, table, flat;
        bool in_fast_range, has_geom, ground_ok;
    } want[8] = {
        {0x4f54fa9e42869b78ull, 0xf6dbc24cb6371f5dull, 0x5a2f61fcb595ff19ull, 0x529f39df29530df0ull, 0x93a14d825fcc0e29ull, 0x1c6ef68951427301ull, 1, 1, 1},
        {0xef307f7c23635578ull, 0x2d4351f3ed79d18dull, 0x0d04cfbaaec761e5ull, 0x529f39df29530df0ull, 0x93a14d825fcc0e29ull, 0x1c6ef68951427301ull, 1, 1, 1},
        {0xcc4faec9cd58d405ull, 0xcc4faec9cd58d405ull, 0x97cf91e389d7ac45ull, 0xc51bf4eb83b97b3bull, 0x182bf30f88f5454cull, 0xba20e3a2ac7d5aafull, 1, 0, 0},
        {0xcc4faec9cd58d405ull, 0xcc4faec9cd58d405ull, 0x97cf91e389d7ac45ull, 0xc51bf4eb83b97b3bull, 0x182bf30f88f5454cull, 0xba20e3a2ac7d5aafull, 1, 0, 0},
        {0xbedbbcca4f38924cull, 0xabce91f71a5ceb15ull, 0x7b0bc7bfbb4e4ed6ull, 0x59c8f52c39ff7f86ull, 0x53b1d16a6260063aull, 0x4d8d746c3a842f12ull, 0, 1, 1},
        {0xbedbbcca4f38924cull, 0xabce91f71a5ceb15ull, 0x5a640bd8e7221825ull, 0x59c8f52c39ff7f86ull, 0x53b1d16a6260063aull, 0x4d8d746c3a842f12ull, 0, 1, 1},
        {0x24a95cb574ab082bull, 0x24a95cb574ab082bull, 0x6af9b6af0b2793c5ull, 0x09f6eaf179126bd8ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 1, 0, 0},
        {0x24a95cb574ab082bull, 0x24a95cb574ab082bull, 0x6af9b6af0b2793c5ull, 0x09f6eaf179126bd8ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 1, 0, 0},
    };
    const std::vector<DeriveCase> cases = derive_cases(golden);
    for (size_t i = 0; i < cases.size(); ++i)
        for (uint32_t v = 0; v < 2u; ++v) {
            rt_options o = rthost::library_defaults();
            o.diag = v ? uint32_t(RT_DIAG_NO_TRAP_END | RT_DIAG_NO_NEIGHBOURS) : 0u;
            const DeriveCase &c = cases[i];
            const uint32_t n = static_cast<uint32_t>(c.s.size());
            CHECK(rthost::check_records("host_check", c.s.data(), n, c.m.data(), static_cast<uint32_t>(c.m.size())) == RT_OK);
            rthost::SceneDerived d;
            rthost::derive_scene(c.s.data(), n, c.m.data(), o, d);
            const auto &w = want[2 * i + v];
            CHECK(fnv1a(d.blobs[0].data) == w.blob0 && fnv1a(d.blobs[1].data) == w.blob1);
            CHECK(fnv1a(d.trap) == w.trap && fnv1a(d.geom_words) == w.geom_words);
            CHECK(fnv1a(d.table) == w.table && fnv1a(d.flat) == w.flat);
            CHECK(d.in_fast_range == w.in_fast_range && d.has_geom == w.has_geom && d.ground_ok == w.ground_ok);
            for (const rthost::blob_t &b : d.blobs) CHECK(b.units == b.data.size() / 4u && b.shade_offset <= b.units);
            CHECK(d.table.size() == 4u * n && d.flat.size() == 5u * n && d.trap.size() == 4u * std::max(n, 1u));
        }
    // the records' checks refuse a material index past the table and an unknown kind
    const rt_sphere s1 = {{0.f, 0.f, 0.f}, 1.f, 1u};
    const rt_material m1 = {RT_LAMBERT, {.5f, .5f, .5f}, 0.f}, m2 = {RT_DIELECTRIC + 1u, {1, 1, 1}, 1.f};
    CHECK(rthost::check_records("host_check", &s1, 1, &m1, 1) == RT_ERR_INVALID);
    CHECK(rthost::check_records("host_check", nullptr, 0, &m2, 1) == RT_ERR_INVALID);
}

// tile classes: the frame-sized classification runs on several threads (each
// writes its own tiles; TSAN checks that), a row share's on one; the frame's is a permutation,
// the same on every run, with the classes' counts in range
void check_tiles(const std::string &golden)
{
    std::vector<rt_sphere> s;
    std::vector<rt_material> m;
    CHECK(load_scene(golden + "/scene_huge_1234.bin", s, m));
    const rthost::blob_t b = rthost::build_blob(s.data(), static_cast<uint32_t>(s.size()), true, 16);
    const rthost::scene_geom g = rthost::scene_geometry(s.data(), b);
    rt_camera cam{};
    CHECK(rt_camera_default(1280, 720, RT_CAMERA_REFERENCE, &cam) == RT_OK);
    const rthost::tile_order a = rthost::classify_tiles(cam, 1280, 720, 0, 1, 720, 3u, g);
    const rthost::tile_order a2 = rthost::classify_tiles(cam, 1280, 720, 0, 1, 720, 3u, g);
    CHECK(a.perm.size() == 14400u && a.perm == a2.perm && a.n_lead == a2.n_lead && a.n_sky == a2.n_sky);
    std::vector<uint32_t> sorted = a.perm;
    std::sort(sorted.begin(), sorted.end());
    for (uint32_t i = 0; i < sorted.size(); ++i) CHECK(sorted[i] == i);
    CHECK(a.n_lead >= 161u && a.n_sky >= 10000u && a.n_lead + a.n_sky <= 14400u);
    // rows 8 j (share 0 of 8; 90 rows): 11 tile rows of 160 tiles (8 x 8 tiles over the packed rows)
    const rthost::tile_order sh = rthost::classify_tiles(cam, 1280, 720, 0, 8, 90, 3u, g);
    CHECK(sh.perm.size() == 1800u);  // 1280 x 90 / 64 blocks
    CHECK(sh.n_sky > 0u && sh.n_sky < 1800u);
}

void check_divisions()
{
    std::mt19937 rng(9);
    for (uint32_t d : {1u, 2u, 3u, 7u, 8u, 100u, 720u, 1280u, 2160u, 3840u, 65535u, 921600u, 0x7fffffffu, 0xffffffffu}) {
        const rt::UDiv u = rthost::make_udiv(d);
        for (int k = 0; k < 20000; ++k) {
            const uint32_t n = k < 10 ? 0xffffffffu - static_cast<uint32_t>(k) : rng();
            const uint32_t t = static_cast<uint32_t>((static_cast<uint64_t>(n) * u.m) >> 32);
            const uint32_t q = (t + ((n - t) >> u.s1)) >> u.s2;
            CHECK(q == n / d);
            if (q != n / d) break;
        }
    }
    for (float b : {1.f, 200.f, 100.f, 720.f, 1280.f}) CHECK(rthost::exact_by_reciprocal(b));
    CHECK(!rthost::exact_by_reciprocal(0.f) && !rthost::exact_by_reciprocal(-3.f) && !rthost::exact_by_reciprocal(NAN));
}

// the synchronous calls' device planes (rthost::plane_layout): the planes that are there packed in
// table order from 0, every offset a multiple of 256, none overlapping, absent ones left alone
void check_plane_layout()
{
    using rthost::Plane;
    int host = 0;  // any address: a given plane
    CHECK(rthost::plane_layout(nullptr, 0, 24u * 16u) == 0u);
    {   // absent planes in the middle take no room and keep their offset
        Plane t[5] = {rthost::plane_in(&host, 12), rthost::plane_in(nullptr, 12), rthost::plane_scratch(false, 12),
                      rthost::plane_out(nullptr, 4), rthost::plane_out(&host, 4)};
        t[1].at = t[2].at = t[3].at = 77u;
        CHECK(t[0].kind == Plane::In && t[1].kind == Plane::Absent && t[2].kind == Plane::Absent &&
              t[3].kind == Plane::Absent && t[4].kind == Plane::Out);
        CHECK(rthost::plane_layout(t, 5, 100u) == 1280u + 512u);
        CHECK(t[0].at == 0u && t[4].at == 1280u && t[1].at == 77u && t[2].at == 77u && t[3].at == 77u);
        CHECK(!t[0].dev && !t[4].dev);
    }
    {   // one pixel: every plane is one 256-byte unit
        Plane t[4] = {rthost::plane_in(&host, 12), rthost::plane_out(&host, 4), rthost::plane_scratch(true, 8),
                      rthost::plane_out(&host, 3)};
        CHECK(rthost::plane_layout(t, 4, 1u) == 1024u);
        for (size_t i = 0; i < 4; ++i) CHECK(t[i].at == 256u * i);
    }
    {   // a 3-channel and a 1-channel float plane of a 5x3 image
        Plane t[2] = {rthost::plane_out(&host, 12), rthost::plane_out(&host, 4)};
        CHECK(rthost::plane_layout(t, 2, 5u * 3u) == 512u);
        CHECK(t[0].at == 0u && t[1].at == 256u);
    }
    {   // an empty image: every plane at 0, nothing taken
        Plane t[2] = {rthost::plane_out(&host, 12), rthost::plane_out(&host, 3)};
        CHECK(rthost::plane_layout(t, 2, 0u) == 0u && t[0].at == 0u && t[1].at == 0u);
    }
    {   // the temporal call's fifteen planes at 24x16: increasing, aligned, not overlapping, the total their end
        const uint32_t px[15] = {12, 4, 12, 4, 4, 4, 12, 4, 4, 12, 4, 4, 12, 4, 4};
        const size_t n = 24u * 16u;
        Plane t[15];
        for (int i = 0; i < 15; ++i) t[i] = i < 12 ? rthost::plane_in(&host, px[i]) : rthost::plane_out(&host, px[i]);
        const size_t total = rthost::plane_layout(t, 15, n);
        CHECK(t[0].at == 0u);
        for (int i = 0; i < 15; ++i) {
            CHECK(t[i].at % 256u == 0u);
            const size_t end = t[i].at + n * px[i], next = i + 1 < 15 ? t[i + 1].at : total;
            CHECK(end <= next && next - end < 256u);
        }
        CHECK(total % 256u == 0u);
        // without the previous frame the outputs follow the current planes directly
        for (int i = 6; i < 12; ++i) t[i] = rthost::plane_in(nullptr, px[i]);
        const size_t without = rthost::plane_layout(t, 15, n);
        CHECK(t[12].at == t[5].at + 1536u && without < total);
    }
}

void check_options()
{
    rt_options o;
    CHECK(rt_options_default(&o) == RT_OK);
    CHECK(rt_options_parse("render_streams=3,max_workspace_bytes=4294967296, stats=1", &o) == RT_OK);
    CHECK(o.render_streams == 3 && o.max_workspace_bytes == (1ull << 32) && (o.diag & RT_DIAG_STATS));
    const char *bad[] = {"x", "=", "render_streams=", "=3", "render_streams=99", "cluster_size=5", "diag=999999",
                         "max_pass_bytes=18446744073709551615", "deep_split=-1", "verbose=2", ",,,render_streams=1x"};
    for (const char *b : bad) {
        rt_options t = o;
        CHECK(rt_options_parse(b, &t) == RT_ERR_INVALID);
        CHECK(std::memcmp(&t, &o, sizeof t) == 0);
        CHECK(std::strlen(rt_last_error()) > 0);
    }
    std::mt19937 rng(3);
    const char alphabet[] = "render_streams=0123456789,x;= \t_dplitagqkmbsvwe";
    for (int k = 0; k < 20000; ++k) {  // random text: never crashes, never leaves a bad record
        std::string t(rng() % 48, ' ');
        for (char &c : t) c = alphabet[rng() % (sizeof alphabet - 1)];
        rt_options r;
        rt_options_default(&r);
        if (rt_options_parse(t.c_str(), &r) == RT_OK) CHECK(rthost::check_options(r) == RT_OK);
    }
    CHECK(rt_set_default_options(&o) == RT_OK);
    rt_options d{};
    CHECK(rt_get_default_options(&d) == RT_OK && std::memcmp(&d, &o, sizeof d) == 0);
    CHECK(rt_set_default_options(nullptr) == RT_OK);
    o.size = 3;
    CHECK(rt_set_default_options(&o) == RT_ERR_INVALID);
}

// The pass planner (rt_plan.cpp) against its documented rules (the comments there, DESIGN.md §4.2
// and §4.14), none of them taken from its own output.
void check_plans()
{
    using rthost::Plan;
    using rthost::PlanInput;
    const rt_options D = rthost::library_defaults();
    auto input = [&](uint64_t n_pixels, uint32_t spp, uint32_t streams, uint32_t wsps) {
        return PlanInput{n_pixels, spp, streams, wsps, D.max_pass_bytes, 0, D.ring_pass_bytes, D.wave_queue_rays,
                         false, false, true, false, true};
    };
    // ring passes: the frame's samples in equal passes of a multiple of 4 within ring_pass_bytes,
    // at least 32; the frame issued alone then runs whole in a workspace of its own
    {
        const uint64_t per_sample = 160u * 90u * 12u;
        const struct { uint64_t ring; uint64_t pass; bool lone; } cases[] = {{40, 32, true}, {64, 48, true}, {28, 96, false}};
        for (const auto &c : cases) {
            PlanInput in = input(160u * 90u, 96, 3, 2);
            in.ring_pass_bytes = c.ring * per_sample;
            Plan pl{};
            CHECK(rthost::plan_frame(in, pl) == RT_OK);
            CHECK(pl.ring_samples == c.pass && pl.lone_samples == 96u && pl.streams == 3u && pl.n_ws == 6u);
            CHECK(pl.has_lone() == c.lone && pl.whole == c.lone && !pl.pairs && !pl.ring_pairs);
            CHECK(pl.pass_samples(0) == c.pass && pl.slot_bytes(5) == c.pass * per_sample);
            if (c.lone) CHECK(pl.lone_ws == 6u && pl.pass_samples(6) == 96u && pl.slot_bytes(6) == 96u * per_sample);
        }
        // the defaults at config 3 with 7 streams: a 384 MiB ring holds 36 samples, 128 in 4 passes of 32
        CHECK(D.ring_pass_bytes == (384ull << 20) && D.workspaces_per_stream == 2u);
        Plan pl{};
        CHECK(rthost::plan_frame(input(1280u * 720u, 128, 7, D.workspaces_per_stream), pl) == RT_OK);
        CHECK(pl.ring_samples == 32u && pl.n_ws == 14u && pl.has_lone() && pl.lone_ws == 14u && pl.whole && pl.lone_samples == 128u);
    }
    // the cap: one workspace per stream first, then pairs, then shorter passes, then fewer streams
    auto deep_bytes = [](uint64_t n_pixels, uint64_t samples) {  // 8 regions of 1/1024 of the samples, at least 512, 60 B each
        return ((n_pixels + 255u) & ~255ull) + 8u * std::max<uint64_t>(512u, n_pixels * samples / 1024u) * 60u;
    };
    // slot rows of samples [a, b) by counting: a full block of 4 below spp & ~3 takes 2 rows as pairs, every other sample 1
    auto count_rows = [](uint32_t spp, uint32_t a, uint32_t b, bool paired) {
        uint64_t rows = 0;
        uint32_t s = a;
        if (paired)
            for (; s + 4u <= b && s + 4u <= (spp & ~3u); s += 4u) rows += 2u;
        return rows + (b - s);
    };
    // the largest pass of the frame cut into passes of `pass` samples
    auto most_rows = [&](uint32_t spp, uint64_t pass, bool paired) {
        uint64_t m = 0;
        for (uint64_t a = 0; a < spp; a += pass)
            m = std::max(m, count_rows(spp, static_cast<uint32_t>(a), static_cast<uint32_t>(std::min<uint64_t>(spp, a + pass)), paired));
        return m;
    };
    // The footprint of a cut from its fields alone, by the documented rules: the ring's workspaces
    // (12 B per slot row and pixel, and a deep queue when the passes may be split), the lone
    // passes' workspace of single samples (the whole frame, or a ring pass when the ring holds
    // pairs), the multi-pass sums (and moments), and the wavefront variant's two ray queues of
    // 52 B a ray with their counters.
    auto footprint_by_rules = [&](const PlanInput &in, const Plan &pl) {
        const uint64_t per_sample = in.n_pixels * 12u;
        auto workspace = [&](uint64_t samples, bool paired) {
            return most_rows(in.spp, samples, paired) * per_sample + (in.may_split ? deep_bytes(in.n_pixels, samples) : 0u);
        };
        const uint64_t n_ws = pl.streams > 1u ? pl.streams * pl.wsps : 1u;
        const bool ring_pairs = pl.pairs && pl.streams > 1u;
        uint64_t t = n_ws * workspace(pl.ring_samples, ring_pairs);
        if (pl.whole) t += workspace(pl.lone_samples, false);
        else if (ring_pairs) t += workspace(pl.ring_samples, false);
        if (pl.ring_samples < in.spp) t += (in.moments ? 2u : 1u) * per_sample;
        if (in.wave) t += 2u * std::min<uint64_t>(in.n_pixels * pl.lone_samples, in.wave_queue_rays) * 52u + 512u;
        return t;
    };
    // Every combination of the five flags, also those choose_kernel never produces (pairs with the
    // variance render; the wavefront variant with streams, pairs or a deep queue): the rules do
    // not depend on which combinations are reachable.
    int plans = 0, refused = 0, wholes = 0;
    for (uint64_t n_pixels : {64u, 2304u, 14400u})
        for (uint32_t spp : {1u, 3u, 4u, 7u, 16u, 64u, 96u, 130u})
            for (uint32_t streams : {1u, 3u, 7u})
                for (uint32_t wsps : {1u, 2u})
                    for (uint32_t flags = 0; flags < 64u; ++flags) {
                        PlanInput in = input(n_pixels, spp, streams, wsps);
                        in.moments = flags & 1u;
                        in.pairs_ok = flags & 2u;
                        in.pairs_forced = flags & 4u;
                        in.may_split = flags & 8u;
                        in.wave = flags & 16u;
                        // with and without ring passes (32 samples: the frames of 64 and more then run
                        // whole in a workspace of their own when issued alone)
                        if (flags & 32u) in.ring_pass_bytes = 32u * n_pixels * 12u;
                        const uint64_t per_sample = n_pixels * 12u, s4 = std::min(4u, spp);
                        const uint64_t dq4 = in.may_split ? deep_bytes(n_pixels, s4) : 0u;
                        const uint64_t sums = spp > 4u ? (in.moments ? 2u : 1u) * per_sample : 0u;
                        const uint64_t wave4 = in.wave ? 2u * std::min<uint64_t>(n_pixels * s4, in.wave_queue_rays) * 52u + 512u : 0u;
                        // one stream, one workspace, 4-sample passes of single samples
                        const uint64_t fp4 = s4 * per_sample + dq4 + sums + wave4;
                        for (uint64_t cap : {uint64_t(0), uint64_t(1), fp4 / 2u, fp4 - 1u, fp4, fp4 + 1u, 2u * fp4, 3u * fp4 + per_sample,
                                             5u * fp4, 8u * fp4, 13u * fp4, 21u * fp4, 40u * fp4, 100u * fp4}) {
                            in.max_workspace_bytes = cap;
                            Plan pl{};
                            const int rc = rthost::plan_frame(in, pl);
                            if (cap && fp4 > cap) {
                                CHECK(rc == RT_ERR_CAPACITY);
                                ++refused;
                                continue;
                            }
                            CHECK(rc == RT_OK);
                            if (rc != RT_OK) continue;
                            ++plans;
                            CHECK(pl.ring_samples <= pl.lone_samples && pl.lone_samples <= spp && pl.ring_samples >= 1u);
                            if (pl.ring_samples < spp) CHECK(pl.ring_samples % 4u == 0u);
                            if (pl.lone_samples < spp) CHECK(pl.lone_samples % 4u == 0u);
                            CHECK(pl.streams >= 1u && pl.streams <= in.streams && pl.wsps >= 1u && pl.wsps <= wsps);
                            CHECK(pl.n_ws == (pl.streams > 1u ? pl.streams * pl.wsps : 1u));
                            CHECK(!pl.pairs || in.pairs_ok);
                            CHECK(pl.ring_pairs == (pl.pairs && pl.streams > 1u));
                            if (in.pairs_ok && in.pairs_forced) CHECK(pl.pairs);
                            CHECK(pl.has_lone() == (pl.ring_pairs || pl.whole) && (!pl.has_lone() || pl.lone_ws == pl.n_ws));
                            // a whole lone frame only beside a ring of smaller passes
                            wholes += pl.whole;
                            if (pl.whole) CHECK(pl.streams > 1u && pl.lone_samples == spp && pl.ring_samples < spp);
                            const uint64_t by_rules = footprint_by_rules(in, pl);
                            if (cap) CHECK(by_rules <= cap);
                            CHECK(pl.footprint() == by_rules);
                            if (!cap) CHECK(pl.streams == in.streams && pl.wsps == wsps && pl.lone_samples == spp);
                            // pairs under the cap only after one workspace per stream
                            if (pl.pairs && !in.pairs_forced && pl.streams > 1u) CHECK(pl.wsps == 1u);
                            // shorter passes only after one workspace per stream and pairs
                            if (cap && pl.streams > 1u && pl.lone_samples < spp) CHECK(pl.wsps == 1u && (!in.pairs_ok || pl.pairs));
                            // fewer streams only when one more, at one workspace each, with pairs and
                            // 4-sample passes, does not fit
                            if (pl.streams < in.streams) {
                                const uint64_t S = pl.streams + 1u;
                                const uint64_t ring_rows = !in.pairs_ok ? s4 : spp >= 4u ? std::max<uint64_t>(2u, spp % 4u) : spp;
                                const uint64_t need = S * (ring_rows * per_sample + dq4) + (in.pairs_ok ? s4 * per_sample + dq4 : 0u) + sums + wave4;
                                CHECK(need > cap);
                            }
                        }
                    }
    CHECK(plans > 10000 && refused > 1000 && wholes > 1000);
    {  // the two failures' texts
        PlanInput in = input((1ull << 31) - 1u, 1, 3, 2);
        Plan pl{};
        CHECK(rthost::plan_frame(in, pl) == RT_ERR_INVALID);
        CHECK(std::string(rt_last_error()) == "rt_render_device: too many pixels in one call");
        in = input(2304, 16, 3, 2);
        in.max_workspace_bytes = 1000;
        CHECK(rthost::plan_frame(in, pl) == RT_ERR_CAPACITY);
        const uint64_t fp4 = 4u * 2304u * 12u + deep_bytes(2304, 4) + 2304u * 12u;
        CHECK(std::string(rt_last_error()) == "rt_render_device: max_workspace_bytes 1000 below one 4-sample pass of this frame (" +
                                                  std::to_string(fp4) + " bytes)");
    }
    // slot rows: each full block of 4 samples below spp & ~3 takes 2 rows as pairs, every other sample 1
    for (uint32_t spp = 1; spp <= 23u; ++spp) {
        Plan pl{};
        CHECK(rthost::plan_frame(input(64, spp, 1, 1), pl) == RT_OK);
        for (uint32_t a = 0; a <= spp; a += 4u)
            for (uint32_t b = a; b <= spp; ++b) {
                CHECK(pl.slot_rows(a, b, true) == count_rows(spp, a, b, true));
                CHECK(pl.slot_rows(a, b, false) == b - a);
            }
    }
    // the grid of a launch: occupancy 6 with 3 streams: 3 in flight, 6 alone; 4 streams and a short pass: a third
    CHECK(rthost::grid_wg_per_cu(6, true, 3, 1u << 20) == 3 && rthost::grid_wg_per_cu(6, true, 3, 1ull << 30) == 3);
    CHECK(rthost::grid_wg_per_cu(6, false, 3, 1u << 20) == 6);
    CHECK(rthost::grid_wg_per_cu(6, true, 4, rthost::kShortPassItems) == 2 && rthost::grid_wg_per_cu(6, true, 4, rthost::kShortPassItems + 1u) == 3);
    CHECK(rthost::grid_wg_per_cu(1, true, 7, 1) == 1 && rthost::grid_wg_per_cu(5, true, 1, 1) == 5);
    // the deep queue: 8 regions of 1/1024 of the samples, never below 512 entries, 60 B an entry,
    // after one flag byte per pixel rounded up to 256
    CHECK(rthost::deep_region_cap(0) == 512u && rthost::deep_region_cap(1000) == 512u && rthost::deep_region_cap(1024u * 512u) == 512u);
    CHECK(rthost::deep_region_cap(1024u * 513u) == 513u && rthost::deep_region_cap(1280ull * 720u * 128u) == 115200u);
    CHECK(rthost::deep_px_bytes(2304) == 2304u && rthost::deep_px_bytes(2590) == 2816u && rthost::deep_px_bytes(1) == 256u);
    CHECK(rthost::deep_queue_bytes(2304, 2304u * 16u) == 2304u + 8u * 512u * 60u);
    CHECK(rthost::guided_l2b(1024, true) < 0.f && rthost::guided_l2b(1024, false) > rthost::guided_l2b(1024, true));
}

void check_ppm(const std::string &golden)
{
    const std::vector<char> ref = read_file(golden + "/c1_simple_200x100_s1.ppm");
    const std::vector<char> u8 = read_file(golden + "/c1_simple_200x100_s1.u8");
    CHECK(u8.size() == 200u * 100u * 3u);
    const std::string path = std::string(std::getenv("TMPDIR") ? std::getenv("TMPDIR") : "/tmp") + "/host_check_" +
                             std::to_string(static_cast<long>(::getpid())) + ".ppm";
    CHECK(rt_write_ppm(path.c_str(), reinterpret_cast<const uint8_t *>(u8.data()), 200, 100) == RT_OK);
    const std::vector<char> mine = read_file(path);
    std::remove(path.c_str());
    const std::string hdr = "P6\n200 100\n255\n";
    CHECK(mine.size() == ref.size() && std::memcmp(mine.data(), hdr.data(), hdr.size()) == 0);
    CHECK(rt_write_ppm("/nonexistent-dir/x.ppm", reinterpret_cast<const uint8_t *>(u8.data()), 200, 100) == RT_ERR_IO);
    CHECK(rt_write_ppm(path.c_str(), nullptr, 4, 4) == RT_ERR_INVALID);
}

int render(int argc, char **argv)
{
    if (argc != 14) return 2;
    std::vector<rt_sphere> s;
    std::vector<rt_material> m;
    CHECK(load_scene(argv[2], s, m));
    const std::vector<char> want = read_file(argv[3]);
    rt_params p{};
    p.width = std::stoul(argv[4]);
    p.height = std::stoul(argv[5]);
    p.spp = std::stoul(argv[6]);
    p.max_depth = std::stoul(argv[7]);
    p.seed = std::stoull(argv[8]);
    p.row_offset = std::stoul(argv[9]);
    p.row_stride = std::stoul(argv[10]);
    p.num_rows = std::stoul(argv[11]);
    const uint32_t mode = std::stoul(argv[12]);
    const int threads = std::stoi(argv[13]);
    rt_camera cam{};
    CHECK(rt_camera_default(p.width, p.height, mode, &cam) == RT_OK);
    const uint32_t rows = p.num_rows ? p.num_rows : p.height;
    std::vector<float> out(static_cast<size_t>(rows) * p.width * 3);
    uint64_t seg = 0;
    CHECK(oracle_render_f32(s.data(), static_cast<uint32_t>(s.size()), m.data(), static_cast<uint32_t>(m.size()), &cam, &p, 0,
                            threads, out.data(), &seg) == RT_OK);
    CHECK(want.size() == out.size() * 4 && std::memcmp(want.data(), out.data(), want.size()) == 0);
    CHECK(seg >= static_cast<uint64_t>(rows) * p.width * p.spp || p.max_depth == 0);
    return g_fail ? 1 : 0;
}

int threads(const std::string &scene)
{
    std::vector<rt_sphere> s;
    std::vector<rt_material> m;
    CHECK(load_scene(scene, s, m));
    rt_camera cam{};
    CHECK(rt_camera_default(64, 36, 0, &cam) == RT_OK);
    rt_params p{64, 36, 4, 64, 1234, 0, 1, 0, 0};
    std::vector<float> a(64 * 36 * 3), b(a.size());
    uint64_t sa = 0, sb = 0;
    CHECK(oracle_render_f32(s.data(), static_cast<uint32_t>(s.size()), m.data(), static_cast<uint32_t>(m.size()), &cam, &p, 0, 1,
                            a.data(), &sa) == RT_OK);
    CHECK(oracle_render_f32(s.data(), static_cast<uint32_t>(s.size()), m.data(), static_cast<uint32_t>(m.size()), &cam, &p, 0, 4,
                            b.data(), &sb) == RT_OK);
    CHECK(std::memcmp(a.data(), b.data(), a.size() * 4) == 0 && sa == sb);
    // the library's shared host state from several threads: the exact-division cache, the
    // process-default options (RT_OPTIONS parsed once), thread-local error messages
    std::vector<std::thread> pool;
    std::vector<int> ok(8, 0);
    for (int t = 0; t < 8; ++t)
        pool.emplace_back([&, t] {
            bool good = rthost::exact_by_reciprocal(static_cast<float>(100 + t % 3));
            rt_options o;
            good = good && rt_get_default_options(&o) == RT_OK;
            good = good && rt_options_parse("render_streams=99", &o) == RT_ERR_INVALID && std::strlen(rt_last_error()) > 0;
            ok[t] = good ? 1 : 0;
        });
    for (auto &t : pool) t.join();
    for (int v : ok) CHECK(v == 1);
    return g_fail ? 1 : 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc >= 3 && std::string(argv[1]) == "host") {
        const std::string golden = argv[2];
        check_scene_generators(golden);
        check_cameras();
        check_builders(golden);
        check_derive(golden);
        check_tiles(golden);
        check_divisions();
        check_plane_layout();
        check_plans();
        check_options();
        check_ppm(golden);
        std::printf("host_check host: %s (%d failed checks)\n", g_fail ? "FAIL" : "ok", g_fail);
        return g_fail ? 1 : 0;
    }
    if (argc >= 2 && std::string(argv[1]) == "render") return render(argc, argv);
    if (argc >= 3 && std::string(argv[1]) == "threads") return threads(argv[2]);
    std::fprintf(stderr, "usage: host_check host <golden> | render ... | threads <scene.bin>\n");
    return 2;
}
