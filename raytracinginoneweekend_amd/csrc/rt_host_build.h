// rt_host_build.h — the host-only half of the library (rt_host_build.cpp): error reporting,
// options, the reference's camera and scene constructors, the scene blob and cluster builder,
// the walk-shortcut proofs, what a scene derives from its records (derive_scene), exact-division
// checks and the PPM writer. No HIP: this half is also
// built with -fsanitize=address,undefined / thread for the CPU sanitizer runs (tests/sanitize).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rt_api.h"
#include "rt_consts.h"

namespace rthost {

extern thread_local std::string g_error;
int fail(int code, const std::string &msg);

constexpr uint64_t kMaxSlotsBytes = 1ull << 31;  // slot workspace per pass (2 GiB)
// (the kernel forms a slot index sample * n_pixels + pixel in 32 bits)
static_assert(kMaxSlotsBytes / 12 < (1ull << 32), "slot index width");
// internal render streams for frames in flight (rt_options.render_streams, 2..kMaxBufs), and
// workspaces: rt_options.workspaces_per_stream (1..2) per stream, at most kMaxWs
constexpr uint32_t kMaxBufs = 8;
constexpr uint32_t kMaxWs = 2 * kMaxBufs + 1;  // + the lone passes' own workspace (sample pairs, rt_host.cpp)

rt_options library_defaults();
int check_options(const rt_options &o);
// the process default (rt_set_default_options / RT_OPTIONS)
int default_options(rt_options &out);

// ---- scene blob: always-tested list + spatial clusters -------------------
// what a blob's readers need beside its data (a device scene keeps this record per blob, rt_scene.h)
struct blob_meta {
    uint32_t n_geo = 0, n_always = 0, n_clusters = 0, clus_offset = 0, n_clusters_real = 0;
    uint32_t n_supers = 0, supers_offset = 0, shade_offset = 0;
    float clus_pad = 0.f;
    uint32_t units = 0;  // the data's 16-byte units, shading records included (derive_scene sets it)
};
struct blob_t : blob_meta {
    std::vector<float> data;  // 16-byte units
    std::vector<uint32_t> always;  // sphere indices tested on every segment (not clustered)
};
blob_t build_blob(const rt_sphere *s, uint32_t n, bool clustered, uint32_t cluster_max);
std::vector<uint32_t> shortcut_words(const rt_sphere *s, uint32_t n, const rt_material *m, const blob_t &b,
                                     bool nb_off);
// per sphere {cos_lo, cos_hi}, the trap window of an isolated glass ball (empty: {1, 0})
std::vector<float> trap_windows(const rt_sphere *s, uint32_t n, const rt_material *m);

// ---- tile classes of a pass ---------------------------------------------
// What the classifier needs of a culled scene: the always-tested spheres, the box of every
// non-empty cluster and the box over all of them (centre C, half-extent E), the kernel's pad.
struct scene_geom {
    std::vector<rt_sphere> always;
    std::vector<float> boxes;  // per non-empty cluster: C[3], E[3]
    float root[6] = {0.f, 0.f, 0.f, -1.f, -1.f, -1.f};
    bool has_root = false;
    float clus_pad = 0.f;
};
scene_geom scene_geometry(const rt_sphere *s, const blob_t &b);
// The 64-pixel blocks of a pass's pixel enumeration (tiles of 2^tile_lw x 64/2^tile_lw over
// tiled_rows, then row-major blocks of the remaining rows) in dealing order: `lead` blocks first
// (a primary ray of the tile can meet a cluster's padded box: the tiles whose paths can enter a
// glass ball on their first or second segment), then the others, then `sky` blocks, whose every
// primary ray is PROVEN to meet no sphere (interval arithmetic over the tile's rays, with
// margins far above every float error of the kernel's tests). perm[i] = the natural block of
// dealing block i. Empty perm: the pass keeps its natural order (pixels not in whole blocks).
struct tile_order {
    std::vector<uint32_t> perm;
    uint32_t n_lead = 0, n_sky = 0;
};
tile_order classify_tiles(const rt_camera &cam, uint32_t W, uint32_t H, uint32_t row_offset, uint32_t row_stride,
                          uint32_t num_rows, uint32_t tile_lw, const scene_geom &g, bool sky_only = false);

// ---- the ground class ---------------------------------------------------
// A pass's ground blocks are the tiled blocks of its order's middle class: classify_tile gives a
// tile class 1 only when its beam misses every cluster's padded box, the untiled blocks (class 1
// without a proof) are numbered after every tile, and the order is stable, so they are the
// positions [n_lead, n_lead + ground_blocks) of the order. A render takes them out of the main
// launch when the scene and the pass allow it:
//   the scene: a box over all clusters and 1 to 8 always-tested spheres, every one lambert;
//   the pass: max_depth >= 2, the culled LDS kernels, the root gate on, and a sky kernel
//   (dealt by tile classes, single samples, some sky tile; the caller checks that part).
bool ground_scene_ok(const rt_sphere *s, const rt_material *m, const blob_t &b, const scene_geom &g);
bool ground_pass_ok(const rt_options &o, const rt_params &p);
uint32_t ground_blocks(uint32_t n_blocks, uint32_t n_lead, uint32_t n_sky, uint32_t W, uint32_t num_rows, uint32_t tile_lw);

// ---- what a scene derives from its records (rt_scene_create_ex and rt_scene_update) --------
// The checks of the records, before any HIP call (who: the entry point's name).
int check_records(const char *who, const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials,
                  uint32_t n_materials);
// Everything derived from the records, on the host: the one derivation both entry points install.
struct SceneDerived {
    blob_t blobs[2];             // with the shading records, kinds, dielectric constants, shortcut words
    std::vector<float> trap;     // the windows, then the empty set
    scene_geom geom;             // the tile classes' geometry, and as classify_tiles_kernel reads it
    bool has_geom = false;
    bool ground_ok = false;      // a root box and 1 to 8 always-tested spheres, all lambert
    std::vector<float> geom_words;
    bool in_fast_range = true;
    std::vector<float> table;    // [n][4] {cx, cy, cz, r}
    std::vector<float> flat;     // [n][5] {kind bits, albedo, param}
};
void derive_scene(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials, const rt_options &opt,
                  SceneDerived &d);

uint32_t rows_of(const rt_params &p);  // the rows a call renders (num_rows = 0: to the frame's end)
rt::UDiv make_udiv(uint32_t d);
bool exact_by_reciprocal(float b);

// ---- the plane table of a synchronous host-buffer call (rt_host_sync.h SyncCall) ----------
// One plane of the call in the cached context's device arena: an input is uploaded from `host`
// before the work, an output copied back to `host` after it, a scratch plane lives on the
// device only. An absent plane takes no room and no copy; its `dev` stays null.
struct Plane {
    enum Kind : uint32_t { Absent, In, Out, Scratch } kind;
    void *host;          // In (only read) / Out: the caller's plane
    uint32_t px_bytes;   // bytes per pixel
    bool clear = false;  // zeroed on the device before the work
    size_t at = 0;       // plane_layout: its offset in the arena
    void *dev = nullptr;  // SyncCall::run: its address on the device
    size_t n_px = 0;     // its pixels when the call has planes of two sizes (an input or a scratch plane); 0: the call's
    template <class T> T *as() const { return static_cast<T *>(dev); }
    size_t pixels(size_t call_px) const { return n_px ? n_px : call_px; }
};
inline Plane plane_in(const void *host, uint32_t px_bytes)
{
    return {host ? Plane::In : Plane::Absent, const_cast<void *>(host), px_bytes};
}
inline Plane plane_out(void *host, uint32_t px_bytes) { return {host ? Plane::Out : Plane::Absent, host, px_bytes}; }
inline Plane plane_scratch(bool wanted, uint32_t px_bytes) { return {wanted ? Plane::Scratch : Plane::Absent, nullptr, px_bytes}; }
// Packs the planes that are there, n_px pixels each (or the plane's own count), in table order from offset 0 with every
// offset a multiple of 256 bytes (`at`); returns the bytes they take together.
size_t plane_layout(Plane *planes, size_t n_planes, size_t n_px);

} // namespace rthost
