/*
 * rt_api.h — C-ABI boundary of the MI355X-native path tracer (librt_mi355x.so).
 *
 * This header is the drop-in boundary for the reference's accelerated render path.
 * The reference (Alabuta/RaytracingInOneWeekend) binds its accelerated renderer as
 *
 *     extern void cuda_impl(std::uint32_t width, std::uint32_t height,
 *                           std::vector<math::u8vec3> &image_texels);      // src/main.cxx:18
 *
 * defined at src/CUDA/cuda_impl.cu:384-453 and called once at src/main.cxx:114. That
 * entry has C++ linkage, hardcodes scene/camera/spp/depth and throws on error. The
 * entry points below replace it with a C ABI: plain pointers and sizes, POD records,
 * an int status (0 = RT_OK), no exceptions across the boundary, caller-owned host
 * buffers. The literal `cuda_impl`-shaped C++ drop-in lives in rt_render_impl.hpp.
 *
 * Semantics follow the reference CPU render path (src/main.cxx:120-215 with
 * src/raytracer.hxx, src/camera.hxx, src/math.hxx); the CUDA variant's own semantics
 * (src/CUDA/cuda_impl.cu) are selected with RT_FLAG_CUDA_COMPAT or rt_render_cuda_impl.
 *
 * Threading: every call is synchronous unless its name ends in _device; calls on one
 * rt_scene come from one host thread. Device calls on one rt_scene may use different
 * streams: a call on a new stream is ordered after the previous call's work. Errors: a negative status; rt_last_error() returns a
 * thread-local message for the last failing call on this thread.
 */
#ifndef RT_API_H
#define RT_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_API_VERSION 2  /* 2: rt_options (resource bounds and A/B toggles), rt_scene_usage */

/* ---- status codes ---------------------------------------------------------------- */
enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID = -1,     /* bad argument (null pointer, zero size, bad index)       */
    RT_ERR_DEVICE = -2,      /* HIP runtime error (no device, launch/alloc failure)     */
    RT_ERR_CAPACITY = -3,    /* caller buffer too small                                 */
    RT_ERR_UNSUPPORTED = -4, /* feature not available in this build / on this host     */
    RT_ERR_COMM = -5,        /* RCCL failure in the multi-GPU path                      */
    RT_ERR_IO = -6           /* file could not be opened or written (rt_write_ppm)       */
};

/* ---- scene records ----------------------------------------------------------------
 * rt_sphere replaces primitives::sphere {math::vec3 center; float radius;
 * std::size_t material_index;} (src/primitives.hxx:6-17). A negative radius is legal
 * and flips the normal (hollow bubble, src/main.cxx:129; src/raytracer.hxx:71).      */
typedef struct rt_sphere {
    float center[3];
    float radius;
    uint32_t material;
} rt_sphere;

/* rt_material replaces material::types = std::variant<lambert, metal, dielectric>
 * (src/material.hxx:12-51). `param` is metal::roughness or dielectric::refraction_index
 * (unused for lambert).                                                               */
enum rt_material_kind { RT_LAMBERT = 0, RT_METAL = 1, RT_DIELECTRIC = 2 };
typedef struct rt_material {
    uint32_t kind;
    float albedo[3];
    float param;
} rt_material;

/* ---- camera -----------------------------------------------------------------------
 * Precomputed basis of raytracer::camera (src/camera.hxx:24-44); build it with
 * rt_camera_init() so the host arithmetic matches the reference constructor bit for bit.
 * mode RT_CAMERA_REFERENCE reproduces camera::ray() (src/camera.hxx:46-57) as shipped,
 * whose direction omits "- origin"; RT_CAMERA_CORRECTED subtracts the origin.        */
enum rt_camera_mode { RT_CAMERA_REFERENCE = 0, RT_CAMERA_CORRECTED = 1 };
typedef struct rt_camera {
    float origin[3];
    float lower_left_corner[3];
    float horizontal[3];
    float vertical[3];
    float lens_radius;
    uint32_t mode;
} rt_camera;

/* ---- render parameters ------------------------------------------------------------
 * width/height: FULL image size (u = x/width, v = y/height as src/main.cxx:192,195).
 * spp: samples per pixel (app::data::sampling_number, src/main.cxx:23).
 * max_depth: bounce limit (raytracer::data::bounces_number = 64, src/raytracer.hxx:20).
 * seed: RNG seed. Each (pixel, sample) owns two PCG32 streams keyed by
 *       key = (y*width + x)*spp + s — data stream seq 2*seed, camera stream seq 2*seed+1 —
 *       so any row partition renders the same bits. All 64 bits of the key
 *       count (width*height < 2^32, so a key reaches 2^32 * spp). Of the seed, the low 62 bits
 *       count: the streams' increments are ((2*seed) << 1) | 1 and ((2*seed + 1) << 1) | 1
 *       modulo 2^64, which drops the seed's top two bits, so seeds s and s + 2^62 (and s + 2^63)
 *       render the same bits. With RT_FLAG_CUDA_COMPAT only the low 32 bits of the seed count
 *       (the variant's engine state x + y*width + seed is 32 bits wide and wraps).
 * Rows rendered: y_i = row_offset + i*row_stride for i in [0, num_rows). num_rows = 0
 *       means "all rows of the stride pattern below height".
 * Output layout: row-major RGB f32, 3 floats per pixel. With RT_FLAG_FULL_FRAME the
 *       output is indexed by the global row y (buffer of height*width*3 floats);
 *       otherwise rows are packed in render order (num_rows*width*3 floats).          */
enum rt_flags {
    RT_FLAG_FULL_FRAME = 1u << 0, /* write rows at their global position             */
    RT_FLAG_FAST_MATH = 1u << 1,  /* FMA-contracted kernel, stated tolerance          */
    RT_FLAG_SCALAR_SCENE = 1u << 2, /* A/B: brute force, spheres via the scalar cache   */
    RT_FLAG_BRUTE_FORCE = 1u << 3,  /* test every sphere (no cluster culling); same bits */
    RT_FLAG_CUDA_COMPAT = 1u << 4,  /* semantics of the reference's CUDA variant instead of its
                                       CPU path: src/CUDA/cuda_impl.cu (see rt_render_cuda_impl) */
    RT_FLAG_WAVEFRONT = 1u << 5     /* A/B: the wavefront variant (one launch per segment, ray
                                       queues in HBM) instead of the persistent megakernel;
                                       same bits, cluster culling; rt_options.wave_queue_rays
                                       bounds a chunk (2^25 rays, 52 B each, two queues)       */
};
typedef struct rt_params {
    uint32_t width, height;
    uint32_t spp, max_depth;
    uint64_t seed;
    uint32_t row_offset, row_stride, num_rows;
    uint32_t flags;
} rt_params;

typedef struct rt_stats {
    uint64_t primaries;  /* pixel-samples traced (W*rows*spp)                          */
    uint64_t segments;   /* hit_world() calls = ray segments traced                    */
    uint64_t sphere_tests; /* ray-sphere tests executed (lane level)                   */
    uint64_t box_tests;  /* cluster AABB tests executed (lane level)                    */
    double kernel_ms;    /* render kernel time (HIP events)                            */
    double wall_ms;      /* whole call: upload + kernel + download                     */
} rt_stats;

/* ---- library ----------------------------------------------------------------------- */
int rt_version(void);
const char *rt_last_error(void);
int rt_device_count(int *count);

/* ---- options: resource bounds and same-bits variants of a scene ---------------------
 * rt_options_default() fills the library defaults; change fields, then pass the record to
 * rt_scene_create_ex / rt_multi_create_ex, or make it the process default
 * (rt_set_default_options) for scenes created without one: rt_scene_create, the synchronous
 * renders (rt_render_f32, rt_render_rgb8, rt_render_multi_*) and rt_multi_create.
 * The environment variable RT_OPTIONS ("key=value,key=value", keys as the field names, the
 * diag bits as ieee_roots=1 ...; rt_options_parse) is applied over the defaults once, at the
 * library's first use, so an unmodified caller (the reference's main() with the drop-in) can
 * be A/B-tested. Every value is checked: RT_ERR_INVALID names the field. No option changes
 * a rendered bit (every variant is the reference's arithmetic); they trade memory and speed. */
typedef struct rt_options {
    uint32_t size;                  /* sizeof(rt_options): the record's revision              */
    uint32_t render_streams;        /* frames in flight: internal render streams. 0 = auto
                                       (GPU_MAX_HW_QUEUES - 1, within 2..7), 1 = every kernel
                                       on the caller's stream, 2..8                           */
    uint32_t workspaces_per_stream; /* sample-slot workspaces per render stream, 1..2 (2)     */
    uint32_t deep_split;            /* paths past this many segments finish in a second, dense
                                       launch; 0 = no split, 1..1024 (8)      */
    uint64_t max_pass_bytes;        /* slot workspace of one pass (12 B per pixel and sample):
                                       12 B .. 2 GiB (2 GiB); frames above it run in passes    */
    uint64_t max_workspace_bytes;   /* cap on the scene's device workspaces (slots, deep-path
                                       queues, multi-pass sums, wavefront queues); 0 = none.
                                       Over it, workspaces per stream go to 1, then passes
                                       shrink (to 4 samples), then streams go; RT_ERR_CAPACITY
                                       if one 4-sample pass on the caller's stream does not fit */
    uint64_t deep_min_items;        /* a pass issued while no other render runs (a lone frame)
                                       is split only from this many samples (2^25); passes
                                       issued beside other renders are split at any size       */
    uint32_t cluster_size;          /* spheres per culling cluster, 4..64, a multiple of 4 (16);
                                       read when the scene is created                         */
    uint32_t transpose_max;         /* clusters requested by at most this many lanes run as
                                       (ray, member) pairs over the wave, 0..16 (16)           */
    uint32_t wave_queue_rays;       /* RT_FLAG_WAVEFRONT: rays per chunk, >= 64 (2^25)        */
    uint32_t diag;                  /* rt_diag bits (0)                                        */
    uint64_t ring_pass_bytes;       /* with frames in flight: slot workspace of a pass issued
                                       beside other renders, 0 or 12 B .. 2 GiB (384 MiB); the
                                       frame's samples are cut into equal passes of a multiple
                                       of 4 within it, if they hold 32 samples or more. A frame
                                       issued alone that fits max_pass_bytes runs in one pass in
                                       a workspace of its own. 0 = passes of max_pass_bytes     */
    uint32_t tile_classes;          /* where a pass's dealing order is computed for a camera the
                                       scene has not seen: 0 = on the host (0),
                                       1 = by kernels on a stream of the scene's own, without a
                                       device-wide synchronisation. Same order, same bits        */
    uint32_t sky_moments;           /* frames that carry per-pixel moments (rt_render_var_device,
                                       the progressive, adaptive and preview sessions; DESIGN.md
                                       §4.21): 0 = their proven-sky tiles are traced by the main
                                       launch (0), 1 = sky_moments_kernel renders them, sums and
                                       moments, and the main launch deals the other tiles alone.
                                       Same bits and segment count; the sphere- and box-test
                                       counters (d_segments[1], [2]) drop by the tests it saves   */
} rt_options;
enum rt_diag {
    RT_DIAG_IEEE_ROOTS = 1u << 0,      /* the IEEE sqrt/division sequences for every root     */
    RT_DIAG_NO_SHORTCUT = 1u << 1,     /* no walk shortcut for rays in glass balls            */
    RT_DIAG_NO_NEIGHBOURS = 1u << 2,   /* the shortcut for isolated balls only                */
    RT_DIAG_NO_ROOT_BOX = 1u << 3,     /* no level-3 box gate before the cluster walk         */
    RT_DIAG_SHADE_LDS = 1u << 4,       /* shading records forced into LDS ...                 */
    RT_DIAG_SHADE_GLOBAL = 1u << 5,    /* ... or into global memory (default: by occupancy)   */
    RT_DIAG_STATS = 1u << 6,           /* the instrumented kernel (rt_scene_debug_*)           */
    RT_DIAG_STATS_DEEP_ONLY = 1u << 7, /* with STATS: count the deep launch alone             */
    RT_DIAG_VERBOSE = 1u << 8,         /* print every launch's plan to stderr                 */
    RT_DIAG_STANDIN_TRANSPORT = 1u << 9, /* rt_multi with every rank on one device: the RCCL
                                          gather code path, RCCL replaced by stream-ordered
                                          device copies (tests of that path on one GPU)       */
    RT_DIAG_UNBOUNDED_NB = 1u << 10,    /* with STATS: the walk shortcut's neighbour slots formed
                                          without the lane's own bound (the pre-fd383c3 form),
                                          for the bounds check to report (rt_scene_debug_counters) */
    RT_DIAG_NO_PAIRS = 1u << 11,        /* one sample per item and slot, under a cap too        */
    RT_DIAG_PAIRS = 1u << 12,           /* sample pairs for passes in flight without a cap
                                          (otherwise taken only under max_workspace_bytes)    */
    RT_DIAG_IN_FLIGHT = 1u << 13,       /* every pass planned as if issued beside other renders
                                          (partial grid, ring pass, pairs if asked): tests of
                                          that plan that must not depend on timing             */
    RT_DIAG_NATURAL_ORDER = 1u << 14,   /* items dealt in the pixels' natural tile order (no
                                          tile classes, no sky path)           */
    RT_DIAG_NO_SKY = 1u << 15,          /* tile classes order the dealing, but the tiles proven
                                          to send every primary ray to the sky are dealt last by
                                          the main launch (traced) instead of the sky kernel   */
    RT_DIAG_LONE_UNSPLIT = 1u << 16,    /* a lone pass dealt by tile classes is not split (its
                                          trapped paths start in its first items)              */
    RT_DIAG_SKY_SERIAL = 1u << 17,      /* a lone pass's sky kernel after its main and deep
                                          launches on their stream (not beside them)           */
    /* (bit 18 is unassigned and rejected)                                                      */
    RT_DIAG_NO_TRAP_END = 1u << 19      /* every trap window empty: paths trapped in isolated
                                          glass balls are traced to max_depth (same bits)      */
};
int rt_options_default(rt_options *out);
/* Applies "key=value[,key=value...]" (fields above; diag bits as ieee_roots, no_shortcut,
 * no_neighbours, no_root_box, shade_lds, shade_global, stats, stats_deep_only, verbose,
 * standin_transport = 0/1; tile_classes and sky_moments are fields, 0/1) to *inout;
 * RT_ERR_INVALID on an unknown key or a bad value.                                       */
int rt_options_parse(const char *text, rt_options *inout);
/* The options of scenes created without explicit ones (NULL: the library defaults).      */
int rt_set_default_options(const rt_options *options);
int rt_get_default_options(rt_options *out);

/* ---- host-side scene / camera construction ----------------------------------------- */
/* raytracer::camera ctor, src/camera.hxx:24-44 (aperture -> lens_radius = aperture/2). */
int rt_camera_init(const float position[3], const float lookat[3], const float up[3],
                   float aspect, float vfov_degrees, float aperture, float focus_distance,
                   uint32_t mode, rt_camera *out);
/* The reference's default camera for a width x height image: src/main.cxx:179-183.     */
int rt_camera_default(uint32_t width, uint32_t height, uint32_t mode, rt_camera *out);
/* Simple scene, src/main.cxx:120-129: 5 spheres, 4 materials.                          */
int rt_scene_simple(rt_sphere *spheres, uint32_t sphere_cap, uint32_t *n_spheres,
                    rt_material *materials, uint32_t material_cap, uint32_t *n_materials);
/* The CUDA variant's hardcoded scene, src/CUDA/cuda_impl.cu:425-437: 5 spheres, 4 materials. */
int rt_scene_cuda(rt_sphere *spheres, uint32_t sphere_cap, uint32_t *n_spheres,
                  rt_material *materials, uint32_t material_cap, uint32_t *n_materials);
/* The CUDA variant's camera, src/CUDA/cuda_impl.cu:371-375 (origin 0, look -z, vFOV 88,
 * focus 1; its rays carry no lens offset, camera.hxx:48-50).                            */
int rt_camera_cuda(uint32_t width, uint32_t height, rt_camera *out);
/* Huge random scene: simple scene + the generator of src/main.cxx:131-177 driven by
 * std::mt19937{seed} (the reference seeds from std::random_device). Namespace typo
 * fixed; a "type 3" draw pushes no material (as shipped), so such a sphere aliases the
 * next pushed material and trailing ones are resolved by one default material
 * (material::types{} = lambert{albedo 1}). Pass null buffers to query the counts.     */
int rt_scene_huge(uint32_t seed, rt_sphere *spheres, uint32_t sphere_cap, uint32_t *n_spheres,
                  rt_material *materials, uint32_t material_cap, uint32_t *n_materials);

/* The dealing order of the pass that camera + params describe on this scene:
 * its 64-pixel blocks (8x8 tiles, then row-major blocks of leftover rows) as dealt, perm[i] =
 * the natural block of dealing position i; n_lead blocks first (a primary ray can meet a
 * cluster's box), n_sky blocks last (every primary ray proven to meet no sphere: those samples
 * skip the closest-hit test). n_blocks = 0: the pass keeps the natural order (its pixel count is
 * not a multiple of 64). cap = 0 queries the counts. Host-only (no device needed).            */
int rt_tile_order(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials,
                  uint32_t n_materials, const rt_camera *camera, const rt_params *params,
                  uint32_t *perm, uint32_t cap, uint32_t *n_blocks, uint32_t *n_lead, uint32_t *n_sky);

/* The ground blocks of that pass: the positions [n_lead, n_lead + n_ground) of
 * rt_tile_order's perm, tiles whose every primary ray is proven to miss every cluster's padded
 * box, which a render under the default options gives to the ground kernel in every pass that is
 * split (every pass issued beside other renders, and a pass issued alone of at
 * least rt_options.deep_min_items samples; an unsplit pass keeps them in its main launch, so a
 * small lone frame renders none through the kernel whatever this returns). 0 when the scene
 * (no box over the clusters, or an always-tested list that is not 1 to 8 lambert spheres) or the
 * pass (max_depth < 2, brute force / scalar / wavefront / compat flags, no sky tile, or the
 * default options' natural_order, no_sky, no_root_box, pairs) keeps them in the main launch.
 * Host-only.                                                                                  */
int rt_tile_ground(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials,
                   uint32_t n_materials, const rt_camera *camera, const rt_params *params,
                   uint32_t *n_ground);

/* The trap windows of a scene's spheres: out[2 i], out[2 i + 1] = sphere i's
 * {cos_lo, cos_hi}. A path that reflects totally inside sphere i with its cosine in the window
 * is proven to stay in that ball until max_depth (<= 64) and is ended there with colour 0; {1, 0}
 * = no window (not an isolated glass ball, or the margins leave none). Host-only.              */
int rt_trap_windows(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials,
                    uint32_t n_materials, float *out);

/* ---- synchronous host-buffer renders (the cuda_impl replacement) ------------------- */
/* These keep one device context per device between calls (the scene on the device, its
 * workspaces, the frame buffers), keyed by the scene's records and the process-default
 * options: a repeated call with the same scene renders without rebuilding anything, as the
 * reference's main() calls its entry once per frame (src/main.cxx:114). Another scene or
 * other default options rebuild it. Calls are serialised within the process.
 * rt_release_cached frees every such context (its device memory and streams).           */
int rt_release_cached(void);
/* Linear (pre-gamma) averaged RGB, f32. rgb_out: see rt_params output layout.          */
int rt_render_f32(const rt_sphere *spheres, uint32_t n_spheres,
                  const rt_material *materials, uint32_t n_materials,
                  const rt_camera *camera, const rt_params *params,
                  float *rgb_out, rt_stats *stats);
/* Gamma 1/2.2 + (uint8)(255*c) epilogue (src/main.cxx:39-45,77-85) fused on device.    */
int rt_render_rgb8(const rt_sphere *spheres, uint32_t n_spheres,
                   const rt_material *materials, uint32_t n_materials,
                   const rt_camera *camera, const rt_params *params,
                   uint8_t *rgb_out, rt_stats *stats);
/* Row-interleaved split over ngpu devices of this process (device i renders rows
 * y ≡ i mod ngpu), gathered to device 0 with RCCL over xGMI, then copied to rgb_out
 * (full frame, height*width*3 floats). ngpu <= 0 uses every visible device. One-shot:
 * builds and tears down an rt_multi context (below) around the frame.                 */
int rt_render_multi_f32(const rt_sphere *spheres, uint32_t n_spheres,
                        const rt_material *materials, uint32_t n_materials,
                        const rt_camera *camera, const rt_params *params, int ngpu,
                        float *rgb_out, rt_stats *stats);
/* The same with the gamma/u8 epilogue (src/main.cxx:39-45,77-85) run on every rank's tile
 * before the gather: 3 bytes per pixel cross xGMI instead of 12 (height*width*3 bytes).  */
int rt_render_multi_rgb8(const rt_sphere *spheres, uint32_t n_spheres,
                         const rt_material *materials, uint32_t n_materials,
                         const rt_camera *camera, const rt_params *params, int ngpu,
                         uint8_t *rgb_out, rt_stats *stats);

/* app::save_to_file (src/main.cxx:87-101): binary PPM "P6\n<width> <height>\n255\n"
 * followed by width*height RGB texels, row 0 first. RT_ERR_IO if the file cannot be
 * written (the reference throws "bad file").                                           */
int rt_write_ppm(const char *path, const uint8_t *rgb, uint32_t width, uint32_t height);

/* The literal replacement of the reference's accelerated entry point
 *     void cuda_impl(uint32_t width, uint32_t height, std::vector<u8vec3> &image_texels)
 * (src/main.cxx:18, defined src/CUDA/cuda_impl.cu:384-453): its scene and camera, 48 spp,
 * 32 bounces, one xorshift32 engine per pixel seeded with the pixel index, gamma 1/2.2 and
 * (uint8)(255 c). rgb_out: width*height*3 bytes, row 0 = top. Synchronous.
 * With RT_FLAG_CUDA_COMPAT in rt_params any scene/camera/spp/depth renders with those
 * semantics (seed is added to the pixel index; the camera's lens radius is not used).   */
int rt_render_cuda_impl(uint32_t width, uint32_t height, uint8_t *rgb_out);

/* ---- device-resident API (inputs resident in HBM, async on a caller stream) -------- */
typedef struct rt_scene rt_scene;
/* Uploads the scene to `device` (packed SoA).                   */
int rt_scene_create(const rt_sphere *spheres, uint32_t n_spheres,
                    const rt_material *materials, uint32_t n_materials, int device,
                    rt_scene **out);
/* The same with explicit options (NULL: the process default, rt_set_default_options).   */
int rt_scene_create_ex(const rt_sphere *spheres, uint32_t n_spheres,
                       const rt_material *materials, uint32_t n_materials, int device,
                       const rt_options *options, rt_scene **out);
int rt_scene_destroy(rt_scene *scene);
/* ---- moving spheres: new records into a live scene -------------------------------
 * Replaces the scene's records in place. n_spheres must equal the scene's count (ids are the link
 * between frames; another count is RT_ERR_INVALID); n_materials may differ (materials are flattened
 * per sphere). Every check rt_scene_create_ex makes on the records applies (material index, kind, null
 * pointers), all before any HIP call, the message naming the field.
 * The call is synchronous: it builds everything rt_scene_create_ex derives from the records on the
 * host (both blobs with the clustering, the boxes, the shading records, kinds, dielectric constants
 * and walk-shortcut words; the trap windows, under RT_DIAG_NO_TRAP_END too; the tile classes' geometry;
 * the fast-range flag; the counts and offsets), waits until the scene's device is idle, grows any device
 * buffer that is too small, uploads and swaps. The streams, events, workspaces, deep queues, permutation
 * buffers and debug buffers are kept. What was keyed by the old geometry is dropped: the cached dealing
 * orders (rt_scene_order_counts keeps counting), the deep-split record of cameras, and the occupancy
 * caches that depend on a blob's size. On any failure the scene is exactly as it was.
 * The contract: after rt_scene_update(sc, S, M) every call on sc behaves like the same call on a scene
 * freshly created from (S, M) with sc's options: the same status, the same bits in the beauty, the
 * variance, all five feature planes, the tile orders and counts, the same trap behaviour. A blob that no
 * longer fits LDS is reported by the calls that would report it for a fresh scene.
 * The scene keeps two device tables of n_spheres x 4 floats {cx, cy, cz, radius}, row i = sphere i of
 * the caller's array: the current records, and the records before the most recent update (both the
 * creation's records until then); an update swaps them and uploads the new one. They add 32 B per sphere
 * to rt_scene_usage.device_bytes. geometry_epoch goes up by 1 on an update in which the bits of any
 * centre or radius changed, appearance_epoch on one in which any sphere's flattened {kind, albedo, param}
 * changed. An update whose records equal the current ones bit for bit returns RT_OK at once: no wait,
 * the cached orders stay, both epochs stay.
 * Not covered: an rt_multi context (its scenes are its own), and the cached context of the synchronous
 * host-buffer renders, which rebuilds on a new scene as before.                                       */
int rt_scene_update(rt_scene *scene, const rt_sphere *spheres, uint32_t n_spheres,
                    const rt_material *materials, uint32_t n_materials);
typedef struct rt_scene_motion_t {
    uint32_t size, n_spheres;              /* sizeof(rt_scene_motion_t), filled by the call             */
    const float *centres, *prev_centres;   /* device, [n_spheres][4]; valid until the next update      */
    uint64_t geometry_epoch, appearance_epoch;
} rt_scene_motion_t;
int rt_scene_motion(rt_scene *scene, rt_scene_motion_t *out);
/* Enqueue one render for `stream` (a hipStream_t, or NULL for the null stream).
 * d_rgb: device buffer laid out as rt_params says. d_segments: optional device u64[3]
 * that accumulates {segments, sphere tests, cluster box tests} (zero it first). No
 * host sync (a call whose workspaces must grow, or be re-cut under max_workspace_bytes,
 * synchronises the device once, before enqueuing). The render kernels rotate over the
 * scene's internal render streams (rt_options.render_streams: by default the process's
 * hardware queues - 1, i.e. 3 at HIP's default GPU_MAX_HW_QUEUES=4 and at most 7) with
 * rt_options.workspaces_per_stream slot workspaces each, so consecutive frames overlap; they
 * read only the scene and the by-value arguments, and the writes to d_rgb / d_segments are
 * enqueued on `stream`, so results appear in stream order.
 * A camera (with its rows) the scene has not rendered among its last 8 first gets its dealing
 * order (rt_tile_order). With rt_options.tile_classes = 0 the call computes it on the host
 * (0.5 to 1.2 ms for a 1280x720 frame), allocates and uploads it synchronously and, to drop
 * the oldest of 8, waits for the device to go idle: a camera that moves every frame drains the
 * frames in flight. With tile_classes = 1 two small kernels on a stream of the scene's own
 * compute it and the call waits for that stream's event alone (one short event wait, 0.09 ms on
 * an idle device: the host needs the class counts to size the launches), with no allocation and
 * no device-wide wait once the scene's 8 permutation buffers exist. On a device that frames in
 * flight fill, those kernels themselves wait for room, about as long as the host path's drain
 * (DESIGN.md §4.13). Either way a repeated camera costs nothing, and the images are the same
 * bits.                                                                                       */
int rt_render_device(rt_scene *scene, const rt_camera *camera, const rt_params *params,
                     float *d_rgb, void *stream, uint64_t *d_segments);
/* The device twin of rt_tile_order: the dealing order of the pass camera +
 * params describe, computed by the kernels of rt_options.tile_classes = 1 (whatever the scene's
 * own setting) from this scene's geometry, i.e. with its cluster_size. The kernels run on
 * `stream` and write perm[0 .. n_blocks) to the device buffer d_perm (cap entries); the call
 * returns the counts after synchronising `stream`. cap = 0 queries the counts; 0 < cap < n_blocks
 * is RT_ERR_CAPACITY with the counts set and nothing written. A width that is no multiple of 8
 * gives the identity and zero counts, a pixel count that is no multiple of 64 n_blocks = 0, as
 * on the host. The classes equal rt_tile_order's exactly. Arguments are checked before any HIP
 * call.                                                                                         */
int rt_tile_order_device(rt_scene *scene, const rt_camera *camera, const rt_params *params,
                         uint32_t *d_perm, uint32_t cap, uint32_t *n_blocks, uint32_t *n_lead,
                         uint32_t *n_sky, void *stream);
/* How many dealing orders the scene has computed on the host and on the device since it was
 * created, and how many render / feature-buffer calls found theirs cached (each pointer may be
 * NULL). A pass that needs no classification (pixels not in whole 64-blocks, a width that is no
 * multiple of 8) counts as a host order under either setting.                                   */
int rt_scene_order_counts(rt_scene *scene, uint64_t *host_orders, uint64_t *device_orders,
                          uint64_t *hits);
/* The ground kernel's share of the scene's last frame that used it: the samples
 * of its ground tiles, and how many of them the kernel punted to the redo launch. Both 0 before
 * any such frame. Waits for the device. Each pointer may be NULL.                               */
int rt_scene_ground_counts(rt_scene *scene, uint64_t *ground_samples, uint64_t *redone_samples);
/* ---- the render with the variance of each pixel's mean luminance ----
 * d_rgb receives the bits rt_render_device writes for the same arguments; d_var receives one float
 * per pixel, laid out as the one-channel feature planes below (row * width + x; packed rows or
 * RT_FLAG_FULL_FRAME, with row_offset / row_stride / num_rows). With c_s the colour of the
 * beauty's sample s = 0..spp-1, every operation binary32 and rounded on its own (no contraction):
 *   L_s  = (0.2126f * c_s.r + 0.7152f * c_s.g) + 0.0722f * c_s.b
 *   d_s  = L_s - L_0                          (shifted data: d_0 = 0)
 *   m1   = (((0 + d_0) + d_1) + ...)          sequential, in sample order, across passes
 *   m2   = (((0 + d_0*d_0) + d_1*d_1) + ...)  likewise
 *   n    = float(spp);  mean = m1 / n;  ex2 = m2 / n            (IEEE divisions)
 *   var  = fmaxf(0.0f, ex2 - mean * mean) / float(spp - 1)
 * the unbiased sample variance of L divided by spp: the variance of the pixel's mean luminance. The
 * shift by L_0 keeps the subtraction from cancelling on nearly constant pixels (the sky).
 * spp < 2 is RT_ERR_INVALID. RT_FLAG_BRUTE_FORCE is honoured (same bits); RT_FLAG_FAST_MATH,
 * RT_FLAG_SCALAR_SCENE, RT_FLAG_WAVEFRONT and RT_FLAG_CUDA_COMPAT return RT_ERR_UNSUPPORTED. Every
 * argument is checked before any HIP call. The frame is planned with one sample per slot and its
 * proven-sky tiles traced by the main launch (as under RT_DIAG_NO_PAIRS | RT_DIAG_NO_SKY), whatever
 * the scene's other options say: the per-sample colours must reach the accumulation. With
 * rt_options.sky_moments = 1 the proven-sky tiles go to the sky kernel's moments form instead, which
 * folds each colour into the pixel's sum and moments itself (same bits; rt_scene_usage.sky_tiles
 * reports them). Of d_segments' three words the first, the segments, is the same
 * with the option on or off; the sphere-test and box-test words come out smaller with it on, because
 * the kernel tests its samples, proven to miss, against nothing, exactly as rt_render_device's counters
 * relate to a render under RT_DIAG_NO_SKY. A frame of several
 * passes carries {L_0, m1, m2} per pixel in a workspace accounted like the multi-pass sums
 * (rt_scene_usage, max_workspace_bytes), allocated by the first such frame. d_segments, stream
 * order and frames in flight are rt_render_device's.                                           */
int rt_render_var_device(rt_scene *scene, const rt_camera *camera, const rt_params *params,
                         float *d_rgb, float *d_var, void *stream, uint64_t *d_segments);
/* Host pointers, synchronous, through the cached per-device context of rt_render_f32. With
 * RT_FLAG_FULL_FRAME only the rendered rows of rgb_out and var_out are written.                */
int rt_render_var(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials, uint32_t n_materials,
                  const rt_camera *camera, const rt_params *params,
                  float *rgb_out, float *var_out, rt_stats *stats);
/* ---- first-hit feature buffers --------------------------------------
 * The guide buffers a denoiser or compositor takes, for the pass rt_params describes. Sample s
 * of a pixel is the beauty render's sample s (same key with the frame's spp, same streams, same
 * camera::ray; max_depth is not used), so samples 0..samples-1 are the beauty's first ones.
 * Its first hit is hit_world (raytracer.hxx:94-118). Per sample:
 *   albedo  the hit sphere's material albedo, whatever its kind; on a miss the sky's colour
 *           background(.5 unit_direction(d).y + 1) (main.cxx:71 with an attenuation of 1)
 *   normal  (p - c) / r (raytracer.hxx:71; a negative radius flips it); (0, 0, 0) on a miss
 *   depth   hit.time: t in units of the un-normalised ray direction d; 0 on a miss
 *   alpha   1 on a hit, 0 on a miss
 * A pixel's value of each float plane is the samples' sum in the blocked order of main.cxx:205
 * divided by float(samples). sphere_id is the index (in the caller's array) of the sphere sample
 * 0 hits, or 0xffffffff. Rows and layout follow rt_params as for the beauty (row_offset,
 * row_stride, num_rows; packed or RT_FLAG_FULL_FRAME); one-channel planes are indexed
 * row * width + x. Only the planes given are written. RT_FLAG_BRUTE_FORCE is honoured (same
 * bits); RT_FLAG_FAST_MATH, RT_FLAG_SCALAR_SCENE, RT_FLAG_WAVEFRONT and RT_FLAG_CUDA_COMPAT
 * return RT_ERR_UNSUPPORTED, as does a scene whose geometry does not fit LDS.              */
typedef struct rt_aov_buffers {
    uint32_t size;        /* sizeof(rt_aov_buffers): the record's revision              */
    uint32_t samples;     /* samples 0..samples-1 of every pixel; 0 = params->spp       */
    float *albedo;        /* rows x width x 3, or NULL: plane not wanted                */
    float *normal;        /* rows x width x 3, or NULL                                  */
    float *depth;         /* rows x width, or NULL                                      */
    float *alpha;         /* rows x width, or NULL                                      */
    uint32_t *sphere_id;  /* rows x width, or NULL                                      */
} rt_aov_buffers;
/* Device pointers; one kernel enqueued on `stream` (a hipStream_t, or NULL), results in stream
 * order, no host synchronisation (the first call with a camera and rows computes the pass's
 * dealing order on the host and uploads it). Ordered like any other call on the scene.      */
int rt_render_aov_device(rt_scene *scene, const rt_camera *camera, const rt_params *params,
                         const rt_aov_buffers *aov, void *stream);
/* Host pointers, synchronous, through the cached per-device context of rt_render_f32. With
 * RT_FLAG_FULL_FRAME only the rendered rows of the caller's planes are written. stats
 * (optional): primaries = segments = width * rows * samples, kernel_ms, wall_ms; the test
 * counters are 0.                                                                            */
int rt_render_aov(const rt_sphere *spheres, uint32_t n_spheres, const rt_material *materials,
                  uint32_t n_materials, const rt_camera *camera, const rt_params *params,
                  const rt_aov_buffers *aov, rt_stats *stats);

/* ---- edge-avoiding à-trous denoiser over the feature buffers ----------
 * The 5x5 B3-spline à-trous wavelet filter of Dammertz et al. 2010, guided by the planes of
 * rt_render_aov, with a compact polynomial edge-stopping function in place of the Gaussian so
 * that the result is reproducible bit for bit: all arithmetic is binary32, every operation
 * rounded on its own (add, multiply, max, one division per pixel and channel; no exp or pow).
 *
 * Planes are packed row-major, width x height, pitch = width: beauty[h][w][3] (required),
 * optional guides albedo[h][w][3], normal[h][w][3], depth[h][w] exactly as rt_render_aov writes
 * them, output out[h][w][3].
 *
 * Edge function: edge(d2, r) = m * m with m = fmaxf(0.0f, 1.0f - d2 * r), r = 1.0f / (sigma *
 * sigma) (one float product, one IEEE division, on the host). The colour term of level l uses
 * sigma = sigma_color * 2^-l (exact).
 *
 * One level l, step s = 1 << l, input image C, output D. For pixel p = (x, y): sumw = 0,
 * sum[3] = 0; the taps j = -2..2 (outer loop), i = -2..2 (inner loop), q = (x + i s, y + j s);
 * a tap outside the image is skipped (nothing is added). w = h[|i|] * h[|j|] with h = {0.375f,
 * 0.25f, 0.0625f}, then the terms that are on are multiplied into w in this order:
 *   colour  d = C(q) - C(p) per channel, d2 = (d.r d.r + d.g d.g) + d.b d.b, w = w * edge(d2, r_c)
 *   normal  the same d2 over the normal plane, with r_n
 *   depth   dz = depth(q) - depth(p), d2 = dz dz, with r_z
 *   albedo  the same d2 over the albedo plane, with r_a
 * then sumw = sumw + w and sum[c] = sum[c] + w * C(q)[c] (a product, then a sum), and at the end
 * D(p)[c] = sum[c] / sumw (IEEE division; sumw >= 9/64, the centre tap has d2 = 0). A term is on
 * when its plane is given and its sigma is not 0 (colour: sigma_color not 0). The guides are
 * never filtered: every level reads the caller's planes. Sky pixels have normal 0 and depth 0 on
 * both sides, so d2 = 0 between them.
 *
 * Levels: C_0 = beauty, C_{l+1} = D_l; the last level writes `out`, the levels before it
 * alternate between `scratch` and `out` so that this holds. beauty and the guides are never
 * written.
 *
 * RT_DENOISE_DEMODULATE (needs albedo): A'(q)[c] = fmaxf(albedo(q)[c], 0.0078125f), C_0(q)[c] =
 * beauty(q)[c] / A'(q)[c], and the last level stores (sum[c] / sumw) * A'(p)[c]. On a pixel whose
 * samples all miss the albedo is the beauty pixel's own bits, so the sky demodulates to a constant.
 *
 * Every argument is checked before any HIP call; RT_ERR_INVALID names the field: a size
 * mismatch, zero width or height (or one above 65536), levels outside 1..6, a negative or
 * non-finite sigma, a zero sigma_normal or sigma_depth for a plane that is given, a sigma_color so
 * small that 1 / sigma^2 is not finite at the last level, unknown flags, DEMODULATE without
 * albedo, a null beauty or out, scratch null with levels > 1 (device call), out or scratch equal
 * to an input or to each other. NaN or infinite pixel values give unspecified output.          */
typedef struct rt_denoise_params {
    uint32_t size;            /* sizeof(rt_denoise_params): the record's revision                */
    uint32_t width, height;
    uint32_t levels;          /* 1..6; level l taps at spacing 1 << l                            */
    float sigma_color;        /* > 0; 0 = colour term off. Level l uses sigma_color * 2^-l       */
    float sigma_normal;       /* used only with a normal plane; > 0                              */
    float sigma_depth;        /* used only with a depth plane; > 0                               */
    float sigma_albedo;       /* used only with an albedo plane; > 0; 0 = term off (the albedo
                                 may still serve RT_DENOISE_DEMODULATE)                          */
    uint32_t flags;           /* rt_denoise_flags                                                */
} rt_denoise_params;
enum rt_denoise_flags {
    RT_DENOISE_DEMODULATE = 1u << 0,  /* filter beauty / albedo', multiply back at the end       */
    RT_DENOISE_DIRECT = 1u << 1       /* A/B: every level by the direct-load kernel; same bits   */
};
typedef struct rt_denoise_buffers {
    uint32_t size;            /* sizeof(rt_denoise_buffers)                                      */
    const float *beauty, *albedo, *normal, *depth;
    float *out;
    float *scratch;           /* w*h*3 floats; may be NULL when levels == 1                      */
} rt_denoise_buffers;
/* The defaults (DESIGN.md §4.9 records the sweep that chose them) for a width x height image.   */
int rt_denoise_params_default(uint32_t width, uint32_t height, rt_denoise_params *out);
/* Device pointers on the current device; one launch per level on `stream` (a hipStream_t, or
 * NULL), no host synchronisation, no allocation. Small steps take the tiled kernel (taps from
 * LDS), the others the direct one; RT_DENOISE_DIRECT forces the direct one everywhere.          */
int rt_denoise_device(const rt_denoise_params *params, const rt_denoise_buffers *buffers,
                      void *stream);
/* Measurement (the A/B behind that choice): level `level` (< params->levels) of that run alone,
 * reading buffers->beauty as the level's input C_level and writing buffers->out; scratch is not
 * used. By the tiled kernel wherever its LDS image fits (steps 1, 2 and 4), whatever the library
 * would choose for that level; by the direct one with RT_DENOISE_DIRECT. Same bits.           */
int rt_denoise_level_device(const rt_denoise_params *params, const rt_denoise_buffers *buffers,
                            uint32_t level, void *stream);
/* Host pointers, synchronous; scratch is ignored, the device buffers are the library's (kept in
 * the cached per-device context rt_release_cached frees). stats (optional): kernel_ms, wall_ms;
 * the counters are 0.                                                                           */
int rt_denoise(const rt_denoise_params *params, const rt_denoise_buffers *buffers,
               rt_stats *stats);

/* ---- the variance-guided à-trous filter --------------------------------
 * rt_denoise_device with the colour term steered per pixel by the variance rt_render_var writes
 * (SVGF, Schied et al. 2017, §4.2-4.4). Everything above holds except: V_0 = variance; at level l
 * (step s = 1 << l, colour input C_l, variance input V_l), for pixel p = (x, y):
 *   prefilter  g = 0; for j = -1..1 (outer), i = -1..1 (inner): g = g + k * V_l(q), q = (clamp(x + i,
 *              0, w - 1), clamp(y + j, 0, h - 1)) (spacing 1, not s), k = 0.25f at the centre, 0.125f
 *              when exactly one of i, j is 0, 0.0625f at the corners
 *   colour     r_c(p) = 1.0f / (sc2 * g + var_floor), sc2 = sigma_color * sigma_color formed once on
 *              the host: one IEEE division per pixel and level and no 2^-l factor (V itself
 *              shrinks); the term is edge(d2, r_c(p)) with the RGB d2 above; sigma_color = 0: off
 *   variance   in the same tap loop, from sumv = 0: sumv = sumv + (w * w) * V_l(q) with the tap's
 *              final w; V_{l+1}(p) = sumv / (sumw * sumw)
 * The normal, depth and albedo terms, the tap order, the skipped taps and sumw / sum[c] are
 * unchanged. The levels' V alternate between the two halves of var_scratch; variance_out, if
 * given, receives V_levels. RT_DENOISE_DEMODULATE is RT_ERR_UNSUPPORTED (the variance would have to
 * be demodulated too); RT_DENOISE_DIRECT is accepted and means nothing new (every level is a
 * direct-load launch). RT_ERR_INVALID names the field: every check of rt_denoise_device, a wrong
 * size, a null variance, a null var_scratch (device call), a var_floor that is not positive and
 * finite, variance_out or var_scratch equal to any other plane.                                 */
typedef struct rt_denoise_var_buffers {
    uint32_t size;          /* sizeof(rt_denoise_var_buffers)                                   */
    float var_floor;        /* > 0, finite                                                       */
    const float *variance;  /* [h][w], as rt_render_var writes it; never written                 */
    float *variance_out;    /* optional [h][w]: V after the last level                           */
    float *var_scratch;     /* 2*w*h floats (device call; ignored by the host call)              */
} rt_denoise_var_buffers;
/* The defaults (DESIGN.md §4.10 records the sweep that chose them); either record may be NULL. */
int rt_denoise_var_params_default(uint32_t width, uint32_t height, rt_denoise_params *params,
                                  rt_denoise_var_buffers *var);
/* Device pointers; one launch per level on `stream`, no host synchronisation, no allocation.    */
int rt_denoise_var_device(const rt_denoise_params *params, const rt_denoise_buffers *buffers,
                          const rt_denoise_var_buffers *var, void *stream);
/* Host pointers, synchronous, device planes in the cached per-device context (as rt_denoise).   */
int rt_denoise_var(const rt_denoise_params *params, const rt_denoise_buffers *buffers,
                   const rt_denoise_var_buffers *var, rt_stats *stats);

/* ---- temporal accumulation: the last frame's history reprojected ----------
 * The stage between rt_render_var / rt_render_aov and rt_denoise_var (SVGF, Schied et al. 2017,
 * §4.1): every pixel of the current frame reconstructs its first hit, projects it into the previous
 * camera, resamples the previous frame's accumulated colour, variance and history length under
 * consistency tests, and blends. The scene is static, so motion is camera motion and comes from the
 * two rt_camera records. All arithmetic is binary32, every operation rounded on its own, in the order
 * written; divisions are IEEE divisions.
 *
 * Planes are packed row-major, width x height, exactly as rt_render_var and rt_render_aov write them
 * (the guides of the frame's samples). Current frame, all required: beauty[h][w][3], variance[h][w],
 * normal[h][w][3], depth[h][w], alpha[h][w], sphere_id[h][w]. Previous frame, all given or all NULL
 * (NULL: no history exists yet): prev_color[h][w][3], prev_variance[h][w], prev_history[h][w] (float),
 * prev_normal, prev_depth, prev_sphere_id. Outputs, all required: out_color, out_variance,
 * out_history. The caller ping-pongs; what it feeds back as prev_color is its choice: out_color, or,
 * as SVGF does, the first filter level's output.
 *
 * Projection record (rt_reproject_basis, on the host). With h', v', llc', o' the previous camera's
 * horizontal, vertical, lower_left_corner and origin:
 *   a'          = llc' (RT_CAMERA_REFERENCE) or llc' - o' componentwise (RT_CAMERA_CORRECTED)
 *   cross(x, y) = (x.y y.z - x.z y.y, x.z y.x - x.x y.z, x.x y.y - x.y y.x), each product rounded
 *   dot(x, y)   = (x.x y.x + x.y y.y) + x.z y.z
 *   D = dot(h', cross(v', a'));  A = cross(v', a') / D, B = cross(a', h') / D, G = cross(h', v') / D
 *   out = {A, B, G, o'}
 * D = 0 or a non-finite entry of out is RT_ERR_INVALID (prev_camera). For q = P - o' the Cramer
 * solution of [h' v' a'] (al, be, ga) = q is al = dot(A, q), be = dot(B, q), ga = dot(G, q): ga is
 * P's ray parameter in the previous camera (what its depth plane stores), and P projects to
 * u' = al / ga, 1 - v' = be / ga. In REFERENCE mode too: that mode's rays have the image-plane point
 * itself as their direction.
 *
 * Per pixel p = (x, y), with a formed from the current camera as a' above, o, hor, ver its origin,
 * horizontal and vertical:
 *   1 class   alpha(p) == 1.0f: surface; alpha(p) == 0.0f: sky; anything else: edge, no history
 *   2 ray     u = ((float)x + 0.5f) / (float)w;  m = 1.0f - ((float)y + 0.5f) / (float)h
 *             d = (a + hor * u) + ver * m, componentwise (the pinhole ray through the pixel centre)
 *   3 q       surface: q = (o + depth(p) * d) - o';  sky: q = d (the point at infinity: the sky is
 *             stable under rotation)
 *   4 project al, be, ga as above; no history unless ga > 0.0f
 *             px = (al / ga) * (float)w - 0.5f;  py = (1.0f - be / ga) * (float)h - 0.5f
 *             no history unless px > -1.0f && px < (float)w && py > -1.0f && py < (float)h (false
 *             for NaN)
 *   5 taps    fx = floorf(px), tx = px - fx, ix = (int)fx; fy, ty, iy likewise. The taps
 *             t = (ix + i, iy + j), j = 0, 1 (outer loop), i = 0, 1 (inner loop), with
 *             wgt = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty). A tap is skipped (nothing is added)
 *             when it lies outside the image, or prev_sphere_id(t) != sphere_id(p), or
 *             d2 > normal_tol with dn = prev_normal(t) - normal(p) per component and
 *             d2 = (dn.x dn.x + dn.y dn.y) + dn.z dn.z, or, for a surface pixel,
 *             fabsf(prev_depth(t) - ga) > depth_tol * ga. (Sky pixels have id 0xffffffff, normal 0
 *             and depth 0 on both sides and take no depth test.) From sumw = sum[3] = sumv = sumn = 0:
 *             sumw = sumw + wgt;  sum[c] = sum[c] + wgt * prev_color(t)[c]
 *             sumv = sumv + (wgt * wgt) * prev_variance(t);  sumn = sumn + wgt * prev_history(t)
 *   6 blend   history exists iff sumw >= 0.01f. Then C_h[c] = sum[c] / sumw,
 *             V_h = sumv / (sumw * sumw) (the variance of a weighted mean, as §4.10's levels),
 *             N_h = sumn / sumw;  N = fminf(N_h + 1.0f, max_history);  k = fmaxf(1.0f / N, alpha_min)
 *             out_color(p)[c] = k * beauty(p)[c] + (1.0f - k) * C_h[c]
 *             out_variance(p) = (k * k) * variance(p) + ((1.0f - k) * (1.0f - k)) * V_h (the frames
 *             taken as independent estimates);  out_history(p) = N
 *   7 no history (any reason above, or prev NULL): out_color(p) = beauty(p), out_variance(p) =
 *             variance(p), copies of the bits, and out_history(p) = 1.0f
 * Ten divisions per pixel with history: two for the pixel centre, two for the projection, five for
 * the resample, one for k. SVGF's 3x3 search when all four taps fail and its spatial variance
 * estimate for short histories are left out. NaN or infinite plane values give
 * unspecified output values; no tap is read outside the image whatever the values are.
 *
 * Every argument is checked before any HIP call; RT_ERR_INVALID names the field: a wrong size, zero
 * width or height (or one above 65536), alpha_min outside (0, 1], max_history < 1, a negative
 * normal_tol or depth_tol, a non-finite parameter, nonzero flags, a null camera, a null required
 * plane, prev partly given, an output plane equal to an input plane or to another output plane, and,
 * when prev is given, a null or degenerate prev_camera (ignored otherwise).                        */
typedef struct rt_temporal_params {
    uint32_t size;            /* sizeof(rt_temporal_params): the record's revision               */
    uint32_t width, height;
    float alpha_min;          /* 0 < alpha_min <= 1: the least weight of the current frame        */
    float max_history;        /* >= 1: the cap of the history length                              */
    float normal_tol;         /* >= 0: the largest squared normal distance of an accepted tap     */
    float depth_tol;          /* >= 0: the largest relative depth difference of an accepted tap   */
    uint32_t flags;           /* none defined: must be 0                                          */
} rt_temporal_params;
typedef struct rt_temporal_buffers {
    uint32_t size;            /* sizeof(rt_temporal_buffers)                                      */
    const float *beauty, *variance, *normal, *depth, *alpha;
    const uint32_t *sphere_id;
    const float *prev_color, *prev_variance, *prev_history, *prev_normal, *prev_depth;
    const uint32_t *prev_sphere_id;
    float *out_color, *out_variance, *out_history;
} rt_temporal_buffers;
/* The defaults (DESIGN.md §4.11 records the sweep that chose them) for a width x height image.   */
int rt_temporal_params_default(uint32_t width, uint32_t height, rt_temporal_params *out);
/* The projection record {A, B, G, o'} of a previous camera, as stated above. Host-only.          */
int rt_reproject_basis(const rt_camera *prev, float out[12]);
/* Device pointers on the current device; one launch on `stream` (a hipStream_t, or NULL), no host
 * synchronisation, no allocation.                                                                 */
int rt_temporal_device(const rt_temporal_params *params, const rt_camera *camera, const rt_camera *prev_camera,
                       const rt_temporal_buffers *buffers, void *stream);
/* Host pointers, synchronous; the device planes are the library's (kept in the cached per-device
 * context rt_release_cached frees). stats (optional): kernel_ms, wall_ms; the counters are 0.     */
int rt_temporal(const rt_temporal_params *params, const rt_camera *camera, const rt_camera *prev_camera,
                const rt_temporal_buffers *buffers, rt_stats *stats);

/* ---- the temporal stage with object motion -----------------------------------
 * rt_temporal_device for spheres that moved between the two frames. Spheres are rigid and uniformly
 * coloured, so a sphere's motion is its centre's motion, and sphere_id names the sphere under each
 * pixel: the stage takes two tables of n_spheres x 4 floats {cx, cy, cz, radius}, row i = sphere i of
 * the caller's array, now (centres) and at the previous frame (prev_centres), and no motion-vector
 * plane. Everything in rt_temporal_device's contract holds except step 3 for a surface pixel. With
 * id = sphere_id(p):
 *   id >= n_spheres: no history; neither table is read at that index
 *   C = centres[id], C' = prev_centres[id]; if the bits of C.r and C'.r differ (compared as uint32): no
 *   history (a resized sphere restarts)
 *   m = C.xyz - C'.xyz, componentwise
 *   q = ((o + depth(p) * d) - m) - o'
 * every operation binary32, rounded on its own, in the order written. Sky and edge pixels, the
 * projection, the four taps and their tests, the blend and the no-history copy are unchanged: the depth
 * test compares ga with prev_depth (the previous frame saw the sphere at C', which is what q describes),
 * and a translation keeps the normal and the id.
 *   Equal tables give the static stage's bits: if the two tables hold the same bits, m = +0 and
 *   x - (+0) = x for every x, so the output equals rt_temporal_device's bit for bit. The two pointers may
 *   be the same pointer.
 *   Scope of the motion: it is that of the first hit only. Reflections and shadows of a moving sphere on
 *   other spheres lag; alpha_min bounds that lag, as in any SVGF loop.
 * Every argument is checked before any HIP call; RT_ERR_INVALID names the field: every check
 * rt_temporal_device makes, then a null record or a wrong size, n_spheres > 0 with a null table, a table
 * that is not 16-byte aligned (a row is one 16-byte load), a table that is also an output plane. With
 * the prev_ planes NULL the record is still checked and then unused. NaN or infinite table entries give
 * unspecified output values; no read outside a plane or a table happens whatever the values are.       */
typedef struct rt_temporal_motion_t {
    uint32_t size, n_spheres;              /* sizeof(rt_temporal_motion_t); rows of either table        */
    const float *centres, *prev_centres;   /* [n_spheres][4] {cx, cy, cz, r}: now, and at the previous frame */
} rt_temporal_motion_t;
/* Device pointers (the tables too); one launch on `stream`, no host synchronisation, no allocation. */
int rt_temporal_motion_device(const rt_temporal_params *params, const rt_camera *camera, const rt_camera *prev_camera,
                              const rt_temporal_buffers *buffers, const rt_temporal_motion_t *motion, void *stream);
/* Host pointers, synchronous, through the cached per-device context as rt_temporal (the tables are two
 * more staged inputs, of any alignment).                                                              */
int rt_temporal_motion(const rt_temporal_params *params, const rt_camera *camera, const rt_camera *prev_camera,
                       const rt_temporal_buffers *buffers, const rt_temporal_motion_t *motion, rt_stats *stats);

/* ---- the temporal stage with the history clamped to the frame's own colours ----
 * rt_temporal_device (motion NULL: a static scene) or rt_temporal_motion_device (motion given) with
 * history rectification ("variance clipping", Salvi 2016): the resampled history colour is pulled into
 * the box mean +- gamma standard deviations of the current frame's colours in a (2 radius + 1)^2 window
 * around the pixel, taken over the taps on the pixel's own sphere. Everything in the underlying stage's
 * contract holds; one step is new, between the resample (step 5) and the blend (step 6), and it applies
 * only to a pixel whose history exists (sumw >= 0.01f). All arithmetic is binary32, every operation
 * rounded on its own, in the order written; sqrtf is the correctly rounded square root.
 *   5b window With b = beauty(p) and id = sphere_id(p), from n = 0, m1[3] = 0, m2[3] = 0: the taps
 *             q = (x + i, y + j), j = -radius..radius (outer loop), i = -radius..radius (inner loop). A
 *             tap is skipped (nothing is added) when it lies outside the image or sphere_id(q) != id.
 *             Otherwise n = n + 1.0f and per channel d = beauty(q)[c] - b[c];  m1[c] = m1[c] + d;
 *             m2[c] = m2[c] + d * d. (The data are shifted by the centre, as §4.10's L_0, so that a flat
 *             region does not cancel; the centre tap always counts, so n >= 1.)
 *      box    per channel: mean = m1[c] / n;  ex2 = m2[c] / n;  s2 = fmaxf(0.0f, ex2 - mean * mean)
 *             half = gamma * sqrtf(s2);  mu = b[c] + mean;  lo = mu - half;  hi = mu + half
 *      clamp  C_h[c] = fminf(fmaxf(C_h[c], lo), hi), with C_h[c] = sum[c] / sumw of step 6
 * The blend of step 6 uses this C_h. V_h, N_h, k and the outputs' layout are unchanged: a clamped
 * history keeps its length and its variance (left out). The window reads beauty and
 * sphere_id of the current frame only; no texel is read outside the image.
 *
 * Every argument is checked before any HIP call; RT_ERR_INVALID names the field: every check of the
 * underlying stage (rt_temporal_motion_device's when motion is not NULL), then a null clip record or a
 * wrong size, a radius outside 1..3, a negative or non-finite gamma, nonzero flags. With the prev_
 * planes NULL the record is still checked and then unused: the call is rt_temporal_device's copy.     */
typedef struct rt_temporal_clip_t {
    uint32_t size;    /* sizeof(rt_temporal_clip_t)                                        */
    uint32_t radius;  /* 1..3: the window is (2 radius + 1)^2 pixels of the current frame   */
    float gamma;      /* >= 0, finite: half-width of the box in standard deviations         */
    uint32_t flags;   /* none defined: must be 0                                            */
} rt_temporal_clip_t;
/* The defaults (DESIGN.md §4.17 records the sweep that chose them).                                  */
int rt_temporal_clip_default(rt_temporal_clip_t *out);
/* Device pointers (the tables of `motion` too); one launch on `stream`, no host synchronisation, no
 * allocation. motion NULL: a static scene.                                                           */
int rt_temporal_clip_device(const rt_temporal_params *params, const rt_camera *camera, const rt_camera *prev_camera,
                            const rt_temporal_buffers *buffers, const rt_temporal_motion_t *motion,
                            const rt_temporal_clip_t *clip, void *stream);
/* Host pointers, synchronous, through the cached per-device context as rt_temporal and
 * rt_temporal_motion: the window reads planes those calls already stage.                             */
int rt_temporal_clip(const rt_temporal_params *params, const rt_camera *camera, const rt_camera *prev_camera,
                     const rt_temporal_buffers *buffers, const rt_temporal_motion_t *motion,
                     const rt_temporal_clip_t *clip, rt_stats *stats);

/* ---- guided upsampling of a low-resolution frame ---------------------------------
 * The stage that brings a filtered image of lo_width x lo_height up to width x height: a joint-
 * bilateral upsample (Kopf et al. 2007) whose four bilinear taps are tested against first-hit guides
 * of the output size with the temporal stage's consistency tests. Both sets of guides are what
 * rt_render_aov writes for the same camera at the two sizes. Depth is t in units of the un-normalised
 * ray direction, and that direction is a function of (u, v) alone, so depths of the two sizes compare
 * directly: the stage takes no camera. All arithmetic is binary32, every operation rounded on its
 * own, in the order written; divisions are IEEE divisions.
 *
 * Planes are packed row-major, pitch = their width. Low resolution, lw x lh: lo_color[lh][lw][3]
 * (required), lo_variance[lh][lw] (given iff out_variance is), lo_normal[lh][lw][3], lo_depth[lh][lw],
 * lo_sphere_id[lh][lw] (required). Output size, w x h, all required: normal[h][w][3], depth[h][w],
 * alpha[h][w], sphere_id[h][w]. Outputs: out_color[h][w][3] (required), out_variance[h][w] (optional).
 *
 * Per output pixel p = (x, y):
 *   1 position  px = (((float)x + 0.5f) / (float)w) * (float)lw - 0.5f
 *               py = (((float)y + 0.5f) / (float)h) * (float)lh - 0.5f
 *               fx = floorf(px), tx = px - fx, ix = (int)fx; fy, ty, iy likewise. For sides up to
 *               65536 and lw <= w, lh <= h this gives ix in [-1, lw - 1] and iy in [-1, lh - 1]
 *               ((x + 0.5) / w lies in (0, 1) after rounding too, since x + 0.5 is exact and below w);
 *               the in-image test is made on every tap regardless
 *   2 class     surface iff alpha(p) == 1.0f. Sky pixels and edge pixels take the id test only
 *   3 taps      t = (ix + i, iy + j), j = 0, 1 (outer loop), i = 0, 1 (inner loop), with
 *               wgt = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty). A tap outside the low-resolution
 *               image is skipped for both sets of sums. From pw = ps[3] = pv = 0 (the plain sums):
 *               pw = pw + wgt;  ps[c] = ps[c] + wgt * lo_color(t)[c]
 *               pv = pv + (wgt * wgt) * lo_variance(t)
 *               The guided sums gw, gs[3], gv are formed the same way from 0, but the tap is skipped
 *               when lo_sphere_id(t) != sphere_id(p), or, for a surface pixel, d2 > normal_tol with
 *               dn = lo_normal(t) - normal(p) per component and d2 = (dn.x dn.x + dn.y dn.y) + dn.z dn.z,
 *               or, for a surface pixel, fabsf(lo_depth(t) - depth(p)) > depth_tol * depth(p)
 *   4 result    gw >= 0.01f: out_color(p)[c] = gs[c] / gw, out_variance(p) = gv / (gw * gw) (the
 *               variance of a weighted mean, as §4.10's levels and §4.11's resample). Otherwise the
 *               plain bilinear value ps[c] / pw and pv / (pw * pw); pw >= 0.25, because the tap nearest
 *               to (px, py) lies inside the image and both of its factors are at least 0.5
 * NaN or infinite plane values give unspecified output values; no tap is read outside a plane whatever
 * the values are.
 *
 * Every argument is checked before any HIP call; RT_ERR_INVALID names the field: a wrong size, a side
 * outside 1..65536, lo_width > width or lo_height > height, a negative or non-finite tolerance,
 * nonzero flags, a null required plane, lo_variance given without out_variance or the reverse, an
 * output plane equal to an input plane or to the other output.                                        */
typedef struct rt_upsample_params {
    uint32_t size;                /* sizeof(rt_upsample_params): the record's revision (32 bytes)      */
    uint32_t width, height;       /* the output's, 1..65536                                            */
    uint32_t lo_width, lo_height; /* the low-resolution planes', 1..width, 1..height                   */
    float normal_tol;             /* >= 0: the largest squared normal distance of a guided tap         */
    float depth_tol;              /* >= 0: the largest relative depth difference of a guided tap       */
    uint32_t flags;               /* none defined: must be 0                                           */
} rt_upsample_params;
typedef struct rt_upsample_buffers {
    uint32_t size;                /* sizeof(rt_upsample_buffers)                                       */
    const float *lo_color;        /* [lh][lw][3] required                                              */
    const float *lo_variance;     /* [lh][lw]; given iff out_variance is                               */
    const float *lo_normal, *lo_depth;
    const uint32_t *lo_sphere_id; /* required                                                          */
    const float *normal, *depth, *alpha;
    const uint32_t *sphere_id;    /* [h][w], required                                                  */
    float *out_color;             /* [h][w][3] required                                                */
    float *out_variance;          /* [h][w] optional                                                   */
} rt_upsample_buffers;
/* The defaults (DESIGN.md §4.15 records the sweep that chose them). A zero side is RT_ERR_INVALID.   */
int rt_upsample_params_default(uint32_t width, uint32_t height, uint32_t lo_width, uint32_t lo_height,
                               rt_upsample_params *out);
/* Device pointers on the current device; one launch on `stream` (a hipStream_t, or NULL), no host
 * synchronisation, no allocation.                                                                     */
int rt_upsample_device(const rt_upsample_params *params, const rt_upsample_buffers *buffers, void *stream);
/* Host pointers, synchronous; the device planes are the library's (kept in the cached per-device
 * context rt_release_cached frees). stats (optional): kernel_ms, wall_ms; the counters are 0.         */
int rt_upsample(const rt_upsample_params *params, const rt_upsample_buffers *buffers, rt_stats *stats);

/* ---- the preview session: the whole denoised-preview loop, one call per frame ----
 * A device-resident object beside the stage entry points above. It owns every plane of the loop
 * rt_render_var -> rt_render_aov -> rt_temporal -> rt_denoise_var -> epilogue and the prev / cur
 * bookkeeping of guides and cameras, and enqueues one whole frame on the caller's stream per call:
 * no host synchronisation and no allocation after rt_preview_create beyond what rt_render_var_device
 * itself does on a camera's first use. With flags 0 a frame's bits are those of the five stage calls
 * made by hand. Two switches are capabilities the stage calls do not have:
 *
 * RT_PREVIEW_DEMODULATE  the temporal stage and the filter work on illumination, not on albedo x
 *   illumination. Per pixel p, binary32, every operation rounded on its own (the kernel preview_split):
 *     A'[c] = fmaxf(albedo(p)[c], 0.0078125f)            (RT_DENOISE_DEMODULATE's floor)
 *     I[c]  = beauty(p)[c] / A'[c]                       (IEEE division)
 *     LA    = (0.2126f * A'.r + 0.7152f * A'.g) + 0.0722f * A'.b
 *     V'    = variance(p) / (LA * LA)
 *   LA is exact for grey albedos and an approximation otherwise (the variance is that of the mean
 *   luminance and only scales the colour term). The stages run over I and V'; the last step
 *   multiplies back: out(p)[c] = F(p)[c] * A'[c] with F the filter's output.
 * RT_PREVIEW_FEEDBACK    as SVGF does, the first filter level's output C_1, V_1 is what the next frame
 *   reprojects (its prev_color, prev_variance), not the temporal stage's own output; levels 1..L-1
 *   continue from C_1, V_1. With levels == 1 the fed-back image is the frame's output.
 * RT_PREVIEW_NO_TEMPORAL the temporal stage is skipped: every frame is filtered on its own.
 *
 * One frame, all on `stream`, in this order:
 *   1 render   rt_render_var_device and rt_render_aov_device with rt_params {width, height, spp,
 *              max_depth, seed, every row, flags 0}, aov samples = 0, all five planes
 *   2 split    under DEMODULATE only (otherwise I = beauty, V' = variance: the same planes)
 *   3 temporal rt_temporal_device's launch over I, V', the frame's guides and the session's prev_
 *              planes and previous camera; no prev_ planes on the first frame and after
 *              rt_preview_reset; skipped under NO_TEMPORAL
 *   4 filter   rt_denoise_var_device's levels over the temporal outputs, guided by albedo, normal and
 *              depth. The next frame's prev_color and prev_variance are C_1, V_1 under FEEDBACK and
 *              the temporal outputs otherwise; its prev_history is out_history; its prev_ guides are
 *              this frame's guides; its previous camera is `camera`
 *   5 merge    one pass (the kernel preview_merge): out as above under DEMODULATE, the filter's bits
 *              otherwise, stored to d_rgb if given; the texel rt_epilogue_rgb8_device computes from
 *              those f32 bits stored to d_rgb8 if given
 *
 * rt_preview_create checks `p` field by field before it looks at `scene` and before any HIP call;
 * RT_ERR_INVALID names the field: a wrong size, width or height outside 1..65536, spp < 2, max_depth
 * 0, unknown flags, FEEDBACK with NO_TEMPORAL, a var_floor that is not positive and finite, then
 * every check rt_temporal makes on its params (named temporal.alpha_min ...; temporal.width and
 * .height must be the session's) and every check rt_denoise_var makes on its (denoise.levels ...;
 * denoise.flags may hold RT_DENOISE_DIRECT only: the session's flag is the way to demodulate); then
 * a null scene. What the two render calls refuse (a scene that does not fit LDS ...) comes back from
 * the frame call as they report it; a failing frame call leaves the session's history as it was.
 * A session uses its scene: destroy it before the scene. One host thread per session; sessions on
 * one scene are independent.                                                                      */
enum rt_preview_flags {
    RT_PREVIEW_DEMODULATE = 1u << 0,
    RT_PREVIEW_FEEDBACK = 1u << 1,
    RT_PREVIEW_NO_TEMPORAL = 1u << 2
};
typedef struct rt_preview_params {
    uint32_t size;                /* sizeof(rt_preview_params): the record's revision              */
    uint32_t width, height;
    uint32_t spp, max_depth;      /* of every frame's render; spp >= 2                             */
    uint32_t flags;               /* rt_preview_flags                                              */
    float var_floor;              /* rt_denoise_var_buffers.var_floor                              */
    rt_temporal_params temporal;  /* width / height must equal the session's                       */
    rt_denoise_params denoise;    /* likewise; flags: 0 or RT_DENOISE_DIRECT                       */
} rt_preview_params;
/* What the last enqueued frame wrote (device pointers, valid until the next frame call; all NULL
 * before the first one): the temporal stage's outputs, the frame's guides, and the planes the next
 * frame will take as prev_. Under NO_TEMPORAL out_color and out_variance are I and V', out_history
 * and the prev_ planes are NULL. After rt_preview_reset the next frame ignores the prev_ planes. */
typedef struct rt_preview_planes_t {
    uint32_t size;                /* sizeof(rt_preview_planes_t), filled by the call               */
    uint32_t frames;              /* frames enqueued since creation or the last reset              */
    const float *out_color, *out_variance, *out_history;
    const float *albedo, *normal, *depth, *alpha;
    const uint32_t *sphere_id;
    const float *prev_color, *prev_variance, *prev_history, *prev_normal, *prev_depth;
    const uint32_t *prev_sphere_id;
} rt_preview_planes_t;
typedef struct rt_preview rt_preview;
/* The defaults: the sub-records from rt_temporal_params_default and rt_denoise_var_params_default,
 * max_depth 64, the flags scripts/preview_sweep.py chose (RT_PREVIEW_DEMODULATE).
 * A zero width or height or spp < 2 is RT_ERR_INVALID.                                           */
int rt_preview_params_default(uint32_t width, uint32_t height, uint32_t spp, rt_preview_params *out);
/* Allocates every plane of the session on the scene's device (one allocation).                  */
int rt_preview_create(rt_scene *scene, const rt_preview_params *p, rt_preview **out);
/* Enqueue one frame. d_rgb: [height][width][3] floats (linear) or NULL; d_rgb8: [height][width][3]
 * bytes (gamma 1/2.2) or NULL; one of them must be given (an upscaled session, below: both of its
 * output size). A NULL camera is RT_ERR_INVALID.                                                   */
int rt_preview_frame_device(rt_preview *pv, const rt_camera *camera, uint64_t seed, float *d_rgb, uint8_t *d_rgb8,
                            void *stream);
/* The next frame has no history (as the first one). Nothing is enqueued.                          */
int rt_preview_reset(rt_preview *pv);
/* The history clamp of rt_temporal_clip_device as a switch of the session: from the
 * next frame on, step 3 is rt_temporal_clip_device's launch with `clip` (a copy is kept) in the place of
 * rt_temporal_device's, over the same planes (under RT_PREVIEW_DEMODULATE the window is taken over the
 * illumination I, which is what the stage sees as its beauty) and, after one step of the scene's
 * geometry, with the scene's two tables as today. clip NULL: off, as after creation. Ordinary and
 * upscaled sessions alike. Nothing is enqueued and the history is kept. RT_ERR_INVALID: a null
 * session, a session with RT_PREVIEW_NO_TEMPORAL (it has no temporal stage), and the record's own
 * checks as rt_temporal_clip_device makes them (the session is then left as it was).              */
int rt_preview_set_clip(rt_preview *pv, const rt_temporal_clip_t *clip);
int rt_preview_planes(rt_preview *pv, rt_preview_planes_t *out);
/* The bytes of the session's device allocation (the scene's own workspaces: rt_scene_usage_get). */
int rt_preview_usage(const rt_preview *pv, uint64_t *bytes);
void rt_preview_destroy(rt_preview *pv);
/* The session's two kernels on planes of the caller's (device pointers, one launch on `stream`, no
 * host synchronisation): step 2 above, and step 5 (albedo NULL: out = the bits of `filtered`; one of
 * d_rgb, d_rgb8 must be given). RT_ERR_INVALID names a null plane or a side outside 1..65536.    */
int rt_preview_split_device(uint32_t width, uint32_t height, const float *beauty, const float *variance,
                            const float *albedo, float *illumination, float *variance_out, void *stream);
int rt_preview_merge_device(uint32_t width, uint32_t height, const float *filtered, const float *albedo, float *d_rgb,
                            uint8_t *d_rgb8, void *stream);
/* ---- the upscaled session: a render scale --------------------------------------
 * A session whose frames are rendered, accumulated and filtered at `p`'s size and shown at a larger
 * one. rt_preview_params keeps describing the render resolution; this record adds the output. A frame
 * of such a session, all on the caller's stream, no host synchronisation, no allocation after creation:
 *   1-4        steps 1 to 4 above exactly as an ordinary session of the same `p` enqueues them
 *   5 guides   rt_render_aov_device with rt_params {out_width, out_height, p->spp, p->max_depth, seed,
 *              every row, flags 0} and samples = guide_samples: normal, depth, alpha, sphere_id, and
 *              albedo only under RT_PREVIEW_DEMODULATE
 *   6 upsample rt_upsample_device's launch: lo_color the filter's output (the plane step 5 of an
 *              ordinary session would have merged), the low-resolution guides the frame's, the
 *              output-size guides step 5's, no variance
 *   7 merge    preview_merge at the output size: under DEMODULATE out = upsampled * max(albedo, 2^-7)
 *              with the output-size albedo (the low-resolution one served the split), the upsampled
 *              bits otherwise; d_rgb and d_rgb8 are [out_height][out_width][3]
 * rt_preview_planes keeps reporting the render-size planes, rt_preview_reset and the history (which
 * lives at the render size) are untouched, rt_preview_usage counts the output-size planes (part of
 * the one allocation). rt_preview_create_upscaled checks `p` as rt_preview_create does, then `u` field
 * by field (RT_ERR_INVALID names it: a wrong size, out_width or out_height outside 1..65536 or below
 * p's, a product of 2^31 or more, guide_samples above p->spp, a negative or non-finite tolerance),
 * then the scene, all before any HIP call.                                                          */
typedef struct rt_preview_upscale {
    uint32_t size;                  /* sizeof(rt_preview_upscale)                                       */
    uint32_t out_width, out_height; /* >= p->width, p->height; 1..65536, product below 2^31             */
    uint32_t guide_samples;         /* samples of the output-size guide pass, 0 = p->spp, <= p->spp     */
    float normal_tol, depth_tol;    /* rt_upsample_params'                                              */
} rt_preview_upscale;
/* out_width x out_height with guide_samples 0 and rt_upsample_params_default's tolerances.            */
int rt_preview_upscale_default(const rt_preview_params *p, uint32_t out_width, uint32_t out_height,
                               rt_preview_upscale *out);
int rt_preview_create_upscaled(rt_scene *scene, const rt_preview_params *p, const rt_preview_upscale *u,
                               rt_preview **out);
/* What the last frame of an upscaled session wrote at the output size (device pointers, valid until
 * the next frame call; NULL before the first one; albedo NULL without RT_PREVIEW_DEMODULATE).
 * RT_ERR_INVALID on a session made by rt_preview_create.                                              */
typedef struct rt_preview_output_t {
    uint32_t size, width, height;   /* filled by the call                                               */
    const float *upsampled, *albedo, *normal, *depth, *alpha;
    const uint32_t *sphere_id;
} rt_preview_output_t;
int rt_preview_output(rt_preview *pv, rt_preview_output_t *out);

/* ---- the progressive session: a frame in sample windows --------------------------
 * A session fixes a scene, a camera and an rt_params record P. P.spp = N >= 2 is the WHOLE frame's
 * sample count; the row fields and RT_FLAG_FULL_FRAME are honoured; flags are accepted or refused
 * exactly as rt_render_var_device does. The session owns two device planes of n_pixels x 3 floats
 * (n_pixels = P.width x the rows P renders), the running sums `acc` and the luminance moments
 * {L_0, m1, m2} of rt_render_var_device's accumulation, and a count `done`: 0 after creation, and always
 * a multiple of 4 or equal to N.
 *   Step(n)  m = min(n, N - done). n % 4 != 0 with n < N - done is RT_ERR_INVALID (passes start on
 *            multiples of 4). n = 0 or done = N renders nothing. Otherwise samples [done, done + m) of
 *            the N-sample frame are rendered (the keys (pixel) * N + s, the streams and the sample
 *            numbers are the frame's) and folded into the planes by the accumulation of
 *            rt_render_var_device, in that frame's own addition order: per block of 4 samples
 *            acc = acc + ((c0 + c1) + (c2 + c3)), then the N % 4 tail one by one, which arrives with
 *            the last window; the moments sample by sample. Then done += m.
 *   Resolve  (out given; done >= 2) for every rendered pixel, d = done, every operation binary32 and
 *            rounded on its own: nf = (float)d; rgb[c] = acc[c] / nf; mean = m1 / nf; ex2 = m2 / nf;
 *            var = fmaxf(0.0f, ex2 - mean * mean) / (float)(d - 1); rgb8[c] = the texel of rgb[c]
 *            (pow(c, 1 / 2.2f) in double, narrowed, then (uint8)(255 c)). Laid out as P says; only
 *            the planes given are written. With d = N these are rt_render_var_device's bits for the
 *            same arguments, hence rt_render_device's.
 *   Noise    (out->noisy given) t2 = noise_tau * noise_tau formed once on the host in binary32;
 *            L = (0.2126f * rgb.r + 0.7152f * rgb.g) + 0.0722f * rgb.b; a pixel is noisy iff
 *            var > t2 * (L * L). The step zeroes the word on the stream and the resolve adds the
 *            number of noisy rendered pixels; the caller reads it when it likes, the library never
 *            waits for it.
 * The estimate after d < N samples is NOT a d-sample frame (the keys differ): it is the prefix of the
 * N-sample frame's own sample set. A step is planned like the variance render, as under RT_DIAG_NO_PAIRS
 * | RT_DIAG_NO_SKY: single-sample slots, proven-sky tiles traced by the main launch; the cut into
 * passes is made for the window's samples and never changes the bits.
 * Several sessions on one scene are independent, and plain or multi-pass renders on that scene between
 * two steps do not disturb them (the sums belong to the session, not to the scene). A step does no host
 * synchronisation and no allocation after creation beyond what rt_render_var_device itself does; steps
 * of one session are ordered through its planes in the scene's stream order. After rt_scene_update
 * moved either epoch of the scene a step is RT_ERR_INVALID with nothing enqueued, until
 * rt_progressive_reset. rt_scene_usage does not count a session: rt_progressive_info reports its own
 * 24 B per pixel.                                                                                     */
typedef struct rt_progressive rt_progressive;
typedef struct rt_progressive_outputs {
    uint32_t size;       /* sizeof(rt_progressive_outputs)                                           */
    float noise_tau;     /* finite, >= 0; read only when noisy is given                              */
    float *rgb;          /* optional: linear f32, as rt_render_device lays it out                    */
    float *variance;     /* optional: one float per pixel, as rt_render_var_device lays it out       */
    uint8_t *rgb8;       /* optional: gamma 1/2.2 texels, 3 bytes per pixel, laid out as rgb         */
    uint32_t *noisy;     /* optional: one device word, zeroed by the step, the count added           */
} rt_progressive_outputs;
typedef struct rt_progressive_info_t {
    uint32_t size;         /* filled by the call                                                     */
    uint32_t done, spp;    /* samples folded so far, and N                                           */
    uint32_t reserved;
    uint64_t n_pixels;     /* pixels the session renders                                             */
    uint64_t state_bytes;  /* what rt_progressive_save writes                                        */
    uint64_t device_bytes; /* the session's device allocation: 24 B per pixel                        */
} rt_progressive_info_t;
/* Supported API, like rt_progressive_blob_check below: a caller sizes its windows, or inspects a
 * checkpoint before it creates a session, with the library's own rule.
 * The Step rule alone (host arithmetic, no session): *m = min(n_samples, spp - done), or
 * RT_ERR_INVALID (n_samples is not a multiple of 4 and stops before the frame's end; done is not a
 * multiple of 4 or spp; done > spp; spp < 2; m null).                                                */
int rt_progressive_window(uint32_t spp, uint32_t done, uint32_t n_samples, uint32_t *m);
/* Checks params (as rt_render_var_device: RT_ERR_INVALID / RT_ERR_UNSUPPORTED, before the scene is
 * looked at), camera, scene and out, then allocates both planes on the scene's device.               */
int rt_progressive_create(rt_scene *scene, const rt_camera *camera, const rt_params *params, rt_progressive **out);
/* Step(n_samples), then Resolve (and Noise) when `out` is not NULL, on `stream`. Every argument is
 * checked before any HIP call and RT_ERR_INVALID names the field: out's record first (a wrong size, no
 * plane and no count given, two of its pointers equal, a noise_tau that is negative or not finite with
 * noisy given), then a null session, the Step rule, `out` given while done + m < 2, the scene's
 * epochs (a resolve-only step, n_samples = 0 with `out`, is refused after a scene update too, although
 * the planes still hold the old scene's estimate). d_segments: optional device uint64[3], as
 * rt_render_device: the step adds its render's counts and never zeroes them; a step that renders nothing
 * leaves them alone.                                                                                  */
int rt_progressive_step_device(rt_progressive *pg, uint32_t n_samples, const rt_progressive_outputs *out, void *stream,
                               uint64_t *d_segments);
int rt_progressive_info(const rt_progressive *pg, rt_progressive_info_t *info);
/* done = 0 with a new camera and / or seed (NULL: kept); the scene's epochs are taken anew. Nothing is
 * enqueued, nothing allocated.                                                                        */
int rt_progressive_reset(rt_progressive *pg, const rt_camera *camera, const uint64_t *seed);
/* Checkpoints. save waits for the session's enqueued work and writes state_bytes bytes: a header
 * {magic, RT_API_VERSION, layout tag, rt_params, rt_camera, n_pixels, done}, then both planes
 * (RT_ERR_CAPACITY: cap is smaller). load waits likewise, refuses a header that does not match the
 * session (RT_ERR_INVALID, the field named) and a buffer shorter than the header or than state_bytes
 * (RT_ERR_CAPACITY), then uploads the planes and takes `done`; the epochs are taken anew as by reset. The
 * blob is opaque and valid for the same library build; the scene's identity is the caller's business.
 * rt_progressive_blob_check is load's check alone, against a params / camera pair, without a session
 * (info optional: done, spp, n_pixels, state_bytes of the blob).                                      */
int rt_progressive_save(rt_progressive *pg, void *host, uint64_t cap);
int rt_progressive_load(rt_progressive *pg, const void *host, uint64_t bytes);
int rt_progressive_blob_check(const void *host, uint64_t bytes, const rt_params *params, const rt_camera *camera,
                              rt_progressive_info_t *info);
int rt_progressive_destroy(rt_progressive *pg);
/* The preview session at rest: once the camera stops, a preview session refines
 * towards the frame the library exists to produce instead of blending new noisy frames. The session
 * owns a progressive session (allocated on the first call, counted by rt_preview_usage) for the frame
 * rt_params {width, height, total_spp, max_depth, seed, every row, flags 0}. A call starts a new
 * refinement when camera, seed or total_spp differ from the one in progress, when either epoch of the
 * scene moved, or when rt_preview_frame_device was called in between. On a start the guides (albedo,
 * normal, depth, alpha, sphere_id) are rendered once by rt_render_aov_device with those params and
 * samples = min(total_spp, p->spp). Every call, on `stream`, no host synchronisation:
 *   1 step     rt_progressive_step_device(n_samples) resolved into the session's beauty and variance
 *              planes (the Step rule holds; the first call of a refinement renders at least 2 samples)
 *   2 split    under RT_PREVIEW_DEMODULATE, as a frame's step 2
 *   3 filter   as a frame's step 4 on that colour and variance: no temporal stage; the carried variance
 *              shrinks as samples arrive, so the filter narrows by itself
 *   4 merge    as a frame's step 5 into d_rgb and / or d_rgb8 ([height][width][3])
 * The call that completes the frame (done = total_spp), and any call after it, stores the frame itself,
 * unfiltered: the resolve's f32 bits (rt_render_device's for those params) and their texels. After a
 * refinement the next rt_preview_frame_device has no history, as after rt_preview_reset.
 * RT_ERR_UNSUPPORTED on an upscaled session; RT_ERR_INVALID names a null argument, total_spp < 2 or
 * n_samples. rt_preview_refine_info: samples done and the total of the refinement in progress (0, 0:
 * none).                                                                                              */
int rt_preview_refine_device(rt_preview *pv, const rt_camera *camera, uint64_t seed, uint32_t total_spp, uint32_t n_samples,
                             float *d_rgb, uint8_t *d_rgb8, void *stream);
int rt_preview_refine_info(const rt_preview *pv, uint32_t *done, uint32_t *total);

/* ---- the adaptive session: a progressive session that retires converged tiles -----
 * A session of its own type beside rt_progressive_* (whose contract above is unchanged). It fixes a
 * scene, a camera, an rt_params record P and an rt_adaptive_params record. P.spp = N >= 2 is the cap of
 * every pixel's sample count; P's row fields, RT_FLAG_FULL_FRAME and flags are taken or refused exactly
 * as rt_progressive_create does. noise_tau is finite and >= 0, max_noisy is in 0..63, min_samples is a
 * multiple of 4 and >= 4.
 *   Blocks   the 64-pixel blocks of P's natural enumeration: the 8 x 8 tiles over the tiled rows in
 *            row-major tile order, then row-major runs of 64 pixels over the leftover rows. B of them;
 *            n_pixels % 64 != 0 is RT_ERR_UNSUPPORTED at creation.
 *   State    the two planes of a progressive session, acc and mom (24 B per pixel); per block one
 *            uint32 d_b, the samples folded into it (0 at start), and one flag word; the frontier
 *            `done`; the active set A (every block at start); two permutation buffers of B words; four
 *            count words on the device and in pinned host memory.
 *   Step(n)  1 Render. A empty or done == N: nothing is rendered. Otherwise m is the progressive Step
 *              rule's (rt_progressive_window(N, done, n)), and samples [done, done + m) of the N-sample
 *              frame are rendered FOR THE PIXELS OF THE BLOCKS IN A ONLY (the keys (pixel) * N + s, the
 *              streams and the sample numbers are the frame's) and folded into the planes by the
 *              accumulation of rt_render_var_device in the frame's own addition order, as a progressive
 *              step does. Then done += m and d_b = done for every b in A: every active block has the
 *              same d_b, which is what makes one window serve them all.
 *            2 Resolve (whenever done >= 2, also without `out`). For every pixel the progressive
 *              session's Resolve with d = d_b of its block. The outputs that are given are written for
 *              the whole frame: rgb, variance, rgb8 and `samples`, a uint32 plane laid out like variance
 *              that holds d_b. A retired block's pixels are written again, with the same bits, at
 *              every step.
 *            3 Retire. t2 = noise_tau * noise_tau formed once on the host in binary32; a pixel is noisy
 *              iff var > t2 * (L * L), the progressive session's expression; c_b = the noisy pixels of
 *              block b. A block b of A leaves A when d_b >= min_samples and c_b <= max_noisy. A never
 *              grows. out->noisy (optional; the step zeroes the word first) receives the sum of c_b over
 *              ALL blocks, each at its own d_b.
 *            4 Compact. The next step's dealing order is the frame's dealing order restricted to A,
 *              relative order kept: the frame's order is the one its progressive window would take for
 *              this camera and rows (lead tiles, others, proven-sky tiles), and the identity with every
 *              block in the middle class where the scene or the flags have no tile classes
 *              (RT_FLAG_BRUTE_FORCE, a scene without clusters). The three class counts are counted
 *              again; {|A|, lead, others, sky} go to the pinned words and an event is recorded.
 * The host wait: the host sizes a step's launches from these counts, so before a step plans its passes
 * it waits for the previous step's event, and for nothing else: one short event wait per step (like a
 * first render under rt_options.tile_classes = 1). rt_adaptive_info makes the same wait.
 * The session is finished when done == N or A is empty; further steps render nothing and resolve
 * again. With min_samples >= N nothing retires before the end: every step's outputs are then the
 * progressive session's bits, and after the last window rt_render_var_device's, hence rt_render_device's
 * (this follows from the rules; it is not a mode). A pixel that stopped after d samples holds the
 * d-sample prefix of the N-sample frame's own sample set.
 * A step is planned like a progressive step over 64 |A| pixel positions (single-sample slots, no sky
 * and no ground kernel); the cut into passes never changes the bits. Several adaptive and progressive
 * sessions on one scene, and plain renders between their steps, do not disturb each other. After
 * rt_scene_update moved either epoch a step is RT_ERR_INVALID with nothing enqueued, until
 * rt_adaptive_reset. rt_scene_usage does not count a session: rt_adaptive_info reports its bytes.
 * Not provided: checkpoints of an adaptive session, re-activating a retired block, masks inside a block. */
typedef struct rt_adaptive rt_adaptive;
typedef struct rt_adaptive_params {
    uint32_t size;        /* sizeof(rt_adaptive_params)                                               */
    float noise_tau;      /* finite, >= 0: a pixel is noisy iff var > tau^2 L^2                       */
    uint32_t max_noisy;   /* 0..63: a block retires with at most this many noisy pixels               */
    uint32_t min_samples; /* a multiple of 4, >= 4: no block retires with fewer samples               */
} rt_adaptive_params;
typedef struct rt_adaptive_outputs {
    uint32_t size;       /* sizeof(rt_adaptive_outputs)                                               */
    uint32_t reserved;   /* 0                                                                         */
    float *rgb;          /* optional: linear f32, as rt_render_device lays it out                     */
    float *variance;     /* optional: one float per pixel, as rt_render_var_device lays it out        */
    uint8_t *rgb8;       /* optional: gamma 1/2.2 texels, 3 bytes per pixel, laid out as rgb          */
    uint32_t *samples;   /* optional: d_b of the pixel's block, one word per pixel, laid out as variance */
    uint32_t *noisy;     /* optional: one device word, zeroed by the step, the sum of c_b added       */
} rt_adaptive_outputs;
typedef struct rt_adaptive_info_t {
    uint32_t size;             /* filled by the call                                                  */
    uint32_t done, spp;        /* the frontier, and N                                                 */
    uint32_t n_blocks;         /* B                                                                   */
    uint32_t active_blocks;    /* |A| after the last step                                             */
    uint32_t finished;         /* 1: done == N or A is empty                                          */
    uint64_t n_pixels;         /* pixels of the frame the session covers: 64 B                        */
    uint64_t samples_rendered; /* 64 x the sum of d_b                                                 */
    uint64_t device_bytes;     /* the session's device allocation: 24 B per pixel, 16 B per block, the counts */
} rt_adaptive_info_t;
/* Every argument is checked before any HIP call and RT_ERR_INVALID names the field: the adaptive
 * record first (null, size, noise_tau, max_noisy, min_samples), then params as rt_progressive_create
 * (RT_ERR_INVALID / RT_ERR_UNSUPPORTED), n_pixels % 64 (RT_ERR_UNSUPPORTED), camera, scene and out;
 * then the planes, the block words and both permutation buffers are allocated on the scene's device. */
int rt_adaptive_create(rt_scene *scene, const rt_camera *camera, const rt_params *params, const rt_adaptive_params *adaptive,
                       rt_adaptive **out);
/* Step(n_samples) on `stream`. Checked before any HIP call, RT_ERR_INVALID naming the field: out's
 * record first (a wrong size, two of its pointers equal; `out` may be NULL and may hold no plane: the
 * step then retires and compacts only), then a null session, the Step rule, `out` given while
 * done + m < 2, the scene's epochs. Then the host wait above. d_segments: optional device uint64[3] as
 * rt_progressive_step_device: the step adds its render's counts; a step that renders nothing leaves
 * them alone.                                                                                         */
int rt_adaptive_step_device(rt_adaptive *ad, uint32_t n_samples, const rt_adaptive_outputs *out, void *stream,
                            uint64_t *d_segments);
/* Waits for the last step's counts (the host wait above), then reports.                               */
int rt_adaptive_info(rt_adaptive *ad, rt_adaptive_info_t *info);
/* d_b of every block, in natural block order, into host[0 .. B): synchronous (it waits for the
 * session's enqueued work); for tools and tests. RT_ERR_CAPACITY: cap < B.                            */
int rt_adaptive_blocks(rt_adaptive *ad, uint32_t *host, uint32_t cap);
/* A = every block, d_b = 0, done = 0, with a new camera and / or seed (NULL: kept); the scene's epochs
 * are taken anew. Nothing is enqueued, nothing allocated.                                             */
int rt_adaptive_reset(rt_adaptive *ad, const rt_camera *camera, const uint64_t *seed);
int rt_adaptive_destroy(rt_adaptive *ad);
/* The compaction stage alone, on device pointers without a session (the kernel of Step 4): d_src_perm
 * holds n_blocks distinct block numbers below n_blocks, of which the first class_counts[0] are the lead
 * class, the next class_counts[1] the middle class and the last class_counts[2] the sky class (host
 * array; their sum must be n_blocks); d_active holds one word per natural block, nonzero = kept.
 * d_out_perm[0 .. kept) receives the kept entries in d_src_perm's order (entries past `kept` are left
 * alone), d_counts[0 .. 4) = {kept, kept lead, kept middle, kept sky}. One launch on `stream` of the
 * current device, no host synchronisation. RT_ERR_INVALID names a null pointer, n_blocks = 0 or above
 * 2^26, a class sum that is not n_blocks, d_out_perm == d_src_perm.                                    */
int rt_block_compact_device(const uint32_t *d_src_perm, uint32_t n_blocks, const uint32_t class_counts[3],
                            const uint32_t *d_active, uint32_t *d_out_perm, uint32_t *d_counts, void *stream);

/* Device memory a scene holds and how its renders are cut (after the last render call).  */
typedef struct rt_scene_usage {
    uint64_t device_bytes;     /* every device allocation of the scene                       */
    uint64_t workspace_bytes;  /* of which workspaces (bounded by max_workspace_bytes)       */
    uint32_t render_streams;   /* streams the last render rotated over (1: caller's only)    */
    uint32_t workspaces;       /* slot workspaces in use                                     */
    uint32_t pass_samples;     /* samples per pass of the last render                        */
    uint32_t static_lds_bytes; /* the culled render kernel's static LDS per workgroup        */
    uint32_t max_lds_bytes;    /* the device's LDS per workgroup                              */
    uint32_t deep_launch;      /* the last render's last deep-path launch: waves per workgroup
                                  (4: beside other renders; 8: a lone pass, shading records in
                                  LDS) | 16 when it dealt its chunks statically; 0 = none      */
    uint32_t pair_passes;      /* passes of the last render that stored sample pairs          */
    uint32_t split_passes;     /* passes of the last render with a deep-path launch           */
    uint32_t lead_tiles;       /* the last pass: 64-pixel tiles dealt first (a primary can meet
                                  a dielectric sphere), 0 = natural order      */
    uint32_t sky_tiles;        /* the last pass: tiles whose primaries are proven to reach the
                                  sky (dealt last, no closest-hit test)                        */
} rt_scene_usage;
int rt_scene_usage_get(const rt_scene *scene, rt_scene_usage *out);
/* Spans (ms, HIP events) of the render kernels of the most recent calls of
 * rt_render_device on this scene, oldest first: entry i runs from the start event of the
 * call's first pass to the end event of its last pass. Consecutive calls' launches run
 * side by side (frames in flight), so a span also covers time the GPU spent on other
 * calls' renders and accumulations: it is a latency, not a per-frame cost. Writes up to
 * `max` entries, *n = entries written. Waits for those calls to finish.                 */
int rt_scene_kernel_times(rt_scene *scene, uint32_t max, float *ms, uint32_t *n);
/* Diagnostics: with RT_DIAG_STATS in the scene's options, its renders use an
 * instrumented kernel (identical output) that tallies: [0] wave loop iterations,
 * [1] wave refill rounds, [2] wave / [3] lane sphere blocks with a positive discriminant,
 * [4] wave / [5] lane root evaluations, [6] segments, [7] wave-level blocks of 8 cluster
 * members executed, [8..12] shader-clock cycles summed over waves per loop region
 * (refill, sample start + rejection loop, closest hit, shading, fold), [13] items dealt (the
 * deep launch: queued paths), [14] ~(earliest wave
 * start, 100 MHz clock), [15] the bounds check's first violation, code << 32 | index
 * (rt_device.h BoundsCode; 0 = none). Copies them out; reset zeroes. Returns RT_ERR_DEVICE
 * (the message names the index) when [15] is set: the instrumented kernel checks every
 * lane-computed index into the scene, the sample slots and the deep queue before using it. */
int rt_scene_debug_counters(rt_scene *scene, uint64_t out[16], int reset);
/* Diagnostics: per-wave records of the last instrumented render launch, out[4w .. 4w+3] for
 * wave w of the grid = {time the wave found every queue dry, exit} (100 MHz realtime
 * clock), (shader-clock cycles in the loop << 32 | refill rounds << 16 | loop iterations),
 * and (hardware CU id << 48 | iterations after dry (a deep launch: iterations in which the wave
 * walked the clusters) << 32 | low 32 bits of the wave's start on
 * the realtime clock); at most max_waves records, *n = records written (0 without
 * RT_DIAG_STATS).                                                                            */
int rt_scene_debug_timeline(rt_scene *scene, uint64_t *out, uint32_t max_waves, uint32_t *n);
/* Diagnostics: with RT_DIAG_STATS, how often each block of the render loop ran, counted once
 * per wave per execution, summed over the instrumented launches since the last reset: [0] loop
 * iterations, [1] refill trips, [2] sample starts, [3] rejection attempts, [4] lens rays done,
 * [5] scatters done, [6] root-box passes, [7] level-2 boxes walked, [8] level-2 boxes passed,
 * [9] clusters requested, [10] transposed member tests, [11] their rounds, [12] their far-root
 * passes, [13] per-lane member tests, [14] sky, [15] hit shading, [16] lambert, [17] unit
 * direction (metal/dielectric), [18] dielectric, [19] sample stores, [20] metal absorptions,
 * [21] live lanes summed over iterations, [22] iterations after the item queues ran dry, [23]
 * live lanes summed over those, [24] lanes that skipped the walk (shortcut), [25] iterations
 * whose walk no lane needed, [26..29] iterations whose walk 1, 2, 3-4, 5-8 lanes needed.                                        */
int rt_scene_debug_events(rt_scene *scene, uint64_t out[32], int reset);
/* Enqueue the gamma/u8 epilogue over n_pixels RGB f32 texels.                          */
int rt_epilogue_rgb8_device(const float *d_rgb, uint8_t *d_out, uint64_t n_pixels,
                            void *stream);

/* ---- persistent multi-GPU context (row tiles over ranks, gather over xGMI) ----------
 * Rank r of n_ranks renders rows y = r, r + n, ... of every frame on device devices[r]
 * (devices = NULL: rank r on device r) into a packed tile; tiles are gathered to rank 0's
 * device with RCCL send/recv when every rank has its own device, and de-interleaved into
 * the caller's frame. Scenes, streams and communicators are built once here; tiles and the
 * gather buffer are allocated on first use of a frame size. Ranks that share a device with
 * rank 0 ("virtual ranks", e.g. devices = {0, 0, 0, 0}: an N-way split rehearsed on one
 * GPU) move their tiles with device copies instead of RCCL; the result is the same frame.
 * A device list is either all distinct or all equal to devices[0]; a mix is RT_ERR_INVALID. */
typedef struct rt_multi rt_multi;
enum rt_output_format { RT_OUTPUT_F32 = 0, RT_OUTPUT_RGB8 = 1 };
int rt_multi_create(const rt_sphere *spheres, uint32_t n_spheres,
                    const rt_material *materials, uint32_t n_materials,
                    const int *devices, int n_ranks, rt_multi **out);
/* The same with explicit options for every rank's scene (NULL: the process default).     */
int rt_multi_create_ex(const rt_sphere *spheres, uint32_t n_spheres,
                       const rt_material *materials, uint32_t n_materials,
                       const int *devices, int n_ranks, const rt_options *options,
                       rt_multi **out);
int rt_multi_destroy(rt_multi *ctx);
/* n_ranks, and whether the gather runs over RCCL (1) or device copies (0).              */
int rt_multi_info(const rt_multi *ctx, int *n_ranks, int *uses_rccl);
/* Enqueue one full frame (params' row fields and RT_FLAG_FULL_FRAME are ignored; the
 * other flags apply on every rank) into d_out on rank 0's device: height*width*3 floats
 * (RT_OUTPUT_F32) or bytes (RT_OUTPUT_RGB8). Rank 0 renders on `stream` (a stream of rank
 * 0's device) and the frame is complete in `stream` order; other ranks run on their own
 * streams. No host synchronisation, except when a frame is larger than any before it
 * (buffers grow). Frames stream: each rank overlaps consecutive renders as
 * rt_render_device does. One host thread per context.                                   */
int rt_multi_render_device(rt_multi *ctx, const rt_camera *camera, const rt_params *params,
                           uint32_t format, void *d_out, void *stream);
/* Synchronous host-buffer frames through a context (full frame, row 0 = top); stats sum
 * every rank's counters, kernel_ms spans the frame on rank 0's device.                   */
int rt_multi_render_f32(rt_multi *ctx, const rt_camera *camera, const rt_params *params,
                        float *rgb_out, rt_stats *stats);
int rt_multi_render_rgb8(rt_multi *ctx, const rt_camera *camera, const rt_params *params,
                         uint8_t *rgb_out, rt_stats *stats);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RT_API_H */
