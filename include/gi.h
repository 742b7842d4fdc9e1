/*
 * gi.h -- C-ABI drop-in boundary of the MI355X-native photon-mapping renderer.
 *
 * Plain C: pointers, sizes and POD structs only (no C++ / torch types). One context owns one
 * HIP device, the uploaded scene, the photon maps (device-resident) and all scratch buffers.
 * Calls are synchronous and NOT re-entrant per context. Errors are integer status codes; the
 * library never calls exit(); the message of the last failure is returned by gi_last_error().
 *
 * Each entry point names the reference interface it replaces (ReillyBova/Global-Illumination,
 * paths relative to src/):
 *
 *   gi_parse_args           ParseArgs             utils/io_utils.cpp:16-212 (flag set, defaults
 *                                                  photonmap.cpp:27-106)
 *   gi_read_scene           ReadScene / R3Scene::ReadFile (.scn Princeton + .off)
 *                                                  utils/io_utils.cpp:219-250,
 *                                                  R3Graphics/R3Scene.cpp:514-587, 1462-1953
 *   gi_map_photons          static void MapPhotons(void)           photonmap.cpp:260-436
 *   gi_render_image         R2Image *RenderImage(int aa,int w,int h) render.cpp:155-259
 *   gi_render_tiles         the column interleave of Threadable_RayTracer (render.cpp:90)
 *                           re-cut as an image-tile shard for multi-GPU ranks
 *   gi_estimate_radiance_batch   EstimateRadiance(...)     utils/photon_utils.cpp:72-162
 *   gi_knn_batch            R3Kdtree<Photon*>::FindClosestQuick  R3Shapes/R3Kdtree.cpp:688-848
 *   gi_intersect_batch      R3Scene::Intersects(ray, ...)        R3Graphics/R3Scene.cpp:471-479
 *   gi_write_image          WriteImage / R2Image::Write (png: row flip R2Image.cpp:1430, ppm)
 *
 * The photon record is the exchange format of the photon maps (20 B; on device it is split
 * into a 16-B position stream and a 4-B RGBE stream, DESIGN.md "Data layout"): positions are fp32 (reference: fp64 R3Point,
 * render.h:17-21), power in Ward RGBE (as the reference), direction as the reference's
 * 8+8-bit spherical code (photon_utils.cpp:56-60).
 */
#ifndef GI_H
#define GI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes -------------------------------------------------------------------- */
enum {
  GI_OK = 0,
  GI_ERR_ARG = 1,         /* bad argument / flag (reference: "Invalid program argument", exit 1) */
  GI_ERR_IO = 2,          /* scene / image file error (reference: exit(-1)) */
  GI_ERR_HIP = 3,         /* HIP runtime failure */
  GI_ERR_STATE = 4,       /* call out of order (e.g. render before scene) */
  GI_ERR_UNSUPPORTED = 5, /* feature not available on the device path */
  GI_ERR_ALLOC = 6        /* device / host allocation failure */
};

enum { GI_FILTER_DISK = 0, GI_FILTER_CONE = 1, GI_FILTER_GAUSS = 2 }; /* render.h Filter_Type */
enum { GI_MAP_GLOBAL = 0, GI_MAP_CAUSTIC = 1 };                      /* render.h Photon_Type */
/* an estimate size no map reaches: every estimate is a fixed-radius one (all photons within the
 * estimate distance, normalised by that distance, as EstimateRadiance does below K photons) */
#define GI_ESTIMATE_ALL (1 << 30)

/* ---- parameters: one field per reference global (photonmap.cpp:40-106, render.h:27-81) -- */
typedef struct gi_params {
  int32_t verbose;              /* VERBOSE                        -v            */
  int32_t threads;              /* THREADS (host CPU threads)     -threads N    */
  int32_t fresnel;              /* FRESNEL                        -no_fresnel   */
  int32_t ambient;              /* AMBIENT                        -no_ambient   */
  int32_t direct_illum;         /* DIRECT_ILLUM                   -no_direct    */
  int32_t transmissive_illum;   /* TRANSMISSIVE_ILLUM             -no_transmissive */
  int32_t specular_illum;       /* SPECULAR_ILLUM                 -no_specular  */
  int32_t indirect_illum;       /* INDIRECT_ILLUM                 -no_indirect  */
  int32_t caustic_illum;        /* CAUSTIC_ILLUM                  -no_caustic   */
  int32_t direct_photon_illum;  /* DIRECT_PHOTON_ILLUM            -photon_viz   */
  int32_t fast_global;          /* FAST_GLOBAL                    -fast_global  */
  int32_t irradiance_cache;     /* IRRADIANCE_CACHE               -cache        */
  int32_t shadows;              /* SHADOWS                        -no_shadow    */
  int32_t soft_shadows;         /* SOFT_SHADOWS                   -no_ss        */
  int32_t light_test;           /* LIGHT_TEST                     -lt N         */
  int32_t shadow_test;          /* SHADOW_TEST                    -ss N         */
  int32_t monte_carlo;          /* MONTE_CARLO                    -no_monte     */
  int32_t max_monte_depth;      /* MAX_MONTE_DEPTH                -md N         */
  int32_t recursive_shadows;    /* RECURSIVE_SHADOWS              -no_rs        */
  int32_t distrib_transmissive; /* DISTRIB_TRANSMISSIVE           -no_dt        */
  int32_t transmissive_test;    /* TRANSMISSIVE_TEST              -tt N         */
  int32_t distrib_specular;     /* DISTRIB_SPECULAR               -no_ds        */
  int32_t specular_test;        /* SPECULAR_TEST                  -st N         */
  int32_t depth_of_field;       /* DEPTH_OF_FIELD                 -dof N D R    */
  int32_t dof_test;             /* DOF_TEST                                     */
  int32_t global_photon_count;  /* GLOBAL_PHOTON_COUNT            -global N     */
  int32_t caustic_photon_count; /* CAUSTIC_PHOTON_COUNT           -caustic N    */
  int32_t max_photon_depth;     /* MAX_PHOTON_DEPTH               -pd N         */
  int32_t indirect_test;        /* INDIRECT_TEST                  -it N         */
  int32_t global_estimate_size; /* GLOBAL_ESTIMATE_SIZE           -gs N         */
  int32_t global_filter;        /* GLOBAL_FILTER                  -gf cone K | gauss */
  int32_t caustic_estimate_size;/* CAUSTIC_ESTIMATE_SIZE          -cs N         */
  int32_t caustic_filter;       /* CAUSTIC_FILTER                 -cf cone K | gauss */
  int32_t gpus;                 /* extension: devices of the drop-in CLI (-gpus N); 0/1 = one */
  double ir_air;                /* IR_AIR                         -ir F         */
  double prob_absorb;           /* PROB_ABSORB                    -absorb F     */
  double focus_depth;           /* FOCUS_DEPTH                                  */
  double aperture_radius;       /* APERTURE_RADIUS                              */
  double global_estimate_dist;  /* GLOBAL_ESTIMATE_DIST           -gd F         */
  double caustic_estimate_dist; /* CAUSTIC_ESTIMATE_DIST          -cd F         */
  double filter_const_a;        /* FILTER_CONST_A (0.918)                       */
  double filter_const_b;        /* FILTER_CONST_B (1.953)                       */
  double filter_const_k;        /* FILTER_CONST_K                               */
  uint64_t seed;                /* extension: RNG seed (-seed S); reference RNG is unseeded */
} gi_params;

/* ---- photon record (exchange format, 20 bytes; device layout is SoA) -------- */
typedef struct gi_photon {
  float pos[3];       /* hit point, fp32 (reference: R3Point fp64)            */
  uint8_t rgbe[4];    /* Ward RGBE power (graphics_utils.cpp:50-77)           */
  uint16_t dir;       /* phi*256+theta travel direction (photon_utils.cpp:56) */
  uint16_t flags;     /* reserved (0)                                         */
} gi_photon;

/* ---- EstimateRadiance test-seam query (photon_utils.h:32-35 argument list) ------------- */
typedef struct gi_radiance_query {
  double point[3];
  double normal[3];
  double exact_bounce[3];
  double cos_theta;
  double kd[3];        /* brdf->Diffuse()   */
  double ks[3];        /* brdf->Specular()  */
  double shininess;    /* brdf->Shininess() */
  double max_dist;     /* estimate_dist     */
  int32_t k;           /* estimate_size     */
  int32_t filter;      /* GI_FILTER_*       */
} gi_radiance_query;

typedef struct gi_photon_stats {
  int64_t global_stored, caustic_stored;
  int64_t global_emitted, caustic_emitted;
  /* trace_s: emission rounds + power rescale; kd_s: kd builds and the k-NN kernels' per-photon
   * K-th distance bound pass; irradiance_s: the -cache pass and replication over a device set */
  double total_s, trace_s, kd_s, irradiance_s;
} gi_photon_stats;

/* Counters mirror the -v report of render.cpp:224-255 */
typedef struct gi_render_stats {
  uint64_t screen_rays, shadow_rays, monte_carlo_rays, transmissive_samples;
  uint64_t specular_samples, indirect_samples, caustic_samples;
  uint64_t knn_queries, knn_photons;   /* sum over queries of photons returned */
  uint64_t knn_visited;                /* photons distance-tested by the k-NN search */
  double render_s;                     /* wall time of the render phase       */
  double knn_kernel_ms;                /* summed k-NN kernel time (HIP events) */
  double knn_kernel_launches;
  /* the same split per photon map (0 = global, 1 = caustic) */
  uint64_t knn_map_queries[2], knn_map_photons[2], knn_map_visited[2];
  double knn_map_kernel_ms[2], knn_map_launches[2];
  /* chunk k-NN path, within knn_map_kernel_ms: time and queries of the final fallback kernel
   * (per-lane for K <= 64, query-per-wave for K > 64): the queries neither chunk pass resolved */
  double knn_map_fallback_ms[2];
  uint64_t knn_map_fallback_queries[2];
  /* k-NN launch sequence the last batch ran per map (-1 none): 7 lane-select chunk kernel +
   * per-lane fallback, 8 large-K chunk kernel (+ second chunk pass) + query-per-wave fallback,
   * 3 per-lane, 1 query-per-wave, 0 per-lane with global heaps, 9 irradiance-cache lookup,
   * 10 fixed-radius range estimate (estimate size above the map's photon count) */
  int32_t knn_map_kind[2];
  /* chunk k-NN path: time of the second chunk pass (larger LDS candidate set) and the queries
   * the first pass handed to it (those it did not resolve are in knn_map_fallback_queries) */
  double knn_map_pass2_ms[2];
  uint64_t knn_map_pass2_queries[2];
  /* device sets (gi_create_devices): the slowest and fastest device's render phase and the
   * tile gather onto the first device after the last one finished (0 on one device) */
  double device_render_s_max, device_render_s_min, gather_s;
} gi_render_stats;

typedef struct gi_ctx gi_ctx;

/* ---- host-side flag parsing (drop-in ParseArgs) --------------------------------------- */
void gi_params_default(gi_params *p);
/* returns GI_OK, or GI_ERR_ARG with the reference's message in *err (static storage) */
int gi_parse_args(int argc, char **argv, gi_params *p, const char **scene_path,
                  const char **output_path, int *width, int *height, int *aa,
                  int *real_material, const char **err);

/* ---- context ----------------------------------------------------------------------- */
int gi_create(gi_ctx **out, int hip_device);
/* One context over several HIP devices (SURVEY.md 8(b) gi_create(gi_ctx**, const
 * gi_device_set*); render.cpp:90's thread interleave re-cut as a device shard). Every call on
 * it drives all of them: the scene and photon maps are replicated (photon emission ranges are
 * split across the devices, the maps built once), gi_render_image deals 16x16 output tiles
 * (tx, ty) to device (tx + ty) % count and gathers the tiles onto devices[0] (RCCL send/recv over xGMI when the
 * devices are distinct, else a peer copy). Test seams (gi_*_batch) run on devices[0]. */
#define GI_MAX_DEVICES 64
typedef struct gi_device_set {
  int32_t count;
  int32_t devices[GI_MAX_DEVICES];
} gi_device_set;
int gi_create_devices(gi_ctx **out, const gi_device_set *set);
/* What a context really drives, so that a multi-GPU run can prove it (no reference
 * counterpart: the reference's threads share one host). *ndev = the context's device count;
 * for each (up to max): devices[k] = its HIP ordinal, pci_bus[k] = that device's PCI bus id
 * (hipDeviceAttributePciBusId; -1 if unknown), comm_rank[k] = ncclCommUserRank of its RCCL
 * communicator (-1 without one). *comm_count = ncclCommCount of the first communicator (0 when
 * the set gathers without RCCL: one device, or entries naming the same device). */
int gi_device_info(const gi_ctx *ctx, int max, int *ndev, int *devices, int *pci_bus,
                   int *comm_rank, int *comm_count);
void gi_destroy(gi_ctx *ctx);
const char *gi_last_error(const gi_ctx *ctx);
int gi_set_params(gi_ctx *ctx, const gi_params *p);
/* Progress reports (the reference's PrintProgress calls, io_utils.cpp:257-268): stage 0 =
 * RenderImage, progress = output pixels done / total after each batch (render.cpp:80-87, 201);
 * stage 1 / 2 = the global / caustic map's emission rounds, progress = stored / goal
 * (photonmap.cpp:193-197, 244-248). Called on the thread that made the gi_ call; null = off. */
typedef void (*gi_progress_fn)(int stage, double progress, void *user);
int gi_set_progress(gi_ctx *ctx, gi_progress_fn fn, void *user);
int gi_read_scene(gi_ctx *ctx, const char *path, int real_material);
/* scene summary: nodes, lights, radius, ambient/background */
int gi_scene_info(gi_ctx *ctx, int *nnodes, int *nlights, int *nprims, double *radius);

/* ---- photon maps ---------------------------------------------------------------------- */
int gi_map_photons(gi_ctx *ctx, gi_photon_stats *stats);
/* Replace a photon map with caller photons (kd build + upload); n == 0 disables the map. */
int gi_set_photon_map(gi_ctx *ctx, int map, const gi_photon *photons, int64_t n);
/* Copy a photon map back in storage (emission) order. */
int gi_get_photon_map(gi_ctx *ctx, int map, gi_photon *out, int64_t capacity, int64_t *n);
/* Test seam: the map's kd tree as the k-NN kernels read it (the R3Kdtree the reference builds
 * in R3Kdtree.cpp:1552-1671). nodes: 8 floats per node of the implicit tree (node v = 1 ..
 * 2 * nleaves - 1; {lo.xyz, split}, {hi.xyz, axis bits}); perm: kd-order position -> emission
 * index. Null outputs only report the sizes. */
int gi_get_kd_tree(gi_ctx *ctx, int map, float *nodes, int64_t node_floats, int32_t *perm,
                   int64_t perm_capacity, int32_t *nleaves, int64_t *n);

/* ---- rendering ------------------------------------------------------------------------ */
/* Full frame; rgb8 is W*H*3 bytes row-major with row 0 = image row y=0 (bottom, as R2Image);
 * rgbf (optional) receives the clamped box-filtered colour in [0,1]. */
int gi_render_image(gi_ctx *ctx, int aa, int width, int height, uint8_t *rgb8, float *rgbf,
                    gi_render_stats *stats);
/* Shard: render only the output tiles (tile_px x tile_px pixels; tile column tx, row ty) with
 * (tx + ty) % nshards == shard (a diagonal deal: every run of nshards tiles along a row or a
 * column meets every shard), packed shards in row-major tile order; rgbf is the full W*H*3 image, untouched outside the shard. */
int gi_render_tiles(gi_ctx *ctx, int aa, int width, int height, int tile_px, int shard,
                    int nshards, float *rgbf, gi_render_stats *stats);
/* Shard left on the device (one-process-per-GPU ranks, e.g. torchrun): renders the same tiles
 * as gi_render_tiles and writes them packed into `packed`, a DEVICE pointer on the context's
 * device holding `capacity` pixels: 16 B per pixel of the shard, in the shard's tile order
 * (f32 r, g, b; the u8 r, g, b in the low 24 bits of the fourth word). *npix receives the
 * shard's pixel count (packed == NULL only reports it). Synchronous: the buffer is complete on
 * return. */
int gi_render_tiles_packed(gi_ctx *ctx, int aa, int width, int height, int tile_px, int shard,
                           int nshards, void *packed, int64_t capacity, int64_t *npix,
                           gi_render_stats *stats);
/* Compose the frame from every shard's packed pixels: `packed` is a DEVICE pointer on the
 * context's device to nshards buffers of `stride` pixels (16 B each), shard s at s * stride
 * (the layout of a gather of gi_render_tiles_packed outputs); the caller must have allocated
 * all stride * nshards * 16 bytes (each shard's pixel count must be <= stride, checked).
 * rgb8 / rgbf (host, optional) receive the full image as gi_render_image returns it.
 * Both packed entry points restore the calling thread's current HIP device on return. */
int gi_compose_tiles(gi_ctx *ctx, int width, int height, int tile_px, int nshards,
                     const void *packed, int64_t stride, uint8_t *rgb8, float *rgbf);
/* ---- views from resident photon maps ---------------------------------------------------- */
/* The photon maps, their kd trees and K-th-distance bounds and the -cache irradiance do not
 * depend on the view: after one gi_map_photons a context renders any number of cameras
 * (gi_set_camera + gi_render_image) or caller-made ray batches (gi_render_rays). No reference
 * counterpart: the reference renders the scene file's camera only. */
/* The .scn `camera` command's first ten numbers (R3Scene.cpp camera command;
 * R3Camera(eye, towards, up, xfov, xfov), Q5: yfov = xfov). Raw values as given:
 * towards/up need not be unit or orthogonal, the triad is built as at scene load. */
typedef struct gi_camera { double eye[3], towards[3], up[3], xfov; } gi_camera;
/* The ten numbers the context renders from: the scene file's `camera` line, the default camera
 * of a file without one (R3Scene.cpp:557-566), or the last gi_set_camera, exactly as given
 * (set(get()) changes nothing). GI_ERR_STATE before a scene is read. */
int gi_get_camera(const gi_ctx *ctx, gi_camera *out);
/* Replace the camera (all devices of a device set); everything else the context holds stays.
 * GI_ERR_ARG (camera unchanged) for a non-finite value, a zero towards, an up parallel to
 * towards, or xfov outside (0, pi/2). gi_read_scene resets the camera to the file's. */
int gi_set_camera(gi_ctx *ctx, const gi_camera *cam);

typedef struct gi_ray { double org[3], dir[3]; } gi_ray;   /* dir: unit, used as given */
/* The primary rays gi_render_image(aa, width, height) traces, computed on the device by the
 * render's own camera code: output pixels row-major (row 0 = bottom), within a pixel the 4^aa
 * sub-cells row-major and within a sub-cell the dof_test lens samples; ids (optional) receives
 * each ray's RNG stream id. *n = width * height * 4^aa * dof_test; rays == NULL only reports
 * it, capacity < *n is GI_ERR_ARG. With depth of field the rays are the lens-sampled ones. */
int gi_camera_rays(gi_ctx *ctx, int aa, int width, int height,
                   gi_ray *rays, uint64_t *ids, int64_t capacity, int64_t *n);
/* Render caller-made primary rays (any sensor: panorama, fisheye, orthographic, light-field
 * slice): pixel p (row-major, row 0 = bottom) is the box-filtered mean of rays [p * spp,
 * (p + 1) * spp), each clamped to [0, 1] first, as gi_render_image treats a pixel's sub-cells;
 * same 8-bit truncation. Ray r draws from RNG stream ids[r], or r when ids is NULL. A hit is
 * shaded as seen from its ray's origin (view = normalize(hit - org)); directions are used as
 * given, not renormalised. depth_of_field / dof_test are ignored; every other flag, both
 * photon maps, the counters and device sets behave as in gi_render_image. GI_ERR_ARG for
 * spp < 1, rays == NULL or width * height * spp >= 2^31.
 * Replay: gi_render_rays on gi_camera_rays' output with spp = 4^aa returns gi_render_image's
 * image and counters bit for bit when depth of field is off. With it on, the camera path shades
 * from the eye (not the lens sample) and has advanced the sample's stream past the lens draws,
 * so the replay differs; that is accepted. */
int gi_render_rays(gi_ctx *ctx, int width, int height, int spp,
                   const gi_ray *rays, const uint64_t *ids /* may be NULL */,
                   uint8_t *rgb8, float *rgbf, gi_render_stats *stats);

/* Quantise a full float image like RenderImage's SetPixelRGB (truncate 255*c). */
int gi_quantize(int width, int height, const float *rgbf, uint8_t *rgb8);

/* ---- feature planes and denoise pass -------------------------------------------------- */
/* Per-pixel geometry planes of a frame and an edge-avoiding a-trous filter guided by them
 * (DESIGN.md "Feature planes and denoise pass"). No reference counterpart: the reference
 * writes the noisy frame only. On a device set these calls run on devices[0], as the test
 * seams do. */
typedef struct gi_material { double ka[3], kd[3], ks[3], kt[3], e[3], n, ir; } gi_material;
/* The scene's materials as the device holds them (after -real normalisation), indexed by the
 * `material` value gi_intersect_batch returns. *n = their number; out == NULL only reports it,
 * capacity < *n is GI_ERR_ARG. GI_ERR_STATE before a scene is read. No reference counterpart. */
int gi_get_materials(gi_ctx *ctx, gi_material *out, int32_t capacity, int32_t *n);

typedef struct gi_pixel_features {      /* 32 bytes */
  float normal[3]; float depth; float albedo[3]; float coverage;
} gi_pixel_features;
/* Planes of the frame gi_render_image(aa, width, height) renders: same primary rays as
 * gi_camera_rays (lens-sampled under -dof), output pixels row-major, row 0 = bottom. Of a
 * pixel's S samples, over those that hit, in sample order, in fp64, each value rounded to
 * float32 once: coverage = hits / S, normal = mean hit normal (as gi_intersect_batch returns
 * it: not flipped towards the viewer, not renormalised), depth = mean distance origin -> hit,
 * albedo = mean kd of the hit material; all 0 when no sample hits. Needs a scene, not the
 * photon maps (GI_ERR_STATE before gi_read_scene). No reference counterpart. */
int gi_camera_features(gi_ctx *ctx, int aa, int width, int height, gi_pixel_features *out);
/* ... and of a caller-made ray batch, pixel p = rays [p*spp, (p+1)*spp) as in gi_render_rays.
 * GI_ERR_ARG for spp < 1, null buffers or width * height * spp >= 2^31. No reference
 * counterpart. */
int gi_ray_features(gi_ctx *ctx, int width, int height, int spp, const gi_ray *rays,
                    gi_pixel_features *out);

typedef struct gi_denoise_params {
  int32_t levels;             /* 1..8 a-trous levels, step 2^l            default 5    */
  int32_t normal_power_log2;  /* 0..8: normal weight = max(0,n.n)^(2^e)   default 5    */
  double sigma_color;         /* halved at every level                    default 1.0  */
  double sigma_depth;         /* relative depth difference                default 0.05 */
  double sigma_albedo;        /*                                          default 0.1  */
} gi_denoise_params;
void gi_denoise_params_default(gi_denoise_params *p);
/* Edge-avoiding a-trous wavelet filter (Dammertz et al. 2010; Lorentzian stopping functions, so
 * that every operation is exactly rounded) of a frame by its planes. rgbf: W*H*3 floats as
 * gi_render_image / gi_render_rays return them; feat: the frame's W*H planes (depth > 0 where
 * coverage > 0). out_rgbf (W*H*3 floats) and out_rgb8 = gi_quantize of out_rgbf: either may
 * be NULL, not both. p == NULL: defaults. kernel_ms (optional): summed HIP-event time of the
 * filter launches. GI_ERR_ARG for null buffers, width or height < 1, width * height >= 2^31,
 * levels or normal_power_log2 out of range, or a sigma that is not finite and positive. Needs
 * only a context (no scene). Runs on the context's first device. No reference counterpart. */
int gi_denoise(gi_ctx *ctx, int width, int height, const float *rgbf,
               const gi_pixel_features *feat, const gi_denoise_params *p,
               float *out_rgbf, uint8_t *out_rgb8, double *kernel_ms);

/* ---- radiance frames, accumulation over passes, tone map -------------------------------- */
/* gi_render_image / gi_render_rays clamp every sample to [0, 1] before the box filter (the
 * reference's 8-bit output path) and return only the result. These calls return what the clamp
 * sees (DESIGN.md "Radiance frames, accumulation and tone map"). No reference counterpart.
 * All of them are for contexts over one device: on a device set (gi_create_devices) the renders
 * and the accumulator calls return GI_ERR_UNSUPPORTED (the tile gather packs 16 B per pixel).
 *
 * A pixel has S samples: S = 4^aa sub-cells of a camera frame (each the mean of its dof_test lens
 * samples), S = spp rays of a ray batch. Sample s_j is the fp64 value gi_render_image has before
 * its clamp. With bw = 1.0 / af / af (af = 2^aa) or 1.0 / spp, sums in sample order in fp64:
 *   m = bw * sum_j s_j,  M2 = sum_j (s_j - m)^2,
 *   mean = (float)m,  variance = (float)(M2 / (S - 1) / S), the variance of the mean (0 for S = 1).
 * mean, variance: W*H*3 floats, rows from the bottom; samples: W*H*S*3 doubles, pixel-major,
 * then sample, then r, g, b. Any of the three may be NULL, not all. Pipeline, batches, counters
 * and argument checks are gi_render_image's / gi_render_rays' (aa <= 15 here). */
int gi_render_radiance(gi_ctx *ctx, int aa, int width, int height, float *mean, float *variance,
                       double *samples, gi_render_stats *stats);
int gi_render_rays_radiance(gi_ctx *ctx, int width, int height, int spp, const gi_ray *rays,
                            const uint64_t *ids /* may be NULL */, float *mean, float *variance,
                            double *samples, gi_render_stats *stats);
/* Accumulator, on the device, one per context: per pixel and channel a running fp64 mean mu and
 * sum of squared deviations A, and per pixel one int64 sample count N (written n_p where pixels
 * differ). gi_accum_reset sizes and empties it (every N = 0). gi_accum_add_image /
 * gi_accum_add_rays render one pass of the reset's width x height under the context's current
 * parameters and fold its (S, m, M2) into every pixel, once, after the render has completed; a
 * pixel with N = 0 takes the pass as is, the others by
 *   d = m - mu,  N' = N + S,  mu' = mu + (d * S) / N',  A' = (A + M2) + ((d * d) * (N * S)) / N'.
 * (N, S and N' are converted to double once each; N * S is the product of the two doubles.)
 * The caller decorrelates the passes: for camera passes change `seed` with gi_set_params between
 * them (gi_set_params keeps the photon maps, their kd trees and the -cache irradiance: a second
 * render under another seed is an independent estimate from the same maps); for ray passes give
 * other ids. gi_accum_get (every output optional), each pixel under its own N: mean =
 * (float)mu, variance = (float)(A / (N - 1) / N) (0 where N < 2), *nsamples = the smallest N of
 * the frame (every pixel's N while only whole-frame passes were added), *noise = the mean over
 * the pixels of e = sqrt(v) / (Y + 0.01) with Y = 0.2126 mu_r + 0.7152 mu_g + 0.0722 mu_b and v =
 * 0.2126^2 v_r + 0.7152^2 v_g + 0.0722^2 v_b (v_c the unrounded A / (N - 1) / N): the relative
 * standard error of luminance (e = 0 where N < 2), summed in a fixed order (blocks of 256 pixels
 * by a tree, then block by block), so the same accumulator always reports the same bits.
 * GI_ERR_STATE before a reset; a pass always has the reset's size (a ray pass takes width *
 * height * spp rays). */
int gi_accum_reset(gi_ctx *ctx, int width, int height);
int gi_accum_add_image(gi_ctx *ctx, int aa, gi_render_stats *stats);
int gi_accum_add_rays(gi_ctx *ctx, int spp, const gi_ray *rays, const uint64_t *ids,
                      gi_render_stats *stats);
int gi_accum_get(gi_ctx *ctx, float *mean, float *variance, int64_t *nsamples, double *noise);
/* counts: W*H int64, rows from the bottom (optional); *total = sum of n_p (optional) */
int gi_accum_get_counts(gi_ctx *ctx, int64_t *counts, int64_t *total);

/* ---- light-path layers of radiance frames and passes --------------------------------------- */
/* A primary sample's radiance is the sequential fp64 sum of its path bases and photon-map
 * estimates (DESIGN.md "Light-path layers"). These calls return that sum split into the five
 * groups the reduction visits, each a sequential fp64 sum from +0 in the reduction's own order,
 * with the entries it skips (empty query slots, indirect paths without a stored base) skipped:
 *   SURFACE   the primary's own base: ambient, emission and direct light at the primary hit, or
 *             the background on a miss;
 *   SPECULAR  the bases of its transmissive and specular sample paths (Monte Carlo paths), then
 *             their appended queries of the global list, then those of the caustic list:
 *             everything that reaches the pixel through a Monte Carlo path, those paths' indirect
 *             sub-paths and caustic queries included (what a mirror or glass shows);
 *   INDIRECT  the bases of its indirect sample paths, then their global-map queries;
 *   GLOBAL    the primary's own global-map query (-photon_viz, -fast_global; else zero);
 *   CAUSTIC   the primary's own caustic-map query.
 * A layer's sample is formed like a radiance sample (the sum over the dof_test lens primaries,
 * then / dof_test), and its m, M2, mean and variance are gi_render_radiance's definitions applied
 * to that layer's samples. Plane GI_LAYER_TOTAL is gi_render_radiance's own output, bit for bit.
 * The layers of a sample add up to the total only up to the rounding of two summation orders
 * (relative 2 (n - 1) 2^-53 for n non-negative terms). A layer's variance is that layer's own: the
 * layers of one sample are correlated, so the variances do not add up to the total's.
 * No reference counterpart. */
enum { GI_LAYER_SURFACE = 0, GI_LAYER_SPECULAR = 1, GI_LAYER_INDIRECT = 2,
       GI_LAYER_GLOBAL = 3, GI_LAYER_CAUSTIC = 4, GI_LAYER_COUNT = 5,
       GI_LAYER_TOTAL = 5 /* plane index of the undivided frame */ };
/* gi_render_radiance / gi_render_rays_radiance with GI_LAYER_COUNT + 1 planes per output,
 * layer-major: mean, variance 6*W*H*3 floats, samples 6*W*H*S*3 doubles, each plane laid out as
 * there. Any of the three may be NULL, not all. Counters, batches, argument checks and errors are
 * those calls'. */
int gi_render_layers(gi_ctx *ctx, int aa, int width, int height, float *mean, float *variance,
                     double *samples, gi_render_stats *stats);
int gi_render_rays_layers(gi_ctx *ctx, int width, int height, int spp, const gi_ray *rays,
                          const uint64_t *ids /* may be NULL */, float *mean, float *variance,
                          double *samples, gi_render_stats *stats);
/* One pass. The total is folded into ctx's accumulator exactly as gi_accum_add_image /
 * gi_accum_add_rays do; layer l's (S, m_l, M2_l) is folded by the same update into the
 * accumulator of layers[l] (a NULL entry drops that layer), so gi_accum_get, gi_accum_denoise,
 * gi_accum_export and gi_accum_merge* serve a layer like any accumulator. A layer context is a
 * one-device context on ctx's device whose accumulator (gi_accum_reset / gi_accum_import; it
 * needs no scene) has the size of ctx's; it is not ctx and is listed once. GI_ERR_UNSUPPORTED when
 * ctx is a device set, GI_ERR_STATE when ctx or a layer context has no accumulator, GI_ERR_ARG
 * for a null `layers` or any other layer context, all before anything is rendered: a refused call
 * changes nothing. Otherwise as gi_accum_add_image / gi_accum_add_rays.
 * Accepted limits: whole-frame passes only (no layered gi_accum_add_tiles, adaptive or
 * progressive passes); gi_accum_reproject knows nothing of layers (a caller may reproject the
 * contexts of the diffuse layers and reset the SPECULAR one). */
int gi_accum_add_image_layers(gi_ctx *ctx, int aa, gi_ctx *const layers[GI_LAYER_COUNT],
                              gi_render_stats *stats);
int gi_accum_add_rays_layers(gi_ctx *ctx, int spp, const gi_ray *rays, const uint64_t *ids,
                             gi_ctx *const layers[GI_LAYER_COUNT], gi_render_stats *stats);
/* Diagnostics: the summed HIP-event time of the layer reduction's kernel alone. on != 0 zeroes
 * the sum and makes every later layered render time the kernel (one event pair and one wait per
 * batch); on == 0 stops. *ms (optional) receives the sum so far, before it is zeroed. */
int gi_layers_timing(gi_ctx *ctx, int on, double *ms);

/* ---- accumulator state: export, import and merge ------------------------------------------ */
/* The state of a W x H accumulator (DESIGN.md "Accumulator state"), the device's own bits with no
 * rounding:
 *   state   W*H*6 doubles, pixel-major, rows from the bottom: {mu_r, mu_g, mu_b, A_r, A_g, A_b}
 *   counts  W*H int64 n_p
 * Packed state: one buffer of W*H*56 bytes, the state plane (48 W H bytes) and then the counts
 * plane (8 W H bytes).
 * The fold of state b into state a, per pixel and channel in fp64, each step one IEEE operation
 * in the order written:
 *   n_b == 0:  a unchanged (bit for bit)
 *   n_a == 0:  a = b (bit copy of mu and A; n = n_b)
 *   else:      Na = (double)n_a, Nb = (double)n_b, N1 = (double)(n_a + n_b), NS = Na * Nb
 *              d = mu_b - mu_a
 *              mu' = mu_a + (d * Nb) / N1
 *              A'  = (A_a + A_b) + ((d * d) * NS) / N1
 *              n'  = n_a + n_b
 * This is the pass update above with S = n_b, m = mu_b, M2 = A_b, so folding the state of a
 * context that holds one pass equals adding that pass. K states are folded as ((a + b_0) + b_1)
 * + ... in the given order; the fold is not associative in bits, so the order is part of the
 * result. All six calls: GI_ERR_UNSUPPORTED on a device set, GI_ERR_STATE where they need an
 * accumulator (all but gi_accum_import) and there is none. After an import or a merge every pixel
 * is under its own count, as after gi_accum_reproject, and every other accumulator call behaves
 * as on any accumulator with those bits. No reference counterpart.
 *
 * gi_accum_export: the state to host buffers; either may be NULL, not both.
 * gi_accum_import: sizes the accumulator like gi_accum_reset(width, height) and replaces it by
 * the host state; needs only a context (no scene, no earlier reset). A negative count is
 * GI_ERR_ARG and leaves the accumulator as it was. mu and A are not scanned: a NaN or Inf in them
 * is taken as it is.
 * gi_accum_merge: folds one host state into the accumulator. GI_ERR_ARG (accumulator unchanged)
 * for a width x height other than the accumulator's or a negative count. */
int gi_accum_export(gi_ctx *ctx, double *state, int64_t *counts);
int gi_accum_import(gi_ctx *ctx, int width, int height, const double *state, const int64_t *counts);
int gi_accum_merge(gi_ctx *ctx, int width, int height, const double *state, const int64_t *counts);
/* The packed state written to `packed`, a DEVICE pointer on the context's device holding
 * capacity_bytes; *bytes (optional with a buffer) = W*H*56, and packed == NULL only reports it. A
 * capacity below that is GI_ERR_ARG. Synchronous; restores the calling thread's current HIP
 * device, like the other packed entry points. */
int gi_accum_export_packed(gi_ctx *ctx, void *packed /* DEVICE */, int64_t capacity_bytes,
                           int64_t *bytes);
/* nstates >= 1 packed states, state s at packed + s * stride_bytes in DEVICE memory of the
 * context's device (the layout of a gather of gi_accum_export_packed outputs), folded into the
 * accumulator in the order s = 0 .. nstates - 1 by one launch that reads the accumulator once,
 * each state once, and writes each pixel once. stride_bytes >= W*H*56; packed and stride_bytes
 * are multiples of 8, so that every plane is aligned for its doubles and int64 (else GI_ERR_ARG):
 * padding after a state is allowed. The caller guarantees nstates * stride_bytes
 * bytes. The device counts are not scanned: a negative one is folded as it is. kernel_ms
 * (optional): HIP-event time of the launch. Synchronous; restores the current HIP device. */
int gi_accum_merge_packed(gi_ctx *ctx, int nstates, const void *packed /* DEVICE */,
                          int64_t stride_bytes, double *kernel_ms /* optional */);
/* The accumulator of src folded into dst's: two one-device contexts (on one device or on two)
 * whose accumulators have the same size (else GI_ERR_ARG; dst == src is GI_ERR_ARG). The source's
 * state is copied to the destination's device and folded there; src is left bit for bit
 * unchanged. */
int gi_accum_merge_from(gi_ctx *dst, gi_ctx *src, double *kernel_ms /* optional */);

/* ---- progressive photon-map passes (Knaus & Zwicker 2011, the probabilistic form) ------------
 * Every pass traces fresh photon maps under its own seed, estimates with a fixed radius that
 * shrinks by a global schedule, and is averaged by the accumulator (DESIGN.md "Fixed-radius
 * estimate and progressive passes"). No reference counterpart; tests/progressive_ref.py restates
 * the schedule. */
typedef struct gi_progressive_params {
  double alpha;           /* in (0, 1); default 0.7 */
  double global_radius;   /* r_0 > 0 and finite; 0 = the context's global_estimate_dist */
  double caustic_radius;  /* likewise, caustic_estimate_dist */
} gi_progressive_params;
void gi_progressive_params_default(gi_progressive_params *p);
/* The radius of pass `pass` (0-based). Host only, one IEEE operation per step:
 *   r2 = r0 * r0; for j = 1 .. pass: r2 = (r2 * ((double)j + alpha)) / ((double)j + 1.0);
 *   return sqrt(r2).
 * NaN for r0 <= 0 or not finite, alpha outside (0, 1), pass < 0 or pass >= 2^20. */
double gi_progressive_radius(double r0, double alpha, int64_t pass);
/* Pass `pass`, defined as this sequence of calls, bit for bit: with P the context's parameters
 * and Q = P with seed = P.seed + pass, both estimate sizes GI_ESTIMATE_ALL and both estimate
 * distances gi_progressive_radius(r_0, alpha, pass):
 *   gi_set_params(Q); gi_map_photons (pstats); gi_accum_add_image(aa) (stats); gi_set_params(P).
 * The maps stay the pass's. On failure P is restored and the accumulator is as the failed step
 * left it. The schedule depends on the pass index alone, so a saved accumulator resumes with the
 * index it stopped at. GI_ERR_UNSUPPORTED on a device set; GI_ERR_STATE before a scene or before
 * gi_accum_reset / gi_accum_import; GI_ERR_ARG for a bad parameter, a pass out of range, or
 * irradiance_cache set (the cache bakes a K-estimate into the map). A refused call changes
 * nothing. */
int gi_accum_add_progressive(gi_ctx *ctx, int aa, int64_t pass,
                             const gi_progressive_params *p /* NULL: defaults */,
                             gi_photon_stats *pstats /* optional */,
                             gi_render_stats *stats /* optional */);

/* ---- adaptive passes: refine only the noisy tiles of the accumulator --------------------- */
/* The accumulator's frame is cut into tiles of tile_px x tile_px pixels: tiles_x = ceil(W /
 * tile_px), tiles_y likewise, tile t = ty * tiles_x + tx with ty = 0 at the bottom; the tiles of
 * the last column and row are clipped by the frame. No reference counterpart. One device only:
 * GI_ERR_UNSUPPORTED on a device set, GI_ERR_STATE before gi_accum_reset.
 *
 * Tile error. A tile has T * T slots (T = tile_px), slot q = y_in_tile * T + x_in_tile. A slot
 * inside the frame holds its pixel's e as gi_accum_get defines it under the pixel's own n_p (0
 * where n_p < 2); a slot outside holds 0. In fp64: x[l] (l = 0 .. 63) = the sum of the slots
 * q = l, l + 64, ... in ascending q, starting from 0; then x[l] += x[l + h] for l < h, for h = 32,
 * 16, .., 1; tile_error = x[0] / (pixels of the tile inside the frame). n_min = the smallest n_p
 * of those pixels.
 * Selection. below_max = (max_samples == 0 or n_min < max_samples); by_error = (tile_error >
 * threshold and below_max); core = (n_min < min_samples or by_error); dilated = (dilate and not
 * core and below_max and one of the tile's up to 8 neighbours is by_error); active = core or
 * dilated. */
typedef struct gi_adaptive_params {
  int32_t tile_px;      /* 4..64, default 8 */
  int32_t min_samples;  /* >= 0: a tile whose smallest n_p is below this is always active; default 8 */
  int32_t max_samples;  /* 0 = none; a tile whose smallest n_p is >= this is never active by its error */
  int32_t dilate;       /* 0 or 1, default 1 */
  double threshold;     /* finite, >= 0; default 0.02 */
} gi_adaptive_params;
void gi_adaptive_params_default(gi_adaptive_params *p);
/* The selection of the accumulator as it stands. mask (optional): one byte per tile, 1 = active;
 * tile_error (optional): one double per tile; *active_tiles, *active_pixels (optional): the
 * active tiles and the pixels inside the frame they hold. GI_ERR_ARG for a null p, tile_px
 * outside 4..64, a negative min_samples or max_samples, dilate not 0 or 1, or a threshold that
 * is negative or not finite. Needs no scene. */
int gi_accum_select(gi_ctx *ctx, const gi_adaptive_params *p, uint8_t *mask /* tiles, optional */,
                    double *tile_error /* tiles, optional */, int64_t *active_tiles,
                    int64_t *active_pixels);
/* One camera pass (as gi_accum_add_image: current parameters, -dof lens samples) over the pixels
 * of the tiles with mask[t] != 0, in tile order and row-major inside a tile, folded into those
 * pixels only, once, after the render has completed; every other pixel keeps mu, A and n_p bit
 * for bit. A sample's RNG stream is keyed by its place in the frame, not in the pass, so a pixel
 * gets the samples a whole-frame pass under the same seed gives it. The counters are those of
 * the pixels rendered (screen_rays: those of their *active_pixels * 4^aa * dof_test primary rays
 * that hit the scene, as in every render). An empty mask returns
 * GI_OK with *active_pixels = 0 and zeroed stats and launches nothing. GI_ERR_ARG for tile_px
 * outside 4..64, a null mask or aa outside 0..15. */
int gi_accum_add_tiles(gi_ctx *ctx, int aa, int tile_px, const uint8_t *mask,
                       int64_t *active_pixels, gi_render_stats *stats);
/* gi_accum_select + gi_accum_add_tiles under the same parameters; mask (optional) receives the
 * selection. Errors as those two. */
int gi_accum_add_adaptive(gi_ctx *ctx, int aa, const gi_adaptive_params *p, uint8_t *mask,
                          int64_t *active_pixels, gi_render_stats *stats);
/* ---- variance-guided denoise of radiance frames and of the accumulator --------------------- */
/* An a-trous filter like gi_denoise whose colour stop is each pixel's own standard error instead
 * of a fixed sigma: it takes unclamped radiance with its variance of the mean, filters a noisy
 * pixel widely and a converged one barely, and returns the variance that is left (DESIGN.md
 * "Variance-guided denoise"; tests/vdenoise_ref.py restates it and the device equals it bit for
 * bit). No reference counterpart. fp64 on float32 inputs, one IEEE operation per step in the
 * order written, only + - * / max.
 *
 * Inputs: colour c (W*H*3 floats), the channels' variances of the mean (W*H*3 floats, >= 0) and
 * the frame's planes. Per pixel v = (float)(0.2126^2 v_r + 0.7152^2 v_g + 0.0722^2 v_b), each
 * squared weight one product, summed left to right. For level l = 0 .. levels-1, s = 2^l:
 *   Y(c) = 0.2126 r + 0.7152 g + 0.0722 b, summed left to right;
 *   g_p  = sum h3 v_q / sum h3 over q = p + (i, j), j = -1..1 outer, i = -1..1 inner, inside the
 *          image, h3 = k3[|i|] k3[|j|], k3 = {1/2, 1/4};
 *   il_p = 1 / (sigma_lum^2 g_p + variance_floor)   (g_p, il_p stay fp64);
 *   taps q = p + s (i, j), j = -2..2 outer, i = -2..2 inner, inside the image, h = k[|i|] k[|j|],
 *   k = {3/8, 1/4, 1/16}; covered means coverage > 0;
 *     centre tap: w = h;   exactly one of p, q covered: the tap is skipped;
 *     neither covered: w = h / (1 + xl);
 *     both covered:    w = ((h m) zz) / (((1 + xl) (zz + dz dz)) (1 + xa));
 *     xl = (dY dY) il_p, dY = Y(c_p) - Y(c_q);  m = max(0, n_p . n_q) squared normal_power_log2
 *     times;  dz = z_p - z_q, zs = z_p + z_q, zz = sigma_depth^2 (zs zs);  xa = |a_p - a_q|^2
 *     (summed r, g, b) * isa2, isa2 = 1 / (sigma_albedo sigma_albedo);
 *   c'_p = sum w c_q / sum w per channel,  v'_p = sum (w w) v_q / ((sum w) (sum w)), both rounded
 *   to float32; the next level reads the rounded values. sigma_lum is not halved per level: the
 *   variance shrinks instead. sum w >= 9/64.
 * Accepted limits: a pixel of variance 0 (a single sample, or clamped by the caller) counts as
 * converged and is barely filtered; the inputs are not scanned for NaN / Inf or negative
 * variances; no albedo demodulation (albedo is per material here and the albedo stop already
 * separates materials); one device. */
typedef struct gi_vdenoise_params {
  int32_t levels;             /* 1..8 a-trous levels, step 2^l            default 5    */
  int32_t normal_power_log2;  /* 0..8: normal weight = max(0,n.n)^(2^e)   default 5    */
  double sigma_lum;           /* luminance stop, in standard errors       default 4.0  */
  double sigma_depth;         /* relative depth difference                default 0.05 */
  double sigma_albedo;        /*                                          default 0.1  */
  double variance_floor;      /* added to sigma_lum^2 g                   default 1e-6 */
} gi_vdenoise_params;
void gi_vdenoise_params_default(gi_vdenoise_params *p);
/* The filter of a frame given by the caller: mean, variance as gi_render_radiance / gi_accum_get
 * return them. out_mean (W*H*3 floats) and out_variance_lum (W*H floats, the filtered luminance
 * variance): either may be NULL, not both. p == NULL: defaults. kernel_ms (optional): summed
 * HIP-event time of the level launches. GI_ERR_ARG for null buffers, width or height < 1, width *
 * height >= 2^31, levels or normal_power_log2 out of range, or a sigma or variance_floor that is
 * not finite and positive. Needs only a context (no scene); on a device set it runs on the first
 * device. */
int gi_denoise_radiance(gi_ctx *ctx, int width, int height, const float *mean,
                        const float *variance, const gi_pixel_features *feat,
                        const gi_vdenoise_params *p /* NULL: defaults */, float *out_mean,
                        float *out_variance_lum, double *kernel_ms);
/* The filter of the accumulator as it stands, read on the device: c = (float)mu, v_c = (float)(A /
 * (N - 1) / N) under the pixel's own N, exactly what gi_accum_get returns, so the result equals
 * gi_denoise_radiance of gi_accum_get's mean and variance bit for bit. feat: the planes of the
 * accumulator's W x H frame. The accumulator is left bit for bit unchanged. GI_ERR_STATE before
 * gi_accum_reset and while the smallest per-pixel count is < 2 (no variance yet);
 * GI_ERR_UNSUPPORTED on a device set; GI_ERR_ARG as above. */
int gi_accum_denoise(gi_ctx *ctx, const gi_pixel_features *feat, const gi_vdenoise_params *p,
                     float *out_mean, float *out_variance_lum, double *kernel_ms);

/* ---- reprojection across views: the accumulator carried into a new camera ------------------- */
/* The pinhole frame the device renders from: the four vectors the host puts into the render's
 * camera block (render.cpp:67-77) for the current camera and the current focus_depth, with the
 * same bits: far_org = eye + towards * focus_depth, far_right = right * tan(xfov) * focus_depth,
 * far_up = up * tan(yfov) * focus_depth over the camera's triad. The ray through (dx, dy) in
 * [-1, 1]^2 is normalize(((far_org + far_right * dx) + far_up * dy) - eye). A caller saves the view
 * before gi_set_camera to name the previous camera later. GI_ERR_STATE before a scene is read.
 * No reference counterpart. */
typedef struct gi_view { double eye[3], far_org[3], far_right[3], far_up[3]; } gi_view;
int gi_get_view(const gi_ctx *ctx, gi_view *out);

/* gi_accum_reproject. The accumulator holds W x H pixels seen from prev_view, prev_feat holds the
 * planes of that frame and cur_feat those of the same W x H frame under the context's current
 * camera. Afterwards the accumulator holds, at every pixel of the current frame, the history found
 * for it: mu, A and n_p; a pixel with no history has all three zero, exactly as after
 * gi_accum_reset, and later gi_accum_add_image / gi_accum_add_tiles / gi_accum_add_adaptive fold
 * onto it under each pixel's own count. (Lambertian radiance does not depend on the view: the
 * samples paid for in one view serve the next.) tests/reproject_ref.py restates the definition and
 * the device equals it bit for bit. No reference counterpart.
 *
 * fp64 on the given values (float32 plane values are widened once), one IEEE operation per step in
 * the order written, only + - * / sqrt floor and comparisons; sums and dot products run left to
 * right over x, y, z or r, g, b; len(a) = sqrt(a . a). For pixel p = (x, y) of the current frame,
 * subscript 1 for gi_get_view now and 0 for prev_view, planes n (normal), z (depth), a (albedo):
 *  1. coverage_p = 0: no history.
 *  2. dx = (2x + 1 - W) / W, dy = (2y + 1 - H) / H (the pixel centre),
 *     D = ((far_org1 + far_right1 * dx) + far_up1 * dy) - eye1, d = D / len(D) (D when len is 0).
 *  3. X = eye1 + d * z_p.
 *  4. v = X - eye0, G = far_org0 - eye0, a = (v . G) / (G . G); a <= 0: no history.
 *     sx = ((v . far_right0) / (far_right0 . far_right0)) / a, sy likewise with far_up0;
 *     u = ((sx + 1) * W) * 0.5 - 0.5, t = ((sy + 1) * H) * 0.5 - 0.5;
 *     x0 = floor(u), fx = u - x0, y0 = floor(t), fy = t - y0; r = len(v).
 *  5. taps q = (x0 + i, y0 + j), j = 0, 1 outer, i = 0, 1 inner, weight
 *     h = (i ? fx : 1 - fx) * (j ? fy : 1 - fy). A tap counts when it lies inside the image,
 *     h >= 2^-10, n_q >= 2, the previous coverage_q > 0, |r - z_q| <= depth_tol * r,
 *     c = n_p . n_q > 0 and c * c >= ((normal_min * normal_min) * (n_p . n_p)) * (n_q . n_q), and
 *     |a_p - a_q|^2 <= albedo_tol * albedo_tol.
 *  6. no tap counts: no history.
 *  7. otherwise, sums from 0 over the counting taps in tap order: hs = sum h; per channel
 *     mu' = (sum h * mu_q) / hs, s2 = (sum h * (A_q / (n_q - 1))) / hs;
 *     n' = min(min_q n_q, max_history), A' = s2 * (n' - 1).
 * The carried per-sample variance is the taps' weighted mean, not sum h^2 (interpolated samples
 * are correlated: the conservative choice); the count is the smallest tap count, so a pixel never
 * claims more history than its least-sampled source; the 2^-10 floor keeps a neighbour at weight
 * ~1e-16 from dragging n' down when the camera did not move.
 * stats (optional): kept_pixels + reset_pixels = W * H, kept_samples = sum n'. kernel_ms
 * (optional): HIP-event time of the kernel. GI_ERR_UNSUPPORTED on a device set; GI_ERR_STATE before
 * gi_accum_reset or before a scene is read; GI_ERR_ARG for a null view or planes, max_history < 2,
 * a tolerance that is negative or not finite, or normal_min outside [0, 1]. A refused call leaves
 * the accumulator as it was.
 * Accepted limits: view-dependent radiance (specular lobes, what a mirror or glass shows) is
 * carried as if it were diffuse, bounded by max_history; depth is the mean distance over a pixel's
 * samples and the point is placed on the centre ray; camera frames only; one device. */
typedef struct gi_reproject_params {
  int64_t max_history;   /* >= 2: cap of a carried count;              default 32   */
  double depth_tol;      /* relative, finite, >= 0;                    default 0.02 */
  double normal_min;     /* cosine in [0, 1];                          default 0.9  */
  double albedo_tol;     /* finite, >= 0;                              default 0.05 */
} gi_reproject_params;
void gi_reproject_params_default(gi_reproject_params *p);
typedef struct gi_reproject_stats { int64_t kept_pixels, reset_pixels, kept_samples; } gi_reproject_stats;
int gi_accum_reproject(gi_ctx *ctx, const gi_view *prev_view,
                       const gi_pixel_features *prev_feat, const gi_pixel_features *cur_feat,
                       const gi_reproject_params *p /* NULL: defaults */,
                       gi_reproject_stats *stats /* optional */, double *kernel_ms /* optional */);

/* Tone map of a radiance frame (W*H*3 floats), per channel in fp64: x = exposure * c;
 * y = x * (1 + x / (white * white)) / (1 + x) when white > 0 (extended Reinhard: `white` maps to
 * 1), y = x when white == 0; clamped to [0, 1], rounded to float32. Linear output, as the
 * reference writes (no gamma). out_rgbf and out_rgb8 = gi_quantize of out_rgbf: either may be
 * NULL, not both. GI_ERR_ARG for an exposure that is not finite and positive, a white that is
 * negative or not finite, null buffers or a bad size. Needs only a context; runs on its first
 * device (also on a device set). */
int gi_tonemap(gi_ctx *ctx, int width, int height, const float *radiance, double exposure,
               double white, float *out_rgbf, uint8_t *out_rgb8);

/* ---- test seams ----------------------------------------------------------------------- */
/* n <= 2^26 queries per call (GI_ERR_ARG above). */
int gi_estimate_radiance_batch(gi_ctx *ctx, int map, int64_t n, const gi_radiance_query *q,
                               double *rgb_out, int32_t *nfound, float *max_d2);
int gi_knn_batch(gi_ctx *ctx, int map, int64_t n, const double *points, int k, double max_dist,
                 int32_t *idx_out, float *d2_out, int32_t *nfound);
/* Diagnostics: time the k-NN estimate kernel over n resident queries (Morton-ordered as in
 * rendering; mode 0 radiance, 1 irradiance, 2 list) for `iters` launches with the given
 * kernel (-1 = default; else a GI_KNN_KERNEL kind of gi_host.cpp run_knn). Uses the context's
 * estimate size / distance / filter for `map`. Outputs average ms per launch and the
 * photons found / visited per query. No reference counterpart (measurement only). */
int gi_knn_bench(gi_ctx *ctx, int map, int64_t n, const double *points, const double *normals,
                 const int32_t *materials, int mode, int kernel, int iters, double *ms_per_launch,
                 double *found_per_query, double *visited_per_query);
/* Diagnostics: time the radiance reduction, the accumulator merge and the noise reduction on a
 * synthetic width x height frame of 4^aa samples per pixel (dof_test 1), each launch between two
 * HIP events: the median of `reps` launches after `warmup` ones, in ms (outputs optional). Needs
 * only a context; leaves its accumulator alone. No reference counterpart (measurement only). */
int gi_radiance_bench(gi_ctx *ctx, int aa, int width, int height, int warmup, int reps,
                      double *reduce_ms, double *merge_ms, double *noise_ms);
/* Diagnostics: the adaptive passes' kernels on a synthetic width x height frame, timed as in
 * gi_radiance_bench (outputs optional): the tile error and selection kernels together, the fold
 * of a masked pass over a checkerboard of tiles (half of them active) and the whole-frame fold.
 * Needs only a context; leaves its accumulator alone. No reference counterpart. */
int gi_adaptive_bench(gi_ctx *ctx, int width, int height, int tile_px, int warmup, int reps,
                      double *select_ms, double *masked_merge_ms, double *merge_ms);
int gi_intersect_batch(gi_ctx *ctx, int64_t n, const double *org, const double *dir,
                       int32_t *hit, double *t, double *point, double *normal, int32_t *material);
/* Test seam: gi_intersect_batch through a chosen instance of the scene walk. hint: per ray, the
 * triangle the ray leaves from (an index as `tri` returns it; the walk tests it first), -1 for
 * none; NULL = every ray -1. tri: the triangle hit, an index into the loaded scene's triangles in
 * loading order (triangle shapes and mesh triangles, element by element; mesh triangles in the
 * order of the mesh's hierarchy), -1 for other shapes and for a miss. instance: 0 = the instance
 * a render launches for the loaded scene (the smallest that holds its shape kinds), 1 = the one
 * for every kind, 2 = triangles and spheres only, 3 = those plus meshes and boxes; an instance
 * that does not hold the scene's kinds is GI_ERR_ARG. GI_ELEM_PRETEST applies as in a render. */
int gi_intersect_probe(gi_ctx *ctx, int64_t n, const double *org, const double *dir,
                       const int32_t *hint, int instance, int32_t *hit, double *t, double *point,
                       double *normal, int32_t *material, int32_t *tri);
/* Test seam: RayIlluminationTest (illumination_utils.cpp:16-31) as the soft-light loops call it.
 * Per ray: the shaded point p_scene and a light index. light[i] >= 0 names an area or rect light
 * (else GI_ERR_ARG): the point on it is ((r1 u + r2 v) + centre) + normal * 1e-6 with (r1, r2) =
 * r12[2i], r12[2i + 1] (illumination_utils.cpp:150-157, 315-319: r in the unit disk for an area
 * light, in [-1/2, 1/2]^2 for a rect light). light[i] == -1 takes the point p_light_in[3i..].
 * use_mask: the fan's occluder mask of (light, p_scene) limits the elements searched, as in a
 * render with 16 or more samples per fan; it needs light[i] >= 0 for every ray (else GI_ERR_ARG).
 * instance as in gi_intersect_probe. Outputs: the point on the light used, and lit = 1 when the
 * point sees it, 0 when not. r12 / p_light_in may be NULL when no ray reads them. */
int gi_illum_probe(gi_ctx *ctx, int64_t n, const double *p_scene, const int32_t *light,
                   const double *r12, const double *p_light_in, int use_mask, int instance,
                   double *p_light_out, int32_t *lit);
/* Test seam: the world-space plane (unit normal n, offset d: n . x + d = 0) of every triangle of
 * the loaded scene, four doubles each, indexed as gi_intersect_probe's `tri`. *count = their
 * number; planes == NULL only reports it. */
int gi_scene_triangle_planes(gi_ctx *ctx, int64_t capacity, double *planes, int64_t *count);
/* Test seam, needs no context or device: the boxes of the scene file's two division-free slab
 * tests as the loader builds them, 20 doubles each: kind (0 = an element's box grown for the
 * element pre-test, 1 = a box of a mesh's hierarchy), simple (1 when at most one node on the
 * path from the root to the box's node has a transform), lo[3], hi[3] in the node's frame, and
 * rows 0..2 of that one transform's inverse (parent -> node; the identity when there is none).
 * *count = their number; boxes == NULL only reports it. */
int gi_scene_slab_boxes(const char *scene_path, int64_t capacity, double *boxes, int64_t *count);
/* Test seam: the device's fp64 math on host inputs, fn = 0 acos(x), 1 sin(x), 2 cos(x),
 * 3 pow(x, y), 4 atan2(x, y), 5 sqrt(x), 6 tan(x), 7 asin(x) (y ignored except by 3 and 4): the
 * functions the photon tracer, samplers and Phong terms call (graphics_utils.cpp:95-216,
 * photon_utils.cpp:56-60), gi_math.h's sequences, for comparing the device's results with the
 * oracle's (the same sequences on the host) and the host C library's one for one. */
int gi_math_probe(gi_ctx *ctx, int fn, int64_t n, const double *x, const double *y, double *out);

/* Free the context's render and photon-tracing device scratch (all devices of a device set),
 * keeping the scene, the photon maps and their kd trees; the next render or map build
 * re-allocates what it needs. For a long-lived context that must share the GPU with another
 * large one. No reference counterpart (the reference's buffers are host memory). */
int gi_release_scratch(gi_ctx *ctx);

/* ---- output --------------------------------------------------------------------------- */
int gi_write_image(const char *path, int width, int height, const uint8_t *rgb8);
/* Float image (W*H*3, rows from the bottom) by extension: .pfm = "PF", little-endian (scale
 * -1.0), rows bottom to top, so the pixel bytes are the array; .hdr = Radiance "#?RADIANCE",
 * FORMAT=32-bit_rle_rgbe, "-Y H +X W", flat (not run-length encoded) scanlines from the top row,
 * Ward's RGBE (frexp of the largest channel, mantissa bytes truncated, exponent + 128; four zero
 * bytes when it is below 1e-32). Any other extension: GI_ERR_ARG. No reference counterpart. */
int gi_write_image_float(const char *path, int width, int height, const float *rgbf);

#ifdef __cplusplus
}
#endif
#endif /* GI_H */
