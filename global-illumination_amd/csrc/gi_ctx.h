// gi_ctx.h -- the context behind include/gi.h and what the host units share (private: not
// installed). gi_context.cpp creates and destroys contexts and loads scenes, gi_photons.cpp
// builds the photon maps, gi_host.cpp renders, gi_frames.cpp works on finished frames,
// gi_probe.cpp holds the benchmarks and test seams.
//
// Ownership: every device buffer is a DBuf member of Scratch (freed by gi_release_scratch and at
// destroy) or of Resident (freed at destroy only); a new buffer goes into one of the two and needs
// no other line to be released.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "../../include/gi.h"
#include "gi_dbuf.h"
#include "gi_kdbuild.h"
#include "gi_kernels.h"
#include "gi_scene.h"
#include "gi_sort.h"

#pragma GCC visibility push(hidden)
namespace gi_internal {
using namespace gi;

// photon map on the host: the photons and, when built here (gi_photons.cpp kd_build), the
// implicit complete kd tree over them (leaf l holds photons [start(l), start(l + 1)),
// gi_layout.h kd_leaf_start; nleaves == 1 << levels, check_kd_shape)
struct HostMap {
  std::vector<gi_photon> storage;  // emission order
  std::vector<int32_t> perm;       // kd order -> storage index
  std::vector<float> pos4;
  std::vector<uint32_t> rgbe;
  std::vector<float> nodes;  // 8 floats per node: {lo.xyz, split}, {hi.xyz, axis bits}
  int nleaves = 1, levels = 0;
  float bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0};
};

struct DevMap {
  DBuf pos4, rgbe, nodes;
  DBuf dk;               // per-photon K-th distance bounds (KdView::dk), valid for dk_k / dk_r2
  int dk_k = -1;
  float dk_r2 = -1.0f;
  int64_t n = 0;
  int nleaves = 1, levels = 0;
  KdView view() const {
    KdView v;
    v.pos4 = pos4.as<float>();
    v.rgbe = rgbe.as<uint32_t>();
    v.nodes = nodes.as<float>();
    v.n = n;
    v.nleaves = nleaves;
    v.levels = levels;
    for (int k = 0; k < 3; k++) v.bmin[k] = v.bmax[k] = 0;
    v.dk = nullptr;
    return v;
  }
};

// RCCL, opened at run time by multi-device contexts only (gi_create_devices with distinct
// devices): the single-device library carries no RCCL dependency, and a torch process that
// loads it keeps its own copy.
struct Rccl {
  bool tried = false, ok = false;
  ncclResult_t (*commInitAll)(ncclComm_t *, int, const int *) = nullptr;
  ncclResult_t (*commDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*groupStart)() = nullptr;
  ncclResult_t (*groupEnd)() = nullptr;
  ncclResult_t (*send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  const char *(*errString)(ncclResult_t) = nullptr;
  ncclResult_t (*commCount)(const ncclComm_t, int *) = nullptr;
  ncclResult_t (*commUserRank)(const ncclComm_t, int *) = nullptr;
  bool load();
};
extern Rccl g_rccl;

// The queries a chunk k-NN pass hands on (gi_knn_chunk.hip to_fallback): 64 entries of query ids
// per chunk with the chunks' fill counts (and their scan), and the same ids compacted in chunk
// order (dense[n] = their number, n the pass's queries).
struct FbList {
  DBuf list, count, off, tmp, dense;
};

// Execution state of one photon map's k-NN launches (stream, timing events). One per map, so the
// two maps' estimates can run concurrently on two streams during a render.
struct MapExec {
  hipStream_t st = nullptr;        // the ctx stream, or the side stream while maps overlap
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;  // chunk pass | second
                                   // chunk pass | fallback split timing (ev0 ev2 ev3 ev1)
  uint64_t fb_total = 0;
};
// ... and their scratch
struct MapScratch {
  SortScratch sorter;              // Morton order of the query list
  DBuf list_idx, list_d2, list_n;  // K-best lists of the query-per-wave k-NN path
  DBuf gheap_d2, gheap_idx;        // global-memory heaps (K > 64 per-lane kernel)
  FbList fb[2];                    // chunk k-NN: the first pass writes fb[0], each further pass
                                   // the one its input is not in (run_chunk_knn)
  DBuf dk_q;                       // photon positions as queries (ensure_dk)
};

// The render's, the photon tracer's and the frame functions' device scratch: everything that
// gi_release_scratch frees (by assigning a fresh Scratch) and the next call re-allocates.
struct Scratch {
  MapScratch map[2];
  DBuf pack;                         // this device's shard pixels, packed for the gather
  std::vector<DBuf> recv, peer_pix;  // first device: each peer's packed pixels and pixel list
  KdBuildScratch kdb;            // scratch of the device kd build (gi_kdbuild.hip)
  DBuf kd_ph;                    // emission-ordered photons uploaded for the device build
  DBuf ind_cont, ind_ncont;       // indirect paths that continue past their first bounce
  DBuf mc_cont, mc_ncont;         // Monte Carlo paths' indirect sub-paths
  DBuf mc_cont2, mc_ncont2;       // ... those continuing past a glass / mirror first hit
  DBuf mc_wstate, mc_wlist, mc_wcount;  // breadth-first Monte Carlo paths: states, live lists and counters (McWave)
  DBuf prim_rgb;                  // per-primary sums of the reduction
  DBuf d_rays, d_ray_ids;         // ray mode: the batch's rays and stream ids (gi_render_rays);
                                  // gi_camera_rays: one chunk of its output
  std::vector<gi_ray> ray_stage;  // ... gathered in batch order where the batch's pixels are
  std::vector<uint64_t> id_stage; // not one row-major run (tile shards)
  DBuf ind_tab, mc_tab;           // row -> tile of the tiled indirect entries; owner of MC path 64k
  DBuf ind_trows, ind_rows;       // indirect paths' tiled slots: rows per tile, their scan
  DBuf ind_masks;                 // their rows' query and base masks
  // render scratch
  DBuf spawn, npaths, path_off, nmc, mc_off, nind, ind_off, base, pixels, rgbf, rgb8, stats_bak;
  DBuf qpos[2], qshade[2], qkey[2], qout[2];
  DBuf qseg[2];  // per list, [nprim + 1]: the sorted appends of primary b are [qseg[b], qseg[b + 1])
  KeySortScratch keysort[2];
  DBuf scan_lvl[8], scan_out[8];
  // photon tracing scratch
  DBuf pcounts, poffs, pbuf;
  DBuf pkeys, pcursor, ptmp;      // single pass: slot keys, slot counter, sorted photons (host sink)
  DBuf pacc, pglob;               // maps being traced on the device (emission order), held global map
  KeySortScratch psort;
  // feature planes (gi_camera_features / gi_ray_features): one chunk of sample records and of
  // planes; denoise pass (gi_denoise): the frame's floats, its planes, the two ping-pong images
  DBuf feat_samples, feat_planes, dn_rgbf, dn_planes, dn_img[2];
  // variance-guided denoise (gi_denoise_radiance, gi_accum_denoise): the uploaded channel
  // variances and the filtered luminance-variance plane; the rest is gi_denoise's scratch
  DBuf vdn_var, vdn_vlum;
  // radiance frames: rad_frame holds the pass's {m, M2} (six doubles per pixel), rad_samples the
  // samples when the caller asked for them
  DBuf rad_frame, rad_samples, rad_mean, rad_var;
  // light-path layers (gi.h GI_LAYER_*), layer-major: the batch's per-primary sums, the frame's
  // {m, M2} planes and, when asked for, its samples
  DBuf prim_layers, lay_frame, lay_samples;
  DBuf acc_part;                        // per-block partial sums of the accumulator's reductions
  DBuf tile_err, tile_nmin, tile_mask;  // adaptive passes: per tile error, smallest count, mask
  DBuf rp_prev, rp_cur;                 // reprojection: the two uploaded plane sets
  DBuf tm_in, tm_out;                   // gi_tonemap
};

// Device state that survives gi_release_scratch, freed by gi_destroy: the scene, the direction
// table, the counters, the photon maps with their dk bounds, and the accumulator.
struct Resident {
  DBuf d_nodes, d_elems, d_shapes, d_tris, d_bvh, d_mats, d_lights, d_lut, d_stats;
  DBuf qcount;  // the query lists' fill counters (and mc_persist_kernel's path counter)
  DevMap dmap[2];
  // accumulator over passes (gi_accum_*): {mu, A} per pixel and channel (acc) and one sample
  // count per pixel (acc_cnt); the reprojection's second accumulator and count plane (swapped
  // with acc / acc_cnt afterwards; allocated on first use)
  DBuf acc, acc_cnt, acc2, acc2_cnt;
};

}  // namespace gi_internal
using namespace gi_internal;

struct gi_ctx {
  int device = 0;
  // Device set (gi_create_devices): this context drives the first device and forwards every
  // call to one context per further device. Output tile (tx, ty) goes to device (tx + ty) % ndev
  // (shard_pixels' diagonal deal); photon emission ranges are split across the devices; the maps
  // are built once and replicated.
  std::vector<gi_ctx *> peers;
  std::vector<ncclComm_t> comms;     // [ndev] RCCL communicators (distinct devices), else empty
  std::mutex err_mu;                 // err is written by the map worker threads too
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;     // side stream: Monte Carlo paths beside the indirect paths
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  MapExec mx[2];
  Scratch s;     // device buffers by lifetime (see the two structs)
  Resident res;
  std::string err;
  gi_params P;
  bool have_params = false;
  bool have_scene = false;
  HostScene scene;
  // photon maps
  HostMap hmap[2];
  bool map_valid[2] = {false, false};
  int leaf_size[2] = {64, 256};  // photons per kd leaf, per map (global, caustic)
  bool gpu_kd = true;            // kd trees built on the device (gi_kdbuild.hip); GI_HOST_KD=1: host
  int wave_cap_mul = 1;
  int chunk_cap_big = 512;        // large-K chunk kernel: LDS candidates of the first pass
  // large-K chunk kernel: the centre's dk bound refined to the exact d_K(c) (GI_CHUNK_DK_EXACT,
  // default on: C4 shard caustic k-NN 154.7 -> 145.1 ms per launch, C2 / C3 frames -0.7 / -1.0 %;
  // profiles/r05_dk_exact_ab.txt)
  bool chunk_dk_exact = true;
  int chunk_minsub_big = 64;      // large-K chunk kernel: overflowing chunks retried down to this (64: none, measured best)
  int chunk_minsub = 32;          // chunk kernel: overflowing chunks retried as halves (measured best with the dk bound)
  double fb_ms[2] = {0, 0};       // final fallback kernel's time and queries per map (since the
  uint64_t fb_q[2] = {0, 0};      // last reset)
  double p2_ms[2] = {0, 0};       // second chunk pass's time and queries per map
  uint64_t p2_q[2] = {0, 0};
  int last_kind[2] = {-1, -1};     // k-NN kind run_knn chose last, per map (gi_render_stats)
  bool knn_log = false;            // GI_LOG & 4: one stderr line per chunk k-NN launch
  int knn_dbg = 0;                 // GI_KNN_DBG: k-NN kernel diagnostics (KnnArgs::dbg)
  int render_dbg = 0;              // GI_DBG: render-kernel diagnostics (RenderArgs::dbg)
  int64_t slot_limit = 0;          // GI_SLOT_LIMIT: path slots per batch (tests; 0 = 2^31)
  int elem_pretest = -1;           // GI_ELEM_PRETEST: -1 auto (make_view), 0 off, 1 on
  gi_progress_fn progress = nullptr;  // gi_set_progress
  void *progress_user = nullptr;
  int64_t progress_done = 0, progress_total = 0;  // output pixels of the current RenderImage
  int sel_slack = 64;
  int knn_qpl = 1;
  bool mc_sub = true;             // sub-paths' first bounce in mc_sub_kernel (GI_MC_SUB=0: all in ind_cont_kernel)
  int mc_persist = -1;            // Monte Carlo paths in mc_persist_kernel with this many blocks
                                  // (GI_MC_PERSIST; 0: mc_kernel, one path per lane; -1: auto)
  int mc_wave = -1;               // Monte Carlo paths breadth first, this many single-bounce launches
                                  // before the tail (GI_MC_WAVE; 0: off; -1: auto); a persistent
                                  // grid asked for by number goes first
  bool split_ind = true;          // continuation queue for indirect paths (else one loop per lane)
  double ind_frac = 0.25;         // continuation queue size, as a fraction of its worst case
  bool chunk_big2 = true;            // large-K chunk k-NN: further chunk passes
  // ... the second pass's LDS candidates (1024) and a third pass's (GI_CHUNK_CAP_BIG3, test knob;
  // 0: none). r05: a 576-candidate pass at two waves per SIMD, alone or before the 1024 one, was
  // not faster (profiles/r05_chunk_pass_chain_ab.txt)
  int chunk_cap_big2 = 1024;
  int chunk_cap_big3 = 0;
  bool chunk_lane2 = true;           // lane-select chunk k-NN: second pass (480; without it C5 +1.8 %, C2 / C4 +0.4-0.6 %, r06)
  int chunk_minsub_big2 = 64;        // ... its overflowing chunks retried down to this group size
  bool chunk_dk = true;            // chunk kernel (K <= 64): centre bound from the dk bounds (measured: fewer fallbacks)
  bool chunk_fb_all = false;       // test knob: the lane-select chunk kernel hands every query to its fallback
  // k-NN instances: 0 auto (knn_general), 1 the general estimate form only (GI_KNN_GENERAL=1,
  // and after an instance without it met a query that needed it), -1 test knob: claim that no
  // render query needs it (GI_KNN_GENERAL=-1; exercises render_common's re-run)
  int knn_general_mode = 0;
  // launch-order cells per axis for the global / caustic list (> 10: 64-bit keys, gi_sort.hip
  // curve64_valid_kernel). The caustic queries crowd into foci far smaller than
  // a 10-bit cell of the scene box, where a cell's queries stay in slot order: 16-bit cells cut
  // the C4 shard's caustic k-NN 207 -> 155 ms per launch (second-pass queries 37.8 % -> 14.9 %).
  // The global list (C2: 400 M slots, one query per ~cell) keeps 32-bit keys: a 64-bit sort
  // would cost more than it saves (profiles/r05_key_bits_ab.txt).
  int key_bits[2] = {10, 16};
  // GI_ROW_ORDER (default 1): the global list's valid slots compacted from the row masks before
  // the sort (gi_sort.h curve_order_rows) instead of sorting every slot with the empty ones last
  bool row_order = true;
  bool surf_key = true;             // global list: surface keys (gi_sort.hip surface_key) instead of the 3-D curve
  bool surf_key_c = true;           // caustic list: 64-bit surface keys (surf64_valid_kernel)
  bool fb_wave = true;              // chunk kernel's last fallback: the query-per-wave kernel (r06; the per-lane one: GI_FB_WAVE=0)
  bool use_dk = true;              // wave k-NN kernel starts from per-photon K-th bounds
  size_t qcap_hint[2] = {0, 0};
  int knn_kernel_kind = -1;  // -1 auto; run_knn lists the kinds
  int64_t pacc_n = 0;             // photons in s.pacc
  double prate[2] = {2.0, 2.0};   // stored per emitted photon in the last launch, per map
  bool photon_2pass = false;      // GI_PHOTON_2PASS=1: count pass + scan + re-trace (r03)
  // Primary samples per batch. Denser query batches make the chunk k-NN's 64 Morton-adjacent
  // queries span less of a K-neighbourhood (fewer LDS candidates per query): C2 at 2^19 / 2^20 /
  // 2^21 / 2^22 ran 6.85 / 7.44 / 7.89 / 7.69 Mpixel-samples/s. A batch is also capped by the
  // query budget below (queries per primary sample vary ~10x between scenes).
  int64_t prim_per_batch = 1 << 21;
  int64_t batch_reruns = 0;          // batches re-run smaller for 32-bit path slots (render_pixels)
  bool batch_log = false;            // GI_LOG & 2: per-batch sizes and times on stderr
  int64_t query_budget = 400000000;  // photon-map queries per batch (~120 B each: ~48 GB)
  double q_per_prim = 0.0;           // largest queries per primary sample seen so far
  double mc_app_rate[2] = {0.0, 0.0};  // per list: largest appends per Monte Carlo path seen
  float sbmin[3] = {0, 0, 0}, sbmax[3] = {1, 1, 1};
  // radiance frames (gi_render_radiance, gi_render_rays_radiance, gi_accum_add_*): while rad_on,
  // render_pixels launches reduce_radiance_kernel beside reduce_kernel
  bool rad_on = false, rad_want_samples = false;
  // ... and, while lay_on, reduce_prim_layers_kernel and one reduce_radiance_kernel per layer
  // into s.lay_frame (lay_npix pixels per plane). lay_time: the kernel between two events, waited
  // for per batch and summed into lay_ms (gi_layers_timing)
  bool lay_on = false, lay_time = false;
  size_t lay_npix = 0;
  double lay_ms = 0.0;
  // accumulator over passes (res.acc, res.acc_cnt): state of the context, kept by
  // gi_release_scratch. While only whole-frame passes were folded (acc_uniform) every count is acc_n.
  int acc_w = 0, acc_h = 0;
  int64_t acc_n = 0;
  bool acc_valid = false, acc_uniform = true;
};

namespace gi_internal {

// the calling thread's current HIP device, restored on scope exit (the packed entry points run
// inside processes whose torch shares that device setting)
struct DeviceScope {
  int prev = -1;
  explicit DeviceScope(int d) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    hipSetDevice(d);
  }
  ~DeviceScope() {
    if (prev >= 0) hipSetDevice(prev);
  }
};

// Ray source of a render (gi_render_rays): spp rays per output pixel, pixel (x, y)'s at
// [(y * w + x) * spp, ...) of the caller's frame-wide host buffers; ids may be null.
struct RaySrc {
  const gi_ray *rays;
  const uint64_t *ids;
  int spp;
};

inline void set_err(gi_ctx *c, const std::string &msg) {
  std::lock_guard<std::mutex> g(c->err_mu);
  c->err = msg;
}
inline int fail(gi_ctx *c, int code, const std::string &msg) {
  set_err(c, msg);
  return code;
}

// nleaves == 1 << levels (gi_layout.h kd_levels_ok): the leaf ranges are computed by a shift, so
// a map whose shape breaks it is refused where it is made, exported or handed to a kernel
inline int check_kd_shape(gi_ctx *c, int nleaves, int levels) {
  if (kd_levels_ok(nleaves, levels)) return GI_OK;
  return fail(c, GI_ERR_STATE, "photon map: " + std::to_string(nleaves) + " kd leaves are not 2^" +
                                 std::to_string(levels));
}

#define HIPCHK(ctx, call)                                                                   \
  do {                                                                                      \
    hipError_t _e = (call);                                                                 \
    if (_e != hipSuccess) {                                                                 \
      set_err((ctx), std::string("HIP error: ") + hipGetErrorString(_e) + " at " + __FILE__ + \
                         ":" + std::to_string(__LINE__));                                   \
      return GI_ERR_HIP;                                                                    \
    }                                                                                       \
  } while (0)

// device counters: ST_STRIPES copies of ST_COUNT words (gi_kernels.h wave_add), summed by read_stats
constexpr size_t ST_BYTES = (size_t)ST_STRIPES * ST_COUNT * 8;

// gi_context.cpp
Flags make_flags(const gi_params &P);
DCamera make_camera(const HostScene &H, const gi_params &P);
SceneView make_view(gi_ctx *c);
hipError_t upload(DBuf &b, const void *src, size_t bytes, hipStream_t st);
ScanTemp scan_temp(gi_ctx *c, int64_t n);
int check_ready(gi_ctx *c);
// gi_host.cpp
hipError_t read_stats(gi_ctx *c, unsigned long long *out);
void log_phase_cycles(const gi_ctx *c, const unsigned long long *s);
int knn_general(const std::vector<DMaterial> &mats, int filter, bool every_material = false);
KnnArgs knn_args(gi_ctx *c, int mi);
int ensure_dk(gi_ctx *c, KnnArgs &k);
int run_knn(gi_ctx *c, KnnArgs k, int64_t nq, double *ms);
int render_common(gi_ctx *c, int aa, int w, int h, const std::vector<int32_t> &pix, uint8_t *rgb8,
                  float *rgbf, gi_render_stats *st, bool keep_rgbf, const RaySrc *rsrc = nullptr);
int render_frame(gi_ctx *c, int aa, int w, int h, uint8_t *rgb8, float *rgbf, gi_render_stats *st,
                 const RaySrc *rsrc);

// Run fn(k, ctx_k) for every device of the set (k = 0 is this context, run on the calling
// thread, so its progress callbacks arrive where gi.h promises; each peer on a host thread of
// its own); returns the first failure, with that device's message copied into c->err.
template <typename Fn>
int on_devices(gi_ctx *c, Fn fn) {
  const int nd = 1 + (int)c->peers.size();
  if (nd == 1) return fn(0, c);
  std::vector<int> rc(nd, GI_OK);
  auto run = [&](int k, gi_ctx *d) {
    if (hipSetDevice(d->device) != hipSuccess) {
      rc[k] = fail(d, GI_ERR_HIP, "hipSetDevice failed");
      return;
    }
    try {
      rc[k] = fn(k, d);
    } catch (const std::bad_alloc &) {
      rc[k] = fail(d, GI_ERR_ALLOC, "host allocation failed");
    } catch (...) {
      rc[k] = fail(d, GI_ERR_HIP, "unexpected exception");
    }
  };
  std::vector<std::thread> th;
  for (int k = 1; k < nd; k++) th.emplace_back(run, k, c->peers[k - 1]);
  run(0, c);
  for (auto &t : th) t.join();
  hipSetDevice(c->device);
  for (int k = 0; k < nd; k++)
    if (rc[k] != GI_OK) {
      if (k) set_err(c, "device " + std::to_string(c->peers[k - 1]->device) + ": " + c->peers[k - 1]->err);
      return rc[k];
    }
  return GI_OK;
}

}  // namespace gi_internal
#pragma GCC visibility pop
