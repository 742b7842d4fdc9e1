// gi_host.cpp -- host orchestration of the MI355X renderer's frames: the k-NN dispatch, the
// batched render and its entry points of include/gi.h.
//
// Replaces the reference's RenderImage (render.cpp:155-259): its CPU threads become batched
// wavefront launches, and host code only sequences kernels. The context, the photon maps
// (MapPhotons), the frame functions and the probes are gi_context.cpp, gi_photons.cpp,
// gi_frames.cpp and gi_probe.cpp; gi_ctx.h is what they share.
#include <chrono>
#include <cmath>
#include <functional>
#include "gi_ctx.h"
#include "gi_radiance.h"

namespace gi_internal __attribute__((visibility("hidden"))) {

hipError_t read_stats(gi_ctx *c, unsigned long long *out) {
  std::vector<unsigned long long> all((size_t)ST_STRIPES * ST_COUNT);
  hipError_t e = hipMemcpyAsync(all.data(), c->res.d_stats.p, ST_BYTES, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  for (int i = 0; i < ST_COUNT; i++) {
    out[i] = 0;
    for (int s = 0; s < ST_STRIPES; s++) out[i] += all[(size_t)s * ST_COUNT + i];
  }
  return e;
}
// GI_KNN_DBG & 16: the k-NN kernels' phase counters of the counters read_stats summed, on stderr
void log_phase_cycles(const gi_ctx *c, const unsigned long long *s) {
  if (!(c->knn_dbg & 16)) return;
  fprintf(stderr, "[gi] k-NN phase cycles (sum over waves):");
  for (int i = 0; i < 16; i++) fprintf(stderr, " %llu", s[ST_PHASE + i]);
  fprintf(stderr, "\n");
}

// KnnArgs::general: 0 when the map's filter is the disk and no material a query can carry (kd or
// the diffuse flag: queries sit on diffuse hits) has a specular term -- the device's test for the
// estimate's common form (photon_utils.cpp:98-158; gi_knn.hip wave_estimate) -- so the k-NN
// kernels can run their instances without pow
// (every_material: also those no render query can carry -- the estimate seam's per-query ones)
int knn_general(const std::vector<DMaterial> &mats, int filter, bool every_material) {
  if (filter != 0) return 1;
  for (const DMaterial &m : mats) {
    if (!every_material && !(m.flags & MF_DIFFUSE) && m.max_kd == 0.0) continue;
    const bool spec = (m.flags & MF_SPECULAR) || (m.n < 0);
    if (spec || !std::isfinite(m.ks[0]) || !std::isfinite(m.ks[1]) || !std::isfinite(m.ks[2]))
      return 1;
  }
  return 0;
}

KnnArgs knn_args(gi_ctx *c, int mi) {
  KnnArgs k;
  memset(&k, 0, sizeof k);
  k.map = c->res.dmap[mi].view();
  k.mats = c->res.d_mats.as<DMaterial>();
  k.lut = c->res.d_lut.as<double>();
  const gi_params &P = c->P;
  k.K = mi == GI_MAP_GLOBAL ? P.global_estimate_size : P.caustic_estimate_size;
  double r = mi == GI_MAP_GLOBAL ? P.global_estimate_dist : P.caustic_estimate_dist;
  k.filter = mi == GI_MAP_GLOBAL ? P.global_filter : P.caustic_filter;
  k.r2f = (float)(r * r);
  k.rmax = r;
  k.fa = P.filter_const_a;
  k.fb = P.filter_const_b;
  k.fk = P.filter_const_k;
  k.stats = c->res.d_stats.as<unsigned long long>();
  k.stat_off = mi == GI_MAP_GLOBAL ? 0 : ST_KNN_MAP;
  k.sel_slack = c->sel_slack;
  k.chunk_minsub = c->chunk_minsub;
  k.qpl = c->knn_qpl;
  k.general = c->knn_general_mode > 0 ? 1 : c->knn_general_mode < 0 ? 0 : knn_general(c->scene.mats, k.filter);
  k.dbg = c->knn_dbg;
  return k;
}

// the map a launch's arguments were made for (knn_args): 0 global, 1 caustic
static int map_index(const KnnArgs &k) { return k.stat_off ? 1 : 0; }

// Per-photon K-th distance bounds of map mi for this launch's K and r (KdView::dk): one
// KNN_MODE_DK pass of the wave kernel with the photons themselves as queries, computed once
// per map and (K, r). The wave kernel then starts each query from the bound of the photons in
// its leaf instead of from r.
int ensure_dk(gi_ctx *c, KnnArgs &k) {
  MapExec &X = c->mx[map_index(k)];
  MapScratch &XS = c->s.map[map_index(k)];
  DevMap &D = c->res.dmap[map_index(k)];
  if (!c->use_dk || D.n == 0 || k.K <= 0) return GI_OK;
  if (int rc = check_kd_shape(c, k.map.nleaves, k.map.levels)) return rc;
  if (D.dk_k != k.K || D.dk_r2 != k.r2f) {
    D.dk_k = -1;
    HIPCHK(c, XS.dk_q.ensure((size_t)D.n * 16));
    HIPCHK(c, D.dk.ensure((size_t)D.n * 4));
    launch_photon_queries(D.pos4.as<float>(), D.n, XS.dk_q.as<float4>(), X.st);
    KnnArgs d = k;
    d.mode = KNN_MODE_DK;
    d.map.dk = nullptr;
    d.qpos = XS.dk_q.as<float4>();
    d.qshade = nullptr;
    d.perm = nullptr;
    d.nq = D.n;
    d.q0 = 0;
    d.out_dk = D.dk.as<float>();
    d.stats = nullptr;
    d.dbg = 0;
    if (!launch_knn_wave(d, c->wave_cap_mul, X.st))
      return fail(c, GI_ERR_ARG, "k-NN bound pass: unsupported estimate size");
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(X.st));
    D.dk_k = k.K;
    D.dk_r2 = k.r2f;
  }
  k.map.dk = D.dk.as<float>();
  return GI_OK;
}

// Kernel choice of a launch (GI_KNN_KERNEL overrides; -1 = auto):
//   7  chunk kernel with lane select + per-lane fallback (K <= 64, estimates): the default
//   3  per-lane kernel, LDS heaps (K <= 128; list mode)
//   8  large-K chunk kernel + query-per-wave fallback (K > 64, estimates; needs dk bounds)
//   1  query-per-wave kernel (K + 64 <= 1024)
//   0  per-lane kernel with global-memory heaps (any K)
//  10  fixed-radius range estimate (gi_range.hip; estimates with K above the map's photon count:
//      no query reaches K, so nothing is selected). Automatic where only kind 0 served before.
static int knn_kind(const gi_ctx *c, const KnnArgs &k) {
  int kind = c->knn_kernel_kind;
  const bool list = k.mode == KNN_MODE_LIST, dkm = k.mode == KNN_MODE_DK;
  const bool wide = (int64_t)k.K + 64 > 1024;  // beyond the LDS selection kernels
  const bool range_ok = !list && !dkm && (int64_t)k.K > k.map.n;
  int auto_kind = (k.K <= 64) ? (list ? 3 : 7) : ((list || !c->use_dk) ? 1 : 8);
  if (range_ok && wide) auto_kind = 10;
  if (kind < 0) kind = auto_kind;
  // an override that cannot serve this launch falls back to the automatic choice
  if (kind == 10 && !range_ok) kind = auto_kind;
  if (kind == 10) return kind;
  if (kind == 7 && (k.K > 64 || list)) kind = auto_kind;
  if (kind == 8 && (list || dkm || wide || !c->use_dk)) kind = auto_kind == 8 ? 1 : auto_kind;
  if (kind == 3 && (size_t)k.K * 512 > 64 * 1024) kind = auto_kind;
  if (kind == 1 && wide) kind = 0;
  return kind;
}

// end of a launch on the map's stream: records ev1 and, when the caller times the launch, waits
// for it and adds the time since ev0 to *ms
static int knn_end(gi_ctx *c, MapExec &X, double *ms) {
  HIPCHK(c, hipEventRecord(X.ev1, X.st));
  if (ms) {
    HIPCHK(c, hipEventSynchronize(X.ev1));
    float t = 0;
    HIPCHK(c, hipEventElapsedTime(&t, X.ev0, X.ev1));
    *ms += t;
  }
  return GI_OK;
}

// Makes F ready for what a chunk pass over nq queries hands on and points the pass's arguments
// at it. Per-chunk list (gi_knn_chunk.hip to_fallback): chunk c's queries at [64 c, 64 c + count[c]),
// so the compacted list is in chunk order in every launch.
static int fb_prepare(gi_ctx *c, MapExec &X, FbList &F, int64_t nq, KnnArgs &k) {
  const int64_t chunks = (nq + 63) / 64;
  HIPCHK(c, F.list.ensure((size_t)chunks * 64 * 4));
  HIPCHK(c, F.dense.ensure((size_t)nq * 4 + 4));
  HIPCHK(c, F.count.ensure((size_t)(chunks + 1) * 4));
  HIPCHK(c, F.off.ensure((size_t)(chunks + 1) * 4));
  HIPCHK(c, hipMemsetAsync(F.count.p, 0, (size_t)(chunks + 1) * 4, X.st));
  k.fb_list = F.list.as<uint32_t>();
  k.fb_count = F.count.as<uint32_t>();
  return GI_OK;
}

// Compacts what the pass with arguments k, over nq queries, handed on into F.dense and reads their
// number back (one host synchronization); ev, when given, is recorded behind the compaction.
static int fb_collect(gi_ctx *c, MapExec &X, FbList &F, const KnnArgs &k, int64_t nq,
                      hipEvent_t ev, uint32_t *n) {
  uint32_t *dense = F.dense.as<uint32_t>();
  const int64_t chunks = (nq + 63) / 64;
  size_t tb = 0;
  HIPCHK(c, launch_fb_compact(k.fb_list, k.fb_count, chunks, F.off.as<uint32_t>(), nullptr, tb, dense,
                              dense + nq, X.st));
  HIPCHK(c, F.tmp.ensure(tb + 256));
  HIPCHK(c, launch_fb_compact(k.fb_list, k.fb_count, chunks, F.off.as<uint32_t>(), F.tmp.p, tb, dense,
                              dense + nq, X.st));
  if (ev) HIPCHK(c, hipEventRecord(ev, X.st));
  HIPCHK(c, hipMemcpyAsync(n, dense + nq, 4, hipMemcpyDeviceToHost, X.st));
  HIPCHK(c, hipStreamSynchronize(X.st));
  return GI_OK;
}

// One kernel launch of a chunk pipeline over its arguments' queries, with the changes to them
// that are its own; false: no instance of the kernel serves them.
using KnnPass = std::function<bool(KnnArgs)>;

// The launch sequence of kinds 7 and 8: a chunk pass over all queries, further chunk passes over
// what the pass before handed on (the compacted lists keep each chunk's queries together, in
// Morton order), and a last-resort kernel for what the last chunk pass hands on.
struct ChunkPipeline {
  int kind;
  const char *first_label, *last_label;  // of the GI_LOG & 4 line
  KnnPass first;
  std::vector<KnnPass> more;
  KnnPass last;
};

// k: the first pass's arguments, over nq queries, with the map's fb[0] prepared for them (fb_prepare).
// Every later pass gets k with the dense list of the pass before as its queries; pass i of `more`
// writes fb[(i + 1) & 1] (ping-pong: a list is free once the pass behind it has read it).
static int run_chunk_knn(gi_ctx *c, MapExec &X, const KnnArgs &k, int64_t nq, double *ms,
                         const ChunkPipeline &P) {
  FbList *fb = c->s.map[map_index(k)].fb;
  HIPCHK(c, hipEventRecord(X.ev0, X.st));
  if (!P.first(k)) return fail(c, GI_ERR_ARG, "k-NN launch: large-K chunk kernel unavailable");
  HIPCHK(c, hipGetLastError());
  uint32_t nfb = 0;
  int rc = fb_collect(c, X, fb[0], k, nq, X.ev2, &nfb);
  if (rc) return rc;
  X.fb_total += nfb;
  uint32_t rest = nfb;
  const uint32_t *dense = fb[0].dense.as<uint32_t>();
  bool ran_more = false;
  for (size_t i = 0; i < P.more.size() && rest; i++) {
    ran_more = true;
    FbList &F = fb[(i + 1) & 1];
    const uint32_t nin = rest;
    KnnArgs s = k;
    s.perm = dense;
    s.nq = nin;
    s.q0 = 0;
    s.dbg &= ~16;
    if ((rc = fb_prepare(c, X, F, nin, s))) return rc;
    if (!P.more[i](s)) return fail(c, GI_ERR_ARG, "k-NN launch: large-K chunk kernel unavailable");
    HIPCHK(c, hipGetLastError());
    if ((rc = fb_collect(c, X, F, s, nin, nullptr, &rest))) return rc;
    dense = F.dense.as<uint32_t>();
  }
  HIPCHK(c, hipEventRecord(X.ev3, X.st));
  if (rest) {
    KnnArgs f = k;
    f.perm = dense;
    f.nq = rest;
    f.q0 = 0;
    if (!P.last(f))
      return fail(c, GI_ERR_ARG, "k-NN launch: unsupported estimate size for this kernel");
    HIPCHK(c, hipGetLastError());
  }
  double t = 0;
  if ((rc = knn_end(c, X, ms ? &t : nullptr))) return rc;
  if (ms) {
    float tf = 0, t2 = 0;
    HIPCHK(c, hipEventElapsedTime(&tf, X.ev3, X.ev1));
    HIPCHK(c, hipEventElapsedTime(&t2, X.ev2, X.ev3));
    *ms += t;
    const int mi = map_index(k);
    c->fb_ms[mi] += tf;
    c->fb_q[mi] += rest;
    c->p2_ms[mi] += t2;
    c->p2_q[mi] += ran_more ? nfb : 0;
    if (c->knn_log)
      fprintf(stderr, "[gi] knn map %d kind %d: nq %lld %s %.2f ms, second pass %u (%.2f ms), %s %u (%.2f ms)\n",
              mi, P.kind, (long long)nq, P.first_label, (float)t - tf - t2, nfb, t2, P.last_label,
              rest, tf);
  }
  return GI_OK;
}

// run a k-NN launch over nq queries (chunked when the heap lives in global scratch)
int run_knn(gi_ctx *c, KnnArgs k, int64_t nq, double *ms) {
  MapExec &X = c->mx[map_index(k)];
  MapScratch &XS = c->s.map[map_index(k)];
  const hipStream_t st = X.st;
  if (int rc = check_kd_shape(c, k.map.nleaves, k.map.levels)) return rc;
  const int kind = knn_kind(c, k);
  if (k.mode != KNN_MODE_DK) c->last_kind[map_index(k)] = kind;
  if (kind == 10) {
    // fixed-radius range estimate: one launch, no dk bounds, no fallback
    k.nq = nq;
    k.q0 = 0;
    k.map.dk = nullptr;
    HIPCHK(c, hipEventRecord(X.ev0, X.st));
    if (!launch_knn_range(k, X.st))
      return fail(c, GI_ERR_ARG, "k-NN launch: the range estimate needs an estimate size above the map");
    HIPCHK(c, hipGetLastError());
    return knn_end(c, X, ms);
  }
  if (kind == 8) {
    // large-K chunk kernel, then the query-per-wave kernel on what it hands over
    int rc = ensure_dk(c, k);
    if (rc) return rc;
    k.nq = nq;
    k.q0 = 0;
    if ((rc = fb_prepare(c, X, XS.fb[0], nq, k))) return rc;
    k.chunk_minsub = c->chunk_minsub_big;
    k.dk_exact = c->chunk_dk_exact ? 1 : 0;
    ChunkPipeline P{8, "chunk pass", "wave"};
    P.first = [&](KnnArgs a) { return launch_knn_chunk_big(a, c->chunk_cap_big, st); };
    // further chunk passes with more LDS candidates each (chunk_cap_big2: 1024 by default;
    // chunk_cap_big3 > 0 adds a third)
    const int caps[2] = {c->chunk_cap_big2, c->chunk_cap_big3};
    for (int i = 0; i < 2 && c->chunk_big2 && caps[i] > 0; i++) {
      const int cap = caps[i];
      P.more.push_back([c, st, cap](KnnArgs a) {
        a.chunk_minsub = c->chunk_minsub_big2;
        return launch_knn_chunk_big(a, cap, st);
      });
    }
    P.last = [&](KnnArgs a) { return launch_knn_wave(a, c->wave_cap_mul, st); };
    return run_chunk_knn(c, X, k, nq, ms, P);
  }
  if (kind == 7) {
    // chunk kernel, then its 480-candidate second pass on the chunks that overflowed its LDS
    // gather, then the query-per-wave (or per-lane) kernel on those that overflowed that
    k.nq = nq;
    k.q0 = 0;
    int rc = fb_prepare(c, X, XS.fb[0], nq, k);
    if (rc) return rc;
    // per-photon K-th distance bounds: the fallback's starting bound; the chunk kernel's centre
    // bound uses them only with chunk_dk (else the exact d_K(c) gather)
    const float *fb_dk = nullptr;
    if (c->use_dk && k.mode != KNN_MODE_DK) {
      if ((rc = ensure_dk(c, k))) return rc;
      fb_dk = k.map.dk;
      if (!c->chunk_dk) k.map.dk = nullptr;
    }
    ChunkPipeline P{7, "chunk", "per-lane"};
    P.first = [&](KnnArgs a) {
      if (c->chunk_fb_all) a.dbg |= 4;  // lane select skipped: all to the fallback
      launch_knn_chunk(a, st);
      return true;
    };
    if (c->chunk_lane2 && !c->chunk_fb_all)
      P.more.push_back([st](KnnArgs a) {
        launch_knn_chunk2(a, st);
        return true;
      });
    P.last = [&](KnnArgs a) {
      a.map.dk = fb_dk;
      if (c->fb_wave) return launch_knn_wave(a, c->wave_cap_mul, st);
      launch_knn_lane(a, st);
      return true;
    };
    return run_chunk_knn(c, X, k, nq, ms, P);
  }
  if (kind == 3) {
    k.nq = nq;
    k.q0 = 0;
    HIPCHK(c, hipEventRecord(X.ev0, X.st));
    launch_knn_lane(k, X.st);
    HIPCHK(c, hipGetLastError());
    return knn_end(c, X, ms);
  }
  if (kind == 1) {
    // one query per wave; the search writes per-query K-best lists in list / DK mode (and when
    // the estimate is not fused into it), a second kernel estimates from them
    k.nq = nq;
    k.q0 = 0;
    if (k.mode == KNN_MODE_LIST) {
      k.list_idx = k.out_idx;
      k.list_d2 = k.out_d2;
      k.list_n = k.out_n;
    } else {
      size_t slots = (size_t)nq * (size_t)k.K;
      HIPCHK(c, XS.list_idx.ensure(slots * 4));
      HIPCHK(c, XS.list_d2.ensure(slots * 4));
      HIPCHK(c, XS.list_n.ensure((size_t)nq * 4));
      k.list_idx = XS.list_idx.as<int32_t>();
      k.list_d2 = XS.list_d2.as<float>();
      k.list_n = XS.list_n.as<int32_t>();
    }
    int rc = ensure_dk(c, k);
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(X.ev0, X.st));
    if (!launch_knn_wave(k, c->wave_cap_mul, X.st))
      return fail(c, GI_ERR_ARG, "k-NN launch: unsupported estimate size for this kernel");
    HIPCHK(c, hipGetLastError());
    return knn_end(c, X, ms);
  }
  // kind 0: per-lane heaps in global scratch, launched in slices of 2^20 queries
  const int64_t CH = (int64_t)(1 << 20);
  for (int64_t s = 0; s < nq; s += CH) {
    int64_t m = std::min(CH, nq - s);
    KnnArgs a = k;
    a.nq = m;
    a.q0 = s;
    {
      size_t slots = (size_t)((m + 63) / 64) * 64 * (size_t)k.K;
      HIPCHK(c, XS.gheap_d2.ensure(slots * 4));
      HIPCHK(c, XS.gheap_idx.ensure(slots * 4));
      a.gheap_d2 = XS.gheap_d2.as<float>();
      a.gheap_idx = XS.gheap_idx.as<int32_t>();
    }
    HIPCHK(c, hipEventRecord(X.ev0, X.st));
    launch_knn(a, X.st);
    HIPCHK(c, hipGetLastError());
    int rc = knn_end(c, X, ms);
    if (rc) return rc;
  }
  return GI_OK;
}

// run the k-NN estimate of one query list into out[slot] (Morton-ordered launch)
// the global list's slot layout (render_pixels): primary slots, tiled indirect slots with their
// query row masks, appends from qbase (gi_sort.h curve_order_rows)
struct ListRows {
  int64_t nprim;
  const uint64_t *qmask;
  int64_t trows;
  uint32_t qbase;
};

static int knn_list(gi_ctx *c, int mi, const float4 *qpos, const QShade *qshade, int64_t nq,
             double *out, double *ms, const ListRows *rows = nullptr, uint32_t qbase = 0,
             const uint32_t *app_order = nullptr) {
  MapExec &X = c->mx[mi];
  MapScratch &XS = c->s.map[mi];
  KnnArgs k = knn_args(c, mi);
  k.qpos = qpos;
  k.qshade = qshade;
  k.out = out;
  k.nq = nq;
  if (c->P.irradiance_cache && mi == GI_MAP_GLOBAL) {
    // the cached-radiance lookup runs thread per list slot (it reads no permutation)
    c->last_kind[mi] = 9;
    launch_cached(k, X.st);
    HIPCHK(c, hipGetLastError());
    return GI_OK;
  }
  {
    // only the valid queries are sorted and searched: the empty deterministic slots (indirect
    // paths absorbed, escaped, or whose continuation left no query; primaries without their own
    // query; Monte Carlo paths that deferred none) are ~46 % of C2's global list, and the
    // reduction never reads their outputs (their keys / row-mask bits mark them).
    uint32_t *perm = nullptr;
    if (rows && c->row_order && c->key_bits[mi] <= 10) {
      // compacted from the row masks: the empty slots are never read or sorted
      int64_t nv = 0;
      HIPCHK(c, curve_order_rows(qpos, rows->nprim, rows->qmask, rows->trows, rows->qbase, nq,
                                 c->sbmin, c->sbmax, XS.sorter, &perm, &nv, X.st,
                                 c->surf_key, app_order));
      nq = nv;
      k.nq = nv;
      if (nv == 0) return GI_OK;
    } else {
      int64_t nv = 0;
      HIPCHK(c, morton_order_valid(qpos, nq, c->sbmin, c->sbmax, XS.sorter, &perm, &nv, X.st,
                                   c->key_bits[mi], c->surf_key_c, qbase, app_order));
      nq = nv;
      k.nq = nv;
      if (nv == 0) return GI_OK;
    }
    k.perm = perm;
  }
  return run_knn(c, k, nq, ms);
}

// the rays (and ids) of the batch's npix pixels onto the device, in batch order: straight from
// the caller's buffer where the pixels are one row-major run (a full frame's batches), else
// gathered pixel by pixel first
static int upload_rays(gi_ctx *c, const RaySrc &R, const int32_t *pix_xy, int64_t npix, int w) {
  const size_t spp = (size_t)R.spp, n = (size_t)npix * spp;
  const size_t first = (size_t)pix_xy[1] * w + pix_xy[0];
  bool run = true;
  for (int64_t k = 1; k < npix && run; k++)
    run = (size_t)pix_xy[2 * k + 1] * w + pix_xy[2 * k] == first + (size_t)k;
  const gi_ray *rays = R.rays + first * spp;
  const uint64_t *ids = R.ids ? R.ids + first * spp : nullptr;
  if (!run) {
    c->s.ray_stage.resize(n);
    if (R.ids) c->s.id_stage.resize(n);
    for (int64_t k = 0; k < npix; k++) {
      const size_t src = ((size_t)pix_xy[2 * k + 1] * w + pix_xy[2 * k]) * spp;
      memcpy(&c->s.ray_stage[(size_t)k * spp], R.rays + src, spp * sizeof(gi_ray));
      if (R.ids) memcpy(&c->s.id_stage[(size_t)k * spp], R.ids + src, spp * 8);
    }
    rays = c->s.ray_stage.data();
    ids = R.ids ? c->s.id_stage.data() : nullptr;
  }
  HIPCHK(c, upload(c->s.d_rays, rays, n * sizeof(gi_ray), c->stream));
  if (ids) HIPCHK(c, upload(c->s.d_ray_ids, ids, n * 8, c->stream));
  return GI_OK;
}

// What the stages of one render_pixels batch share beside the batch's RenderArgs.
struct Batch {
  int64_t npix = 0, nprim = 0;   // output pixels and primary samples
  uint32_t trows = 0;            // rows of the indirect paths' tiled slots ...
  uint64_t tind = 0;             // ... and their entries, 64 per row (>= total_ind)
  uint64_t ind_full = 0;         // worst-case entries of one continuation-queue stripe
  McWave mwave;                  // breadth-first Monte Carlo schedule (rounds 0: another one runs)
  uint32_t qbase[2] = {0, 0};    // per list: the first append slot, behind the deterministic ones
  uint32_t nq[2] = {0, 0};       // per list: the slots the path pass filled
  int attempts_used = 0;         // path passes run
  bool timed = false;            // the caller wants the k-NN times ...
  double knn_ms[2] = {0, 0};     // ... of this batch, per map
  bool ran[2] = {false, false};  // the map's estimate was launched
};
constexpr int BATCH_RERUN = -1;  // primary_pass: the batch has to be run again with fewer pixels

// batch size: prim_per_batch primary samples, fewer when the query rate seen so far would
// exceed the query budget (the first batch of a scene starts at 1/8 to measure that rate)
static int64_t batch_pixels(const gi_ctx *c, int64_t per_pix, int64_t shrink, int64_t left) {
  int64_t prim_cap = c->prim_per_batch;
  if (c->q_per_prim > 0.0)
    prim_cap = std::min<int64_t>(prim_cap, (int64_t)(c->query_budget / c->q_per_prim));
  else
    prim_cap = std::max<int64_t>(1, prim_cap / 8);
  prim_cap = std::max<int64_t>(1, prim_cap / shrink);
  const int64_t pix_batch = std::max<int64_t>(1, prim_cap / per_pix);
  return std::min(pix_batch, left);
}

// The primary kernel, the scans of its path counts, the owner table and the indirect paths' tiles.
// Path slots are 32-bit: a batch whose paths (with the indirect tiles' padding) would not fit
// gets its counters put back and BATCH_RERUN (slot_limit: GI_SLOT_LIMIT, tests).
static int primary_pass(gi_ctx *c, RenderArgs &a, Batch &B) {
  const int64_t nprim = B.nprim;
  // counters before the primary kernel, restored if the batch is re-run smaller
  HIPCHK(c, hipMemcpyAsync(c->s.stats_bak.p, c->res.d_stats.p, ST_BYTES, hipMemcpyDeviceToDevice,
                           c->stream));
  launch_primary(a, c->stream);
  HIPCHK(c, hipGetLastError());
  ScanTemp t = scan_temp(c, nprim);
  HIPCHK(c, launch_scan(a.npaths, c->s.path_off.as<uint32_t>(), nprim, t, c->stream));
  HIPCHK(c, launch_scan(a.nmc, c->s.mc_off.as<uint32_t>(), nprim, t, c->stream));
  HIPCHK(c, launch_scan(a.nind, c->s.ind_off.as<uint32_t>(), nprim, t, c->stream));
  uint32_t totals[3] = {0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(&totals[0], c->s.path_off.as<uint32_t>() + nprim, 4,
                           hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&totals[1], c->s.mc_off.as<uint32_t>() + nprim, 4,
                           hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&totals[2], c->s.ind_off.as<uint32_t>() + nprim, 4,
                           hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  a.total_paths = totals[0];
  a.total_mc = totals[1];
  a.total_ind = totals[2];
  // owner tables: the path kernels find their waves' primary sample in one load
  if (a.total_mc > 0) {
    HIPCHK(c, c->s.mc_tab.ensure(((size_t)a.total_mc / 64 + 2) * 4));
    launch_owner_table(c->s.mc_off.as<uint32_t>(), nprim, c->s.mc_tab.as<uint32_t>(), c->stream);
    a.mc_tab = c->s.mc_tab.as<uint32_t>();
  }
  // the indirect paths' tiled slots (RenderArgs::ind_rows): rows per 64-primary tile, scanned
  const int64_t ntiles = (nprim + 63) / 64;
  HIPCHK(c, c->s.ind_trows.ensure((size_t)(ntiles + 1) * 4));
  HIPCHK(c, c->s.ind_rows.ensure((size_t)(ntiles + 1) * 4));
  launch_ind_tiles(a.nind, nprim, c->s.ind_trows.as<uint32_t>(), c->stream);
  HIPCHK(c, launch_scan(c->s.ind_trows.as<uint32_t>(), c->s.ind_rows.as<uint32_t>(), ntiles, t, c->stream));
  HIPCHK(c, hipMemcpyAsync(&B.trows, c->s.ind_rows.as<uint32_t>() + ntiles, 4, hipMemcpyDeviceToHost,
                           c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  B.tind = 64ull * B.trows;
  const uint64_t slot_limit = c->slot_limit > 0 ? (uint64_t)c->slot_limit : 0xFFFFFFF0ull;
  if ((uint64_t)a.total_paths + B.tind + (uint64_t)nprim > slot_limit) {
    if (B.npix == 1)
      return fail(c, GI_ERR_ALLOC, "one output pixel's samples need more than 2^32 path slots");
    HIPCHK(c, hipMemcpyAsync(c->res.d_stats.p, c->s.stats_bak.p, ST_BYTES, hipMemcpyDeviceToDevice,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BATCH_RERUN;
  }
  return GI_OK;
}

// The tiled slots' tables and base slots, the continuation queues, and the Monte Carlo paths'
// schedule (B.mwave, a.mc_next / a.mc_persist_blocks).
static int path_setup(gi_ctx *c, RenderArgs &a, Batch &B) {
  const int64_t ntiles = (B.nprim + 63) / 64;
  a.ind_rows = c->s.ind_rows.as<uint32_t>();
  a.ind_g0 = a.total_paths;
  a.tind = (int64_t)B.tind;
  HIPCHK(c, c->s.ind_tab.ensure(((size_t)B.trows + 1) * 8));
  launch_ind_row_tile(a.ind_rows, ntiles, c->s.ind_tab.as<uint64_t>(), c->stream);
  a.ind_row_info = c->s.ind_tab.as<uint64_t>();
  HIPCHK(c, c->s.ind_masks.ensure(((size_t)B.trows + 1) * 16));
  a.ind_qmask = c->s.ind_masks.as<uint64_t>();
  a.ind_bmask = a.ind_qmask + B.trows + 1;
  HIPCHK(c, c->s.base.ensure(((size_t)a.total_paths + B.tind) * 24));
  a.base = c->s.base.as<double>();
  // continuation queue: stripe s takes the appends of waves w with w % IND_QS == s (<= 64
  // paths per wave, so `full` entries per stripe can never overflow); sized from the fill
  // seen so far (c->ind_frac of full), re-run with more room when a stripe overflows
  B.ind_full = 64 * ((((uint64_t)a.tind + 63) / 64 + IND_QS - 1) / IND_QS);
  if (a.split_ind && a.total_ind > 0) HIPCHK(c, c->s.ind_ncont.ensure(IND_QS * 32 * 4));
  // Monte Carlo paths' indirect sub-paths: at most one per path, so the worst case is sized
  McWave &mwave = B.mwave;
  memset(&mwave, 0, sizeof mwave);
  if (a.split_ind && a.total_mc > 0 && a.F.indirect) {
    const uint64_t full = 64 * ((((uint64_t)a.total_mc + 63) / 64 + IND_QS - 1) / IND_QS);
    HIPCHK(c, c->s.mc_cont.ensure((size_t)IND_QS * full * sizeof(IndCont)));
    HIPCHK(c, c->s.mc_ncont.ensure(IND_QS * 32 * 4));
    a.mc_cont = c->s.mc_cont.as<IndCont>();
    a.mc_ncont = c->s.mc_ncont.as<uint32_t>();
    a.mc_cap_s = (uint32_t)full;
    // mc_persist_kernel (path counter in the spare qcount word): always with a grid given,
    // and by default (-1) where a bounce's direct light is a soft-shadow fan, the only case it
    // was measured faster (C3 +5.5 %; with hard lights the plain kernel wins: C2 -0.4 %, C4
    // -7.4 %, since the persistent waves hold every SIMD's registers while the indirect kernel
    // on the other stream waits)
    // Breadth first (GI_MC_WAVE): by number wherever the persistent kernel is
    // not asked for by number; by default (-1) 4 rounds for the class it was measured faster
    // on, hard lights over triangles and spheres only (C2 -2.0 %; 4 and 8 rounds measured the
    // same, 16 no better). Soft-light scenes keep the persistent kernel, the other hard-light
    // element sets (whose step kernels spill) mc_kernel.
    const bool wave_class = a.S.hard_lights && kinds_within(a.S.kinds, KINDS_TRI_SPHERE);
    const int rounds = c->mc_persist > 0 ? 0 : c->mc_wave >= 0 ? c->mc_wave : wave_class ? 4 : 0;
    if (rounds > 0) {
      HIPCHK(c, c->s.mc_wstate.ensure((size_t)a.total_mc * sizeof(McState)));
      HIPCHK(c, c->s.mc_wlist.ensure(2 * (size_t)a.total_mc * 4));
      HIPCHK(c, c->s.mc_wcount.ensure(((size_t)MC_WAVE_MAX_ROUNDS + 1) * 4));
      mwave.state = c->s.mc_wstate.as<McState>();
      mwave.list[0] = c->s.mc_wlist.as<uint32_t>();
      mwave.list[1] = mwave.list[0] + a.total_mc;
      mwave.count = c->s.mc_wcount.as<uint32_t>();
      mwave.rounds = rounds;
    } else if (c->mc_persist > 0 || (c->mc_persist < 0 && !a.S.hard_lights)) {
      a.mc_next = c->res.qcount.as<uint32_t>() + 2;
      a.mc_persist_blocks = c->mc_persist > 0 ? c->mc_persist : 1024;
    }
    if (c->mc_sub) {
      HIPCHK(c, c->s.mc_cont2.ensure((size_t)IND_QS * full * sizeof(IndCont)));
      HIPCHK(c, c->s.mc_ncont2.ensure(IND_QS * 32 * 4));
      a.mc_cont2 = c->s.mc_cont2.as<IndCont>();
      a.mc_ncont2 = c->s.mc_ncont2.as<uint32_t>();
    }
  }
  return GI_OK;
}

// single Monte Carlo pass; grow the query lists (and the continuation queue) and re-run on
// overflow, three attempts at the most; the rates the next batches are sized by follow it
static int path_pass(gi_ctx *c, RenderArgs &a, Batch &B) {
  const int64_t nprim = B.nprim;
  uint32_t *nq = B.nq, *qbase = B.qbase;
  nq[0] = nq[1] = 0;
  HIPCHK(c, hipMemcpyAsync(c->s.stats_bak.p, c->res.d_stats.p, ST_BYTES,
                           hipMemcpyDeviceToDevice, c->stream));
  // deterministic slots: [0, nprim) per primary sample, then (global list) the indirect
  // paths' tiled slots; Monte Carlo paths append after qbase[l]
  qbase[0] = (uint32_t)(nprim + B.tind);
  qbase[1] = (uint32_t)nprim;
  a.qind_base = nprim;
  // the empty tiled slots need their QMETA_NONE only where something reads every slot: the
  // global list's sort over all slots (no row masks: GI_ROW_ORDER=0, or no indirect paths in a
  // tiled batch) and the -cache lookup (thread per slot). C5 writes ~390 M of them per batch.
  a.tiled_skip = c->row_order && c->key_bits[0] <= 10 && !c->P.irradiance_cache && a.ind_qmask &&
                 (a.total_ind > 0 || B.tind == 0);
  for (int attempt = 0; attempt < 3; attempt++) {
    for (int l = 0; l < 2; l++) {
      // capacity: the largest list seen so far (+25 %), or this batch's primaries at the
      // largest per-primary rate seen (+25 %), so that a batch larger than the ones before (the
      // first full batch after the 1/8 probe, a batch where the scene fills more of the frame)
      // does not overflow and re-run its path pass; before any rate is known, the
      // deterministic slots plus 8 appends per primary
      size_t cap = std::max<size_t>(c->qcap_hint[l], (size_t)qbase[l] + 1024);
      if (attempt == 0) {
        // the deterministic slots are known (qbase); the appends come from the batch's
        // Monte Carlo paths, whose count is known too (total_mc): at the largest appends per
        // Monte Carlo path seen so far (at least 2), +25 %
        const double per_mc = std::max(2.0, c->mc_app_rate[l]);
        size_t pred = (size_t)qbase[l] + (size_t)(1.25 * per_mc * (double)a.total_mc) + 1024;
        cap = std::max(cap, std::min<size_t>(pred, 0xFFFFFFF0u));
      }
      HIPCHK(c, c->s.qpos[l].ensure(cap * 16));
      HIPCHK(c, c->s.qshade[l].ensure(cap * sizeof(QShade)));
      HIPCHK(c, c->s.qkey[l].ensure(cap * 8));
      a.qpos[l] = c->s.qpos[l].as<float4>();
      a.qshade[l] = c->s.qshade[l].as<QShade>();
      a.qkey[l] = c->s.qkey[l].as<uint64_t>();
      a.qcap[l] = (uint32_t)std::min<size_t>(cap, 0xFFFFFFF0u);
    }
    if (a.split_ind && a.total_ind > 0) {
      uint64_t cap_s = std::min<uint64_t>(B.ind_full, 64 * ((uint64_t)(B.ind_full * c->ind_frac) / 64 + 1));
      HIPCHK(c, c->s.ind_cont.ensure((size_t)IND_QS * cap_s * sizeof(IndCont)));
      a.ind_cap_s = (uint32_t)cap_s;
      a.ind_cont = c->s.ind_cont.as<IndCont>();
      a.ind_ncont = c->s.ind_ncont.as<uint32_t>();
    }
    a.qcount = c->res.qcount.as<uint32_t>();
    HIPCHK(c, hipMemcpyAsync(c->res.qcount.p, qbase, 8, hipMemcpyHostToDevice, c->stream));
    if (!a.tiled_skip && B.tind > (uint64_t)a.total_ind) launch_ind_pad(a, c->stream);  // (never when tind = 0)
    launch_path(a, c->stream, c->stream2, c->ev_fork, c->ev_join, true,
                B.mwave.rounds > 0 ? &B.mwave : nullptr);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(nq, c->res.qcount.p, 8, hipMemcpyDeviceToHost, c->stream));
    uint32_t fills[IND_QS * 32];
    if (a.split_ind && a.total_ind > 0)
      HIPCHK(c, hipMemcpyAsync(fills, c->s.ind_ncont.p, sizeof fills, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    B.attempts_used = attempt + 1;
    bool ok = nq[0] <= a.qcap[0] && nq[1] <= a.qcap[1];
    if (a.split_ind && a.total_ind > 0) {
      uint32_t mx = 0;
      for (int q = 0; q < IND_QS; q++) mx = std::max(mx, fills[q * 32]);
      c->ind_frac = std::max(c->ind_frac, std::min(1.0, 1.25 * mx / (double)B.ind_full));
      if (mx > a.ind_cap_s) ok = false;
    }
    for (int l = 0; l < 2; l++)
      c->qcap_hint[l] = std::max<size_t>(c->qcap_hint[l], (size_t)(nq[l] * 1.25) + 1024);
    c->q_per_prim = std::max(c->q_per_prim, (double)((uint64_t)nq[0] + nq[1]) / (double)nprim);
    if (a.total_mc > 0)
      for (int l = 0; l < 2; l++)
        c->mc_app_rate[l] = std::max(c->mc_app_rate[l], (double)(nq[l] - qbase[l]) / (double)a.total_mc);
    if (ok) break;
    if (attempt == 2) return fail(c, GI_ERR_ALLOC, "query list overflow");
    HIPCHK(c, hipMemcpyAsync(c->res.d_stats.p, c->s.stats_bak.p, ST_BYTES,
                             hipMemcpyDeviceToDevice, c->stream));
  }
  return GI_OK;
}

// photon-map estimates of the two lists into qout[l] (zeros where the map is not valid)
static int estimates(gi_ctx *c, RenderArgs &a, Batch &B) {
  const uint32_t *nq = B.nq;
  bool *run = B.ran;
  for (int l = 0; l < 2; l++) {
    run[l] = false;
    a.nq[l] = nq[l];
    a.qapp[l] = B.qbase[l];
    a.qout[l] = nullptr;
    if (nq[l]) {
      HIPCHK(c, c->s.qout[l].ensure((size_t)nq[l] * 24));
      a.qout[l] = c->s.qout[l].as<double>();
      if (!c->map_valid[l])
        HIPCHK(c, hipMemsetAsync(c->s.qout[l].p, 0, (size_t)nq[l] * 24, c->stream));
      else
        run[l] = true;
    }
  }
  // the two maps' estimates, one after the other on the render stream (running the caustic
  // one in a worker thread on a second stream measured no faster: r02)
  for (int l = 0; l < 2; l++) {
    if (!run[l]) continue;
    // the global list's launch order from its row masks (GI_ROW_ORDER, default on)
    ListRows lr{B.nprim, a.ind_qmask, (int64_t)(B.tind / 64), B.qbase[0]};
    const bool use_rows = l == 0 && a.ind_qmask && (a.total_ind > 0 || B.tind == 0);
    int rc = knn_list(c, l, a.qpos[l], a.qshade[l], nq[l], c->s.qout[l].as<double>(),
                      B.timed ? &B.knn_ms[l] : nullptr, use_rows ? &lr : nullptr, B.qbase[l],
                      a.sslot[l]);
    if (rc) return rc;
  }
  return GI_OK;
}

// A deterministic order of each list for the reduction. The deterministic slots (a primary's own
// query at slot b; its indirect paths' at tiled slots) are located by (primary, slot-in-primary);
// only the Monte Carlo appends after qbase[l] are key-sorted and indexed per primary (CSR over
// the sorted keys).
static int order_appends(gi_ctx *c, RenderArgs &a, Batch &B) {
  const int64_t nprim = B.nprim;
  for (int l = 0; l < 2; l++) {
    HIPCHK(c, c->s.qseg[l].ensure((size_t)(nprim + 1) * 4));
    a.qseg[l] = c->s.qseg[l].as<uint32_t>();
    const int64_t napp = (int64_t)B.nq[l] - (int64_t)B.qbase[l];
    if (napp <= 0) {  // no appends: empty segments for every primary
      HIPCHK(c, hipMemsetAsync(c->s.qseg[l].p, 0, (size_t)(nprim + 1) * 4, c->stream));
      a.skey[l] = nullptr;
      a.sslot[l] = nullptr;
      continue;
    }
    uint64_t *sk = nullptr;
    uint32_t *ss = nullptr;
    // keys: primary << 32 | slot in primary << 16 | query in path (empty slots: ~0)
    int bits = 32;
    while (bits < 64 && ((uint64_t)nprim >> (bits - 32)) != 0) bits++;
    if (bits < 64) bits++;  // room for the empty-slot key's top bits
    HIPCHK(c, key_order(a.qkey[l] + B.qbase[l], napp, bits, c->s.keysort[l], &sk, &ss, c->stream));
    a.skey[l] = sk;
    a.sslot[l] = ss;  // slots relative to qbase[l]
    launch_segments(sk, (uint32_t)napp, (uint32_t)nprim, a.qseg[l], c->stream);
    HIPCHK(c, hipGetLastError());
  }
  return GI_OK;
}

// the batch's pixels into the frame's images and, while rad_on, into the radiance frame (while
// lay_on too, into the layer frames)
static int reduce(gi_ctx *c, RenderArgs &a, Batch &B) {
  a.rgbf = c->s.rgbf.as<float>();
  a.rgb8 = c->s.rgb8.as<uint8_t>();
  HIPCHK(c, c->s.prim_rgb.ensure((size_t)B.nprim * 24));
  a.prim_rgb = c->s.prim_rgb.as<double>();
  launch_reduce(a, c->stream);
  HIPCHK(c, hipGetLastError());
  if (c->rad_on) {  // the same primaries once more, unclamped (gi_radiance.hip)
    RadianceArgs ra;
    memset(&ra, 0, sizeof ra);
    ra.prim_rgb = a.prim_rgb;
    ra.pixels = a.pixels;
    ra.npix = a.npix;
    ra.S = a.spp ? a.spp : a.af * a.af;
    ra.dof_test = a.dof_test;
    ra.out_w = a.out_w;
    ra.bw = a.spp ? 1.0 / a.spp : 1.0 / a.af / a.af;
    ra.frame = c->s.rad_frame.as<double>();
    ra.samples = c->rad_want_samples ? c->s.rad_samples.as<double>() : nullptr;
    launch_reduce_radiance(ra, c->stream);
    HIPCHK(c, hipGetLastError());
    if (c->lay_on) {
      // the same terms once more, summed per group, then the radiance reduction per layer plane
      HIPCHK(c, c->s.prim_layers.ensure((size_t)GI_LAYER_COUNT * B.nprim * 24));
      double *pl = c->s.prim_layers.as<double>();
      hipEvent_t e0 = nullptr, e1 = nullptr;
      if (c->lay_time) {
        HIPCHK(c, hipEventCreate(&e0));
        if (hipEventCreate(&e1) != hipSuccess) {
          hipEventDestroy(e0);
          return fail(c, GI_ERR_HIP, "layers: hipEventCreate failed");
        }
        (void)hipEventRecord(e0, c->stream);
      }
      launch_reduce_layers(a, pl, c->stream);
      hipError_t le = hipGetLastError();
      if (c->lay_time) {
        (void)hipEventRecord(e1, c->stream);
        float ms = 0.f;
        if (le == hipSuccess) le = hipEventSynchronize(e1);
        if (le == hipSuccess) le = hipEventElapsedTime(&ms, e0, e1);
        c->lay_ms += ms;
        hipEventDestroy(e0);
        hipEventDestroy(e1);
      }
      HIPCHK(c, le);
      for (int l = 0; l < GI_LAYER_COUNT; l++) {
        ra.prim_rgb = pl + (size_t)l * 3 * B.nprim;
        ra.frame = c->s.lay_frame.as<double>() + (size_t)l * c->lay_npix * 6;
        ra.samples = c->rad_want_samples
                         ? c->s.lay_samples.as<double>() + (size_t)l * c->lay_npix * (size_t)ra.S * 3
                         : nullptr;
        launch_reduce_radiance(ra, c->stream);
        HIPCHK(c, hipGetLastError());
      }
    }
  }
  return GI_OK;
}

// render the given output pixels into the device image buffers (rsrc: their primary rays come
// from the caller instead of the camera, aa is then unused), batch by batch through the stages
// above
static int render_pixels(gi_ctx *c, int aa, int w, int h, const std::vector<int32_t> &pix_xy,
                         gi_render_stats *rs, const RaySrc *rsrc = nullptr) {
  const gi_params &P = c->P;
  int af = rsrc ? 1 : 1 << aa;
  int dof = rsrc ? 1 : std::max(1, P.dof_test);
  int64_t per_pix = rsrc ? (int64_t)rsrc->spp : (int64_t)af * af * dof;
  int64_t npix_total = (int64_t)pix_xy.size() / 2;
  double knn_ms[2] = {0, 0}, launches[2] = {0, 0};
  HIPCHK(c, upload(c->s.pixels, pix_xy.data(), pix_xy.size() * 4, c->stream));
  HIPCHK(c, c->res.qcount.ensure(16));
  HIPCHK(c, c->s.stats_bak.ensure(ST_BYTES));
  // a batch that primary_pass sends back is re-run at half the primary samples, as often as needed
  int64_t shrink = 1;
  int64_t nbatch = 0;
  for (int64_t p0 = 0, npix = 0; p0 < npix_total; p0 += npix) {
    auto tb0 = std::chrono::steady_clock::now();
    Batch B;
    B.timed = rs != nullptr;
    B.npix = npix = batch_pixels(c, per_pix, shrink, npix_total - p0);
    const int64_t nprim = B.nprim = npix * per_pix;
    RenderArgs a;
    memset(&a, 0, sizeof a);
    a.S = make_view(c);
    a.F = make_flags(P);
    a.pixels = c->s.pixels.as<int2>() + p0;
    a.npix = (int)npix;
    a.af = af;
    a.W = w * af;
    a.H = h * af;
    a.dof_test = dof;
    a.out_w = w;
    a.nprim = nprim;
    a.stats = c->res.d_stats.as<unsigned long long>();
    a.split_ind = c->split_ind;
    a.dbg = c->render_dbg;
    HIPCHK(c, c->s.spawn.ensure((size_t)nprim * sizeof(Spawn)));
    HIPCHK(c, c->s.npaths.ensure((size_t)nprim * 4));
    HIPCHK(c, c->s.path_off.ensure((size_t)(nprim + 1) * 4));
    HIPCHK(c, c->s.nmc.ensure((size_t)nprim * 4));
    HIPCHK(c, c->s.mc_off.ensure((size_t)(nprim + 1) * 4));
    HIPCHK(c, c->s.nind.ensure((size_t)nprim * 4));
    HIPCHK(c, c->s.ind_off.ensure((size_t)(nprim + 1) * 4));
    a.spawn = c->s.spawn.as<Spawn>();
    a.npaths = c->s.npaths.as<uint32_t>();
    a.nmc = c->s.nmc.as<uint32_t>();
    a.nind = c->s.nind.as<uint32_t>();
    a.path_off = c->s.path_off.as<uint32_t>();
    a.mc_off = c->s.mc_off.as<uint32_t>();
    a.ind_off = c->s.ind_off.as<uint32_t>();
    if (rsrc) {
      // this batch's slice only (a C2-sized frame's 16.8 M rays are 0.94 GB)
      auto tu0 = std::chrono::steady_clock::now();
      int rc = upload_rays(c, *rsrc, pix_xy.data() + 2 * p0, npix, w);
      if (rc) return rc;
      a.spp = rsrc->spp;
      set_ray_slice(a, RaySlice{c->s.d_rays.as<gi_ray_dev>(),
                                rsrc->ids ? c->s.d_ray_ids.as<uint64_t>() : nullptr});
      if (c->batch_log) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        fprintf(stderr, "[gi] batch %lld: ray upload %lld rays, %.2f ms\n", (long long)nbatch,
                (long long)nprim,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tu0).count());
      }
    }
    int rc = primary_pass(c, a, B);
    if (rc == BATCH_RERUN) {
      shrink *= 2;
      c->batch_reruns++;
      npix = 0;  // same pixels again, half as many per batch
      continue;
    }
    if (!rc) rc = path_setup(c, a, B);
    if (!rc) rc = path_pass(c, a, B);
    // (the appends' key order first: it also fixes their place in the k-NN launch order)
    if (!rc) rc = order_appends(c, a, B);
    if (!rc) rc = estimates(c, a, B);
    if (!rc) rc = reduce(c, a, B);
    if (rc) return rc;
    for (int l = 0; l < 2; l++) {
      knn_ms[l] += B.knn_ms[l];
      if (B.ran[l]) launches[l]++;
    }
    if (c->progress) c->progress(0, (double)(p0 + npix) / (double)npix_total, c->progress_user);
    if (c->batch_log) {  // GI_LOG & 2: one stderr line per batch (synchronises the batch)
      HIPCHK(c, hipStreamSynchronize(c->stream));
      double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count();
      fprintf(stderr, "[gi] batch %lld: pixels %lld primaries %lld paths %u tiled %llu mc %lld "
              "queries %u + %u, path passes %d, %.1f ms\n", (long long)nbatch, (long long)npix,
              (long long)nprim, (uint32_t)a.total_paths, (unsigned long long)B.tind, (long long)a.total_mc,
              B.nq[0], B.nq[1], B.attempts_used, ms);
    }
    nbatch++;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (rs) {
    for (int l = 0; l < 2; l++) {
      rs->knn_map_kernel_ms[l] += knn_ms[l];
      rs->knn_map_launches[l] += launches[l];
      rs->knn_kernel_ms += knn_ms[l];
      rs->knn_kernel_launches += launches[l];
    }
  }
  return GI_OK;
}

int render_common(gi_ctx *c, int aa, int w, int h, const std::vector<int32_t> &pix, uint8_t *rgb8,
                  float *rgbf, gi_render_stats *st, bool keep_rgbf, const RaySrc *rsrc) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (aa < 0 || w <= 0 || h <= 0) return fail(c, GI_ERR_ARG, "bad image size");
  auto t0 = std::chrono::steady_clock::now();
  size_t npx = (size_t)w * h * 3;
  HIPCHK(c, c->s.rgbf.ensure(npx * 4));
  HIPCHK(c, c->s.rgb8.ensure(npx));
  // the frame's device images (the caller's floats kept, or cleared), the counters and the
  // k-NN pass counters, as they are before a frame's first batch
  auto reset_frame = [&]() -> int {
    if (keep_rgbf && rgbf) {
      HIPCHK(c, hipMemcpyAsync(c->s.rgbf.p, rgbf, npx * 4, hipMemcpyHostToDevice, c->stream));
    } else {
      HIPCHK(c, hipMemsetAsync(c->s.rgbf.p, 0, npx * 4, c->stream));
    }
    HIPCHK(c, hipMemsetAsync(c->s.rgb8.p, 0, npx, c->stream));
    HIPCHK(c, hipMemsetAsync(c->res.d_stats.p, 0, ST_BYTES, c->stream));
    c->fb_ms[0] = c->fb_ms[1] = 0;
    c->fb_q[0] = c->fb_q[1] = 0;
    c->p2_ms[0] = c->p2_ms[1] = 0;
    c->p2_q[0] = c->p2_q[1] = 0;
    return GI_OK;
  };
  rc = reset_frame();
  if (rc) return rc;
  c->last_kind[0] = c->last_kind[1] = -1;
  gi_render_stats local;
  unsigned long long s[ST_COUNT];
  for (int pass = 0;; pass++) {
    memset(&local, 0, sizeof local);
    rc = render_pixels(c, aa, w, h, pix, &local, rsrc);
    if (rc) return rc;
    HIPCHK(c, read_stats(c, s));
    if (s[ST_GEN_MISS] == 0) break;
    // a k-NN instance without the general estimate form (KnnArgs::general == 0, knn_general)
    // met a query that needed it and wrote NaN: the host's material check missed a query site.
    // Render again with the general instances only (kept for this context), never return NaN.
    if (pass > 0 || c->knn_general_mode > 0)
      return fail(c, GI_ERR_STATE, "k-NN estimate: general-form query in a general instance");
    fprintf(stderr, "[gi] %llu k-NN queries needed the general estimate form; re-rendering with "
            "the general k-NN instances\n", s[ST_GEN_MISS]);
    c->knn_general_mode = 1;
    rc = reset_frame();
    if (rc) return rc;
  }
  if (rgbf) HIPCHK(c, hipMemcpyAsync(rgbf, c->s.rgbf.p, npx * 4, hipMemcpyDeviceToHost, c->stream));
  if (rgb8) HIPCHK(c, hipMemcpyAsync(rgb8, c->s.rgb8.p, npx, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  log_phase_cycles(c, s);
  if (st) {
    st->screen_rays = s[ST_RAY];
    st->shadow_rays = s[ST_SHADOW];
    st->monte_carlo_rays = s[ST_MONTE];
    st->transmissive_samples = s[ST_TRANS];
    st->specular_samples = s[ST_SPEC];
    st->indirect_samples = s[ST_INDIRECT];
    st->caustic_samples = s[ST_CAUSTIC];
    for (int m = 0; m < 2; m++) {
      st->knn_map_queries[m] = s[ST_KNN + m * ST_KNN_MAP];
      st->knn_map_photons[m] = s[ST_KNN_PHOTONS + m * ST_KNN_MAP];
      st->knn_map_visited[m] = s[ST_KNN_VISITED + m * ST_KNN_MAP];
      st->knn_map_kernel_ms[m] = local.knn_map_kernel_ms[m];
      st->knn_map_launches[m] = local.knn_map_launches[m];
      st->knn_map_fallback_ms[m] = c->fb_ms[m];
      st->knn_map_fallback_queries[m] = c->fb_q[m];
      st->knn_map_pass2_ms[m] = c->p2_ms[m];
      st->knn_map_pass2_queries[m] = c->p2_q[m];
      st->knn_map_kind[m] = c->last_kind[m];
    }
    st->knn_queries = st->knn_map_queries[0] + st->knn_map_queries[1];
    st->knn_photons = st->knn_map_photons[0] + st->knn_map_photons[1];
    st->knn_visited = st->knn_map_visited[0] + st->knn_map_visited[1];
    st->knn_kernel_ms = local.knn_kernel_ms;
    st->knn_kernel_launches = local.knn_kernel_launches;
    st->render_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  return GI_OK;
}

// output pixels of the tiles (tile x tile, row-major tile id t = ty * tx + tx_i) that shard owns:
// tile (tx_i, ty_i) goes to shard (tx_i + ty_i) % nshards, a diagonal deal, so every run of
// nshards tiles along a row or a column meets every shard (t % nshards with tx a multiple of
// nshards deals whole tile columns, and a compact expensive region -- the glass sphere -- then
// lands on a few shards in proportion to the columns it spans)
static std::vector<int32_t> shard_pixels(int w, int h, int tile, int shard, int nshards) {
  int tx = (w + tile - 1) / tile, ty = (h + tile - 1) / tile;
  std::vector<int32_t> pix;
  for (int t = 0; t < tx * ty; t++) {
    if (((t % tx) + (t / tx)) % nshards != shard) continue;
    int x0 = (t % tx) * tile, y0 = (t / tx) * tile;
    for (int y = y0; y < std::min(h, y0 + tile); y++)
      for (int x = x0; x < std::min(w, x0 + tile); x++) {
        pix.push_back(x);
        pix.push_back(y);
      }
  }
  return pix;
}

// RenderImage on a device set: device k renders the 16x16 output tiles of
// shard k (shard_pixels: the reference's column interleave, render.cpp:90, re-cut as diagonally
// dealt tiles), packs its
// pixels (16 B each) and sends them to the first device: ncclSend / ncclRecv in one group over
// xGMI when the devices are distinct (each peer's stream feeds its own link into device 0), a
// peer copy otherwise. Device 0 scatters them into the image; nothing else is exchanged.
static int render_multi(gi_ctx *c, int aa, int w, int h, uint8_t *rgb8, float *rgbf,
                        gi_render_stats *st, const RaySrc *rsrc = nullptr) {
  const int nd = 1 + (int)c->peers.size();
  const int tile = 16;
  auto t0 = std::chrono::steady_clock::now();
  std::vector<std::vector<int32_t>> pix(nd);
  std::vector<gi_render_stats> ls(nd);
  for (int k = 0; k < nd; k++) {
    pix[k] = shard_pixels(w, h, tile, k, nd);
    memset(&ls[k], 0, sizeof ls[k]);
  }
  int rc = on_devices(c, [&](int k, gi_ctx *d) -> int {
    int r = render_common(d, aa, w, h, pix[k], nullptr, nullptr, &ls[k], false, rsrc);
    if (r || k == 0) return r;
    const int64_t n = (int64_t)pix[k].size() / 2;
    HIPCHK(d, d->s.pack.ensure((size_t)n * 16));
    launch_pack_pixels(d->s.pixels.as<int32_t>(), n, w, d->s.rgbf.as<float>(), d->s.rgb8.as<uint8_t>(),
                       d->s.pack.p, d->stream);
    HIPCHK(d, hipGetLastError());
    HIPCHK(d, hipStreamSynchronize(d->stream));
    return (int)GI_OK;
  });
  if (rc) return rc;
  auto tg = std::chrono::steady_clock::now();
  if ((int)c->s.recv.size() < nd) c->s.recv.resize(nd);
  if ((int)c->s.peer_pix.size() < nd) c->s.peer_pix.resize(nd);
  for (int k = 1; k < nd; k++) {
    const int64_t n = (int64_t)pix[k].size() / 2;
    HIPCHK(c, c->s.recv[k].ensure((size_t)n * 16));
    HIPCHK(c, upload(c->s.peer_pix[k], pix[k].data(), pix[k].size() * 4, c->stream));
  }
  if (!c->comms.empty()) {
    ncclResult_t r = g_rccl.groupStart();
    for (int k = 1; k < nd && r == ncclSuccess; k++) {
      const size_t bytes = pix[k].size() / 2 * 16;
      gi_ctx *d = c->peers[k - 1];
      r = g_rccl.send(d->s.pack.p, bytes, ncclUint8, 0, c->comms[k], d->stream);
      if (r == ncclSuccess) r = g_rccl.recv(c->s.recv[k].p, bytes, ncclUint8, k, c->comms[0], c->stream);
    }
    ncclResult_t r2 = g_rccl.groupEnd();
    if (r != ncclSuccess || r2 != ncclSuccess)
      return fail(c, GI_ERR_HIP, std::string("RCCL tile gather: ") +
                                     g_rccl.errString(r != ncclSuccess ? r : r2));
  } else {
    for (int k = 1; k < nd; k++) {
      gi_ctx *d = c->peers[k - 1];
      HIPCHK(c, hipMemcpyPeerAsync(c->s.recv[k].p, c->device, d->s.pack.p, d->device,
                                   pix[k].size() / 2 * 16, c->stream));
    }
  }
  for (int k = 1; k < nd; k++)
    launch_unpack_pixels(c->s.peer_pix[k].as<int32_t>(), (int64_t)pix[k].size() / 2, w,
                         c->s.recv[k].p, c->s.rgbf.as<float>(), c->s.rgb8.as<uint8_t>(), c->stream);
  HIPCHK(c, hipGetLastError());
  const size_t npx = (size_t)w * h * 3;
  if (rgbf) HIPCHK(c, hipMemcpyAsync(rgbf, c->s.rgbf.p, npx * 4, hipMemcpyDeviceToHost, c->stream));
  if (rgb8) HIPCHK(c, hipMemcpyAsync(rgb8, c->s.rgb8.p, npx, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (st) {
    memset(st, 0, sizeof *st);
    for (int k = 0; k < nd; k++) {
      const gi_render_stats &a = ls[k];
      st->screen_rays += a.screen_rays; st->shadow_rays += a.shadow_rays;
      st->monte_carlo_rays += a.monte_carlo_rays; st->transmissive_samples += a.transmissive_samples;
      st->specular_samples += a.specular_samples; st->indirect_samples += a.indirect_samples;
      st->caustic_samples += a.caustic_samples; st->knn_queries += a.knn_queries;
      st->knn_photons += a.knn_photons; st->knn_visited += a.knn_visited;
      st->knn_kernel_ms += a.knn_kernel_ms; st->knn_kernel_launches += a.knn_kernel_launches;
      for (int m = 0; m < 2; m++) {
        st->knn_map_queries[m] += a.knn_map_queries[m];
        st->knn_map_photons[m] += a.knn_map_photons[m];
        st->knn_map_visited[m] += a.knn_map_visited[m];
        st->knn_map_kernel_ms[m] += a.knn_map_kernel_ms[m];
        st->knn_map_launches[m] += a.knn_map_launches[m];
        st->knn_map_fallback_ms[m] += a.knn_map_fallback_ms[m];
        st->knn_map_fallback_queries[m] += a.knn_map_fallback_queries[m];
        st->knn_map_pass2_ms[m] += a.knn_map_pass2_ms[m];
        st->knn_map_pass2_queries[m] += a.knn_map_pass2_queries[m];
        if (k == 0) st->knn_map_kind[m] = a.knn_map_kind[m];
      }
      st->device_render_s_max = k ? std::max(st->device_render_s_max, a.render_s) : a.render_s;
      st->device_render_s_min = k ? std::min(st->device_render_s_min, a.render_s) : a.render_s;
    }
    const auto t1 = std::chrono::steady_clock::now();
    st->gather_s = std::chrono::duration<double>(t1 - tg).count();
    st->render_s = std::chrono::duration<double>(t1 - t0).count();
  }
  return GI_OK;
}

// full frame on the context's device or device set, from the camera or from a ray source
int render_frame(gi_ctx *c, int aa, int w, int h, uint8_t *rgb8, float *rgbf, gi_render_stats *st,
                 const RaySrc *rsrc) {
  hipSetDevice(c->device);
  int rc = check_ready(c);
  if (rc) return rc;
  if (aa < 0 || w <= 0 || h <= 0) return fail(c, GI_ERR_ARG, "bad image size");
  if (!c->peers.empty()) return render_multi(c, aa, w, h, rgb8, rgbf, st, rsrc);
  std::vector<int32_t> pix((size_t)w * h * 2);
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      pix[2 * ((size_t)y * w + x)] = x;
      pix[2 * ((size_t)y * w + x) + 1] = y;
    }
  return render_common(c, aa, w, h, pix, rgb8, rgbf, st, false, rsrc);
}

}  // namespace gi_internal

// =======================================================================================
// C-ABI
// =======================================================================================
extern "C" {

// RenderImage, render.cpp:155-259
int gi_render_image(gi_ctx *c, int aa, int w, int h, uint8_t *rgb8, float *rgbf,
                    gi_render_stats *st) {
  if (!c) return GI_ERR_ARG;
  return render_frame(c, aa, w, h, rgb8, rgbf, st, nullptr);
}

int gi_render_rays(gi_ctx *c, int w, int h, int spp, const gi_ray *rays, const uint64_t *ids,
                   uint8_t *rgb8, float *rgbf, gi_render_stats *st) {
  if (!c) return GI_ERR_ARG;
  if (!rays) return fail(c, GI_ERR_ARG, "null ray buffer");
  if (spp < 1) return fail(c, GI_ERR_ARG, "spp must be at least 1");
  if (w <= 0 || h <= 0) return fail(c, GI_ERR_ARG, "bad image size");
  if ((int64_t)w * h >= ((int64_t)1 << 31) / spp + (((int64_t)1 << 31) % spp != 0))
    return fail(c, GI_ERR_ARG, "width * height * spp must be below 2^31");
  const RaySrc src{rays, ids, spp};
  return render_frame(c, 0, w, h, rgb8, rgbf, st, &src);
}

int gi_camera_rays(gi_ctx *c, int aa, int w, int h, gi_ray *rays, uint64_t *ids, int64_t cap,
                   int64_t *n) {
  if (!c || !n) return GI_ERR_ARG;
  hipSetDevice(c->device);
  int rc = check_ready(c);
  if (rc) return rc;
  if (aa < 0 || aa > 15 || w <= 0 || h <= 0) return fail(c, GI_ERR_ARG, "bad image size");
  const gi_params &P = c->P;
  const int af = 1 << aa, dof = std::max(1, P.dof_test);
  const int64_t total = (int64_t)w * h * af * af * dof;
  *n = total;
  if (!rays) return GI_OK;
  if (cap < total) return fail(c, GI_ERR_ARG, "ray buffer holds fewer rays than the frame");
  CameraRaysArgs a;
  memset(&a, 0, sizeof a);
  a.cam = make_view(c).cam;
  a.seed = P.seed;
  a.dof = P.depth_of_field;
  a.dof_test = dof;
  a.af = af;
  a.W = w * af;
  a.H = h * af;
  a.out_w = w;
  const int64_t chunk = (int64_t)1 << 22;  // 224 MB of rays and ids at a time
  HIPCHK(c, c->s.d_rays.ensure((size_t)std::min(chunk, total) * sizeof(gi_ray)));
  HIPCHK(c, c->s.d_ray_ids.ensure((size_t)std::min(chunk, total) * 8));
  a.rays = c->s.d_rays.as<gi_ray_dev>();
  a.ids = c->s.d_ray_ids.as<uint64_t>();
  for (int64_t s0 = 0; s0 < total; s0 += chunk) {
    a.first = s0;
    a.n = std::min(chunk, total - s0);
    launch_camera_rays(a, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(rays + s0, c->s.d_rays.p, (size_t)a.n * sizeof(gi_ray),
                             hipMemcpyDeviceToHost, c->stream));
    if (ids)
      HIPCHK(c, hipMemcpyAsync(ids + s0, c->s.d_ray_ids.p, (size_t)a.n * 8, hipMemcpyDeviceToHost,
                               c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return GI_OK;
}

int gi_render_tiles(gi_ctx *c, int aa, int w, int h, int tile, int shard, int nshards,
                    float *rgbf, gi_render_stats *st) {
  if (!c || tile <= 0 || nshards <= 0 || shard < 0 || shard >= nshards || !rgbf) return GI_ERR_ARG;
  hipSetDevice(c->device);
  std::vector<int32_t> pix = shard_pixels(w, h, tile, shard, nshards);
  return render_common(c, aa, w, h, pix, nullptr, rgbf, st, true);
}

// One rank's shard, left on the device and packed (torchrun: each rank gathers these buffers to
// rank 0 over RCCL and rank 0 composes them with gi_compose_tiles; nothing else crosses).
int gi_render_tiles_packed(gi_ctx *c, int aa, int w, int h, int tile, int shard, int nshards,
                           void *packed, int64_t cap, int64_t *npix, gi_render_stats *st) {
  if (!c || !npix || tile <= 0 || nshards <= 0 || shard < 0 || shard >= nshards || w <= 0 || h <= 0)
    return GI_ERR_ARG;
  DeviceScope dev(c->device);
  std::vector<int32_t> pix = shard_pixels(w, h, tile, shard, nshards);
  const int64_t n = (int64_t)pix.size() / 2;
  *npix = n;
  if (!packed) return GI_OK;
  if (cap < n) return fail(c, GI_ERR_ARG, "packed buffer holds fewer pixels than the shard");
  if (!c->peers.empty()) return fail(c, GI_ERR_STATE, "packed shards are for one-device contexts");
  int rc = render_common(c, aa, w, h, pix, nullptr, nullptr, st, false);
  if (rc) return rc;
  launch_pack_pixels(c->s.pixels.as<int32_t>(), n, w, c->s.rgbf.as<float>(), c->s.rgb8.as<uint8_t>(),
                     packed, c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GI_OK;
}

int gi_compose_tiles(gi_ctx *c, int w, int h, int tile, int nshards, const void *packed,
                     int64_t stride, uint8_t *rgb8, float *rgbf) {
  if (!c || !packed || tile <= 0 || nshards <= 0 || w <= 0 || h <= 0) return GI_ERR_ARG;
  DeviceScope dev(c->device);
  const size_t npx = (size_t)w * h * 3;
  HIPCHK(c, c->s.rgbf.ensure(npx * 4));
  HIPCHK(c, c->s.rgb8.ensure(npx));
  if ((int)c->s.peer_pix.size() < nshards) c->s.peer_pix.resize(nshards);
  for (int s = 0; s < nshards; s++) {
    std::vector<int32_t> pix = shard_pixels(w, h, tile, s, nshards);
    const int64_t n = (int64_t)pix.size() / 2;
    if (n > stride) return fail(c, GI_ERR_ARG, "packed stride smaller than a shard");
    HIPCHK(c, upload(c->s.peer_pix[s], pix.data(), pix.size() * 4, c->stream));
    launch_unpack_pixels(c->s.peer_pix[s].as<int32_t>(), n, w,
                         (const uint8_t *)packed + (size_t)s * stride * 16, c->s.rgbf.as<float>(),
                         c->s.rgb8.as<uint8_t>(), c->stream);
    HIPCHK(c, hipGetLastError());
  }
  if (rgbf) HIPCHK(c, hipMemcpyAsync(rgbf, c->s.rgbf.p, npx * 4, hipMemcpyDeviceToHost, c->stream));
  if (rgb8) HIPCHK(c, hipMemcpyAsync(rgb8, c->s.rgb8.p, npx, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GI_OK;
}

int gi_quantize(int w, int h, const float *rgbf, uint8_t *rgb8) {
  if (!rgbf || !rgb8) return GI_ERR_ARG;
  for (size_t i = 0; i < (size_t)w * h * 3; i++) rgb8[i] = (uint8_t)(255 * (double)rgbf[i]);
  return GI_OK;
}

}  // extern "C"
