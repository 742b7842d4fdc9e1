// gi_probe.cpp -- kernel benchmarks and the test seams of include/gi.h.
#include <cfloat>
#include <cmath>
#include "gi_ctx.h"
#include "gi_radiance.h"

extern "C" {

// Diagnostics: the three kernels on a synthetic frame (every primary sum the same finite value:
// none of them branches on data), each launch between two HIP events. Buffers of its own, freed
// on return: the context's accumulator is untouched.
int gi_radiance_bench(gi_ctx *c, int aa, int w, int h, int warmup, int reps, double *reduce_ms,
                      double *merge_ms, double *noise_ms) {
  if (!c) return GI_ERR_ARG;
  if (aa < 0 || aa > 15 || w <= 0 || h <= 0 || warmup < 0 || reps < 1 || reps > 10000)
    return fail(c, GI_ERR_ARG, "radiance bench: bad size or repetition count");
  const int64_t S = (int64_t)1 << (2 * aa);
  const size_t npix = (size_t)w * h;
  if ((int64_t)npix >= ((int64_t)1 << 31) / S) return fail(c, GI_ERR_ARG, "radiance bench: frame too large");
  DeviceScope dev(c->device);
  std::vector<int32_t> pix(npix * 2);
  for (size_t p = 0; p < npix; p++) {
    pix[2 * p] = (int32_t)(p % w);
    pix[2 * p + 1] = (int32_t)(p / w);
  }
  DBuf prim, pixels, frame, acc, cnt, part;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  const size_t nb = (npix + NOISE_BLOCK - 1) / NOISE_BLOCK;
  auto run = [&]() -> hipError_t {
    hipError_t e;
    if ((e = prim.ensure(npix * (size_t)S * 24)) != hipSuccess) return e;
    if ((e = upload(pixels, pix.data(), pix.size() * 4, c->stream)) != hipSuccess) return e;
    if ((e = frame.ensure(npix * 48)) != hipSuccess) return e;
    if ((e = acc.ensure(npix * 48)) != hipSuccess) return e;
    if ((e = part.ensure(nb * 8)) != hipSuccess) return e;
    if ((e = cnt.ensure(npix * 8)) != hipSuccess) return e;
    // counts of bytes 0x01 (7.2e16 samples): the merge's general branch, the noise's n >= 2
    if ((e = hipMemsetAsync(cnt.p, 0x01, npix * 8, c->stream)) != hipSuccess) return e;
    // bytes 0x3f: every double is 4.7e-4
    if ((e = hipMemsetAsync(prim.p, 0x3f, npix * (size_t)S * 24, c->stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(acc.p, 0, npix * 48, c->stream)) != hipSuccess) return e;
    if ((e = hipEventCreate(&e0)) != hipSuccess) return e;
    if ((e = hipEventCreate(&e1)) != hipSuccess) return e;
    RadianceArgs ra;
    memset(&ra, 0, sizeof ra);
    ra.prim_rgb = prim.as<double>();
    ra.pixels = pixels.as<int2>();
    ra.npix = (int32_t)npix;
    ra.S = (int32_t)S;
    ra.dof_test = 1;
    ra.out_w = w;
    ra.bw = 1.0 / (1 << aa) / (1 << aa);
    ra.frame = frame.as<double>();
    AccumArgs ma;
    memset(&ma, 0, sizeof ma);
    ma.npix = (int64_t)npix;
    ma.S = S;
    ma.pass = frame.as<double>();
    ma.acc = acc.as<double>();
    ma.counts = cnt.as<int64_t>();
    NoiseArgs na;
    memset(&na, 0, sizeof na);
    na.npix = (int64_t)npix;
    na.counts = cnt.as<int64_t>();
    na.acc = acc.as<double>();
    na.partial = part.as<double>();
    double *out[3] = {reduce_ms, merge_ms, noise_ms};
    for (int k = 0; k < 3; k++) {
      std::vector<float> ms;
      for (int i = 0; i < warmup + reps; i++) {
        if ((e = hipEventRecord(e0, c->stream)) != hipSuccess) return e;
        if (k == 0) launch_reduce_radiance(ra, c->stream);
        else if (k == 1) launch_accum_merge(ma, c->stream);
        else launch_accum_noise(na, c->stream);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipEventRecord(e1, c->stream)) != hipSuccess) return e;
        if ((e = hipEventSynchronize(e1)) != hipSuccess) return e;
        float t = 0.f;
        if ((e = hipEventElapsedTime(&t, e0, e1)) != hipSuccess) return e;
        if (i >= warmup) ms.push_back(t);
      }
      std::sort(ms.begin(), ms.end());
      if (out[k]) *out[k] = ms.size() % 2 ? ms[ms.size() / 2] : 0.5 * (ms[ms.size() / 2 - 1] + ms[ms.size() / 2]);
    }
    return hipSuccess;
  };
  const hipError_t e = run();
  (void)hipStreamSynchronize(c->stream);
  if (e0) hipEventDestroy(e0);
  if (e1) hipEventDestroy(e1);
  HIPCHK(c, e);
  return GI_OK;
}

// Diagnostics: the adaptive passes' kernels on a synthetic frame, as gi_radiance_bench does it.
// select = tile_error_kernel + tile_select_kernel; the masked fold takes the pixel list of a
// checkerboard of tiles (half of them active); the whole-frame fold for comparison.
int gi_adaptive_bench(gi_ctx *c, int w, int h, int tile_px, int warmup, int reps, double *select_ms,
                      double *masked_merge_ms, double *merge_ms) {
  if (!c) return GI_ERR_ARG;
  if (w <= 0 || h <= 0 || (int64_t)w * h >= ((int64_t)1 << 31) || tile_px < 4 || tile_px > 64 ||
      warmup < 0 || reps < 1 || reps > 10000)
    return fail(c, GI_ERR_ARG, "adaptive bench: bad size or repetition count");
  DeviceScope dev(c->device);
  const size_t npix = (size_t)w * h;
  const int tx = (w + tile_px - 1) / tile_px, ty = (h + tile_px - 1) / tile_px;
  const size_t nt = (size_t)tx * ty;
  std::vector<int32_t> pix;
  for (int t = 0; t < tx * ty; t++) {
    if (((t % tx) + (t / tx)) % 2) continue;
    const int x0 = (t % tx) * tile_px, y0 = (t / tx) * tile_px;
    for (int y = y0; y < std::min(h, y0 + tile_px); y++)
      for (int x = x0; x < std::min(w, x0 + tile_px); x++) {
        pix.push_back(x);
        pix.push_back(y);
      }
  }
  DBuf pixels, frame, acc, cnt, terr, tmin, tmask;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  auto run = [&]() -> hipError_t {
    hipError_t e;
    if ((e = upload(pixels, pix.data(), pix.size() * 4, c->stream)) != hipSuccess) return e;
    if ((e = frame.ensure(npix * 48)) != hipSuccess) return e;
    if ((e = acc.ensure(npix * 48)) != hipSuccess) return e;
    if ((e = cnt.ensure(npix * 8)) != hipSuccess) return e;
    if ((e = terr.ensure(nt * 8)) != hipSuccess) return e;
    if ((e = tmin.ensure(nt * 8)) != hipSuccess) return e;
    if ((e = tmask.ensure(nt)) != hipSuccess) return e;
    // bytes 0x3f: every double is 4.7e-4; counts of bytes 0x01: the general branches
    if ((e = hipMemsetAsync(frame.p, 0x3f, npix * 48, c->stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(acc.p, 0x3f, npix * 48, c->stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(cnt.p, 0x01, npix * 8, c->stream)) != hipSuccess) return e;
    if ((e = hipEventCreate(&e0)) != hipSuccess) return e;
    if ((e = hipEventCreate(&e1)) != hipSuccess) return e;
    TileArgs ta;
    memset(&ta, 0, sizeof ta);
    ta.width = w; ta.height = h; ta.T = tile_px; ta.tiles_x = tx; ta.tiles_y = ty;
    ta.acc = acc.as<double>();
    ta.counts = cnt.as<int64_t>();
    ta.tile_error = terr.as<double>();
    ta.tile_nmin = tmin.as<int64_t>();
    SelectArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.tiles_x = tx; sa.tiles_y = ty; sa.dilate = 1;
    sa.min_samples = 8;
    sa.threshold = 0.02;
    sa.tile_error = ta.tile_error;
    sa.tile_nmin = ta.tile_nmin;
    sa.mask = tmask.as<uint8_t>();
    AccumArgs ma;
    memset(&ma, 0, sizeof ma);
    ma.S = 4;
    ma.pass = frame.as<double>();
    ma.acc = acc.as<double>();
    ma.counts = cnt.as<int64_t>();
    ma.width = w;
    double *out[3] = {select_ms, masked_merge_ms, merge_ms};
    for (int k = 0; k < 3; k++) {
      std::vector<float> ms;
      ma.npix = k == 1 ? (int64_t)pix.size() / 2 : (int64_t)npix;
      ma.pixels = k == 1 ? pixels.as<int2>() : nullptr;
      for (int i = 0; i < warmup + reps; i++) {
        if ((e = hipEventRecord(e0, c->stream)) != hipSuccess) return e;
        if (k == 0) {
          launch_tile_error(ta, c->stream);
          launch_tile_select(sa, c->stream);
        } else {
          launch_accum_merge(ma, c->stream);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipEventRecord(e1, c->stream)) != hipSuccess) return e;
        if ((e = hipEventSynchronize(e1)) != hipSuccess) return e;
        float t = 0.f;
        if ((e = hipEventElapsedTime(&t, e0, e1)) != hipSuccess) return e;
        if (i >= warmup) ms.push_back(t);
      }
      std::sort(ms.begin(), ms.end());
      if (out[k]) *out[k] = ms.size() % 2 ? ms[ms.size() / 2] : 0.5 * (ms[ms.size() / 2 - 1] + ms[ms.size() / 2]);
    }
    return hipSuccess;
  };
  const hipError_t e = run();
  (void)hipStreamSynchronize(c->stream);
  if (e0) hipEventDestroy(e0);
  if (e1) hipEventDestroy(e1);
  HIPCHK(c, e);
  return GI_OK;
}

int gi_estimate_radiance_batch(gi_ctx *c, int map, int64_t n, const gi_radiance_query *q,
                               double *rgb_out, int32_t *nfound, float *maxd2) {
  if (!c || map < 0 || map > 1 || (n > 0 && (!q || !rgb_out))) return GI_ERR_ARG;
  if (n == 0) return GI_OK;
  for (int64_t i = 1; i < n; i++)
    if (q[i].k != q[0].k || q[i].max_dist != q[0].max_dist || q[i].filter != q[0].filter)
      return fail(c, GI_ERR_ARG, "estimate_size / estimate_dist / filter must be uniform");
  if (n > QMETA_MAX_MATS) return fail(c, GI_ERR_ARG, "at most 2^26 queries per call");
  // one material per query carries its brdf terms
  std::vector<DMaterial> mats(n);
  std::vector<float> qp(4 * n);
  std::vector<QShade> qs(n);
  for (int64_t i = 0; i < n; i++) {
    DMaterial &m = mats[i];
    memset(&m, 0, sizeof m);
    for (int j = 0; j < 3; j++) { m.kd[j] = q[i].kd[j]; m.ks[j] = q[i].ks[j]; }
    m.n = q[i].shininess;
    bool spec = !(m.ks[0] == 0.0 && m.ks[1] == 0.0 && m.ks[2] == 0.0);
    m.flags = spec ? MF_SPECULAR : 0;
    double ct = q[i].cos_theta;
    uint32_t sign = (ct > 0) ? 1u : ((ct < 0) ? 2u : 0u);
    uint32_t meta = sign | ((uint32_t)i << 2);
    qp[4 * i] = (float)q[i].point[0];
    qp[4 * i + 1] = (float)q[i].point[1];
    qp[4 * i + 2] = (float)q[i].point[2];
    memcpy(&qp[4 * i + 3], &meta, 4);
    for (int j = 0; j < 3; j++) {
      qs[i].n[j] = q[i].normal[j];
      qs[i].ex[j] = q[i].exact_bounce[j];
      qs[i].w[j] = 1.0;
    }
  }
  DBuf dm, dq, ds, dout, dn, dmd;
  HIPCHK(c, upload(dm, mats.data(), mats.size() * sizeof(DMaterial), c->stream));
  HIPCHK(c, upload(dq, qp.data(), qp.size() * 4, c->stream));
  HIPCHK(c, upload(ds, qs.data(), qs.size() * sizeof(QShade), c->stream));
  HIPCHK(c, dout.ensure((size_t)n * 24));
  HIPCHK(c, dn.ensure((size_t)n * 4));
  HIPCHK(c, dmd.ensure((size_t)n * 4));
  KnnArgs k = knn_args(c, map);
  k.mats = dm.as<DMaterial>();
  k.K = q[0].k;
  k.filter = q[0].filter;
  k.general = c->knn_general_mode > 0 ? 1 : knn_general(mats, k.filter, true);  // the batch's own materials
  k.r2f = (float)(q[0].max_dist * q[0].max_dist);
  k.rmax = q[0].max_dist;
  k.qpos = dq.as<float4>();
  k.qshade = ds.as<QShade>();
  k.out = dout.as<double>();
  k.out_n = dn.as<int32_t>();
  k.out_maxd2 = dmd.as<float>();
  // an instance without the general estimate form counts the queries it cannot answer
  // (ST_GEN_MISS; the batch's own materials decide, so none is expected): re-run those batches
  // with the general instances instead of returning NaN
  unsigned long long *miss = c->res.d_stats.as<unsigned long long>() + ST_GEN_MISS;
  for (int pass = 0;; pass++) {
    HIPCHK(c, hipMemsetAsync(miss, 0, 8, c->stream));
    int rc = run_knn(c, k, n, nullptr);
    if (rc) return rc;
    unsigned long long nm = 0;
    HIPCHK(c, hipMemcpyAsync(&nm, miss, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nm == 0) break;
    if (pass > 0 || k.general) return fail(c, GI_ERR_STATE, "k-NN estimate: general-form miss");
    k.general = 1;
  }
  HIPCHK(c, hipMemcpyAsync(rgb_out, dout.p, (size_t)n * 24, hipMemcpyDeviceToHost, c->stream));
  if (nfound) HIPCHK(c, hipMemcpyAsync(nfound, dn.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  if (maxd2) HIPCHK(c, hipMemcpyAsync(maxd2, dmd.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GI_OK;
}

int gi_knn_batch(gi_ctx *c, int map, int64_t n, const double *pts, int K, double max_dist,
                 int32_t *idx_out, float *d2_out, int32_t *nfound) {
  if (!c || map < 0 || map > 1 || K <= 0 || (n > 0 && (!pts || !idx_out || !d2_out || !nfound)))
    return GI_ERR_ARG;
  if (n == 0) return GI_OK;
  std::vector<float> qp(4 * n, 0.0f);
  for (int64_t i = 0; i < n; i++)
    for (int j = 0; j < 3; j++) qp[4 * i + j] = (float)pts[3 * i + j];
  DBuf dq, di, dd, dn;
  HIPCHK(c, upload(dq, qp.data(), qp.size() * 4, c->stream));
  HIPCHK(c, di.ensure((size_t)n * K * 4));
  HIPCHK(c, dd.ensure((size_t)n * K * 4));
  HIPCHK(c, dn.ensure((size_t)n * 4));
  KnnArgs k = knn_args(c, map);
  k.mode = KNN_MODE_LIST;
  k.K = K;
  k.r2f = (float)(max_dist * max_dist);
  k.rmax = max_dist;
  k.qpos = dq.as<float4>();
  k.out_idx = di.as<int32_t>();
  k.out_d2 = dd.as<float>();
  k.out_n = dn.as<int32_t>();
  k.stats = nullptr;
  int rc = run_knn(c, k, n, nullptr);
  if (rc) return rc;
  std::vector<int32_t> idx((size_t)n * K);
  HIPCHK(c, hipMemcpyAsync(idx.data(), di.p, idx.size() * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(d2_out, dd.p, (size_t)n * K * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(nfound, dn.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // kd order -> storage (emission) order indices
  const auto &perm = c->hmap[map].perm;
  for (size_t i = 0; i < idx.size(); i++) idx_out[i] = idx[i] >= 0 ? perm[idx[i]] : -1;
  return GI_OK;
}

int gi_knn_bench(gi_ctx *c, int map, int64_t n, const double *pts, const double *nrm,
                 const int32_t *mat, int mode, int kernel, int iters, double *ms_out,
                 double *found_out, double *visited_out) {
  if (!c || map < 0 || map > 1 || n <= 0 || !pts || iters <= 0 || mode < 0 || mode > 2)
    return GI_ERR_ARG;
  if (mode == KNN_MODE_RADIANCE && (!nrm || !mat || !c->have_scene))
    return fail(c, GI_ERR_STATE, "radiance mode needs normals, materials and a scene");
  std::vector<float> qp(4 * n, 0.0f);
  std::vector<QShade> qs(n);
  for (int64_t i = 0; i < n; i++) {
    for (int j = 0; j < 3; j++) qp[4 * i + j] = (float)pts[3 * i + j];
    uint32_t meta = mat ? ((uint32_t)std::max(0, mat[i]) << 2) : 0u;
    memcpy(&qp[4 * i + 3], &meta, 4);
    for (int j = 0; j < 3; j++) {
      qs[i].n[j] = nrm ? nrm[3 * i + j] : 0.0;
      qs[i].ex[j] = nrm ? nrm[3 * i + j] : 0.0;
      qs[i].w[j] = 1.0;
    }
  }
  KnnArgs k = knn_args(c, map);
  DBuf dq, ds, dout, di, dd, dn;
  HIPCHK(c, upload(dq, qp.data(), qp.size() * 4, c->stream));
  HIPCHK(c, upload(ds, qs.data(), qs.size() * sizeof(QShade), c->stream));
  HIPCHK(c, dout.ensure((size_t)n * 24));
  k.qpos = dq.as<float4>();
  k.qshade = ds.as<QShade>();
  k.out = dout.as<double>();
  k.mode = mode;
  if (mode == KNN_MODE_LIST) {
    HIPCHK(c, di.ensure((size_t)n * k.K * 4));
    HIPCHK(c, dd.ensure((size_t)n * k.K * 4));
    HIPCHK(c, dn.ensure((size_t)n * 4));
    k.out_idx = di.as<int32_t>();
    k.out_d2 = dd.as<float>();
    k.out_n = dn.as<int32_t>();
  }
  float bmin[3], bmax[3];
  for (int j = 0; j < 3; j++) { bmin[j] = FLT_MAX; bmax[j] = -FLT_MAX; }
  for (int64_t i = 0; i < n; i++)
    for (int j = 0; j < 3; j++) {
      bmin[j] = std::min(bmin[j], qp[4 * i + j]);
      bmax[j] = std::max(bmax[j], qp[4 * i + j]);
    }
  uint32_t *perm = nullptr;
  HIPCHK(c, morton_order(dq.as<float4>(), n, bmin, bmax, c->s.map[0].sorter, &perm, c->stream));
  k.perm = perm;
  int saved = c->knn_kernel_kind;
  if (kernel >= 0) c->knn_kernel_kind = kernel;
  HIPCHK(c, hipMemsetAsync(c->res.d_stats.p, 0, ST_BYTES, c->stream));
  double ms = 0;
  int rc = GI_OK;
  for (int it = 0; it < iters && rc == GI_OK; it++) rc = run_knn(c, k, n, &ms);
  c->knn_kernel_kind = saved;
  if (rc) return rc;
  unsigned long long st[ST_COUNT];
  HIPCHK(c, read_stats(c, st));
  // a measurement over wrong (NaN) estimates would be meaningless
  if (st[ST_GEN_MISS]) return fail(c, GI_ERR_STATE, "k-NN bench: queries needed the general estimate form");
  log_phase_cycles(c, st);
  if (ms_out) *ms_out = ms / iters;
  int so = map * ST_KNN_MAP;
  double nqd = (double)std::max<unsigned long long>(1, st[ST_KNN + so]);
  if (found_out) *found_out = (double)st[ST_KNN_PHOTONS + so] / nqd;
  if (visited_out) *visited_out = (double)st[ST_KNN_VISITED + so] / nqd;
  return GI_OK;
}

int gi_math_probe(gi_ctx *c, int fn, int64_t n, const double *x, const double *y, double *out) {
  if (!c || n < 0 || fn < 0 || fn > 7 || (n > 0 && (!x || !y || !out))) return GI_ERR_ARG;
  if (n == 0) return GI_OK;
  DeviceScope scope(c->device);
  DBuf dx, dy, dout;
  HIPCHK(c, upload(dx, x, (size_t)n * 8, c->stream));
  HIPCHK(c, upload(dy, y, (size_t)n * 8, c->stream));
  HIPCHK(c, dout.ensure((size_t)n * 8));
  launch_math_probe(fn, n, dx.as<double>(), dy.as<double>(), dout.as<double>(), c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out, dout.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GI_OK;
}

int gi_intersect_batch(gi_ctx *c, int64_t n, const double *org, const double *dir, int32_t *hit,
                       double *t, double *point, double *normal, int32_t *material) {
  if (!c) return GI_ERR_ARG;
  if (!c->have_scene) return fail(c, GI_ERR_STATE, "no scene loaded");
  if (n == 0) return GI_OK;
  DBuf dorg, ddir, dhit, dt, dp, dn, dm;
  HIPCHK(c, upload(dorg, org, (size_t)n * 24, c->stream));
  HIPCHK(c, upload(ddir, dir, (size_t)n * 24, c->stream));
  HIPCHK(c, dhit.ensure((size_t)n * 4));
  HIPCHK(c, dt.ensure((size_t)n * 8));
  HIPCHK(c, dp.ensure((size_t)n * 24));
  HIPCHK(c, dn.ensure((size_t)n * 24));
  HIPCHK(c, dm.ensure((size_t)n * 4));
  launch_intersect(make_view(c), n, dorg.as<double>(), ddir.as<double>(), dhit.as<int32_t>(),
                   dt.as<double>(), dp.as<double>(), dn.as<double>(), dm.as<int32_t>(), c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(hit, dhit.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(t, dt.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(point, dp.p, (size_t)n * 24, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(normal, dn.p, (size_t)n * 24, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(material, dm.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GI_OK;
}

int gi_intersect_probe(gi_ctx *c, int64_t n, const double *org, const double *dir,
                       const int32_t *hint, int instance, int32_t *hit, double *t, double *point,
                       double *normal, int32_t *material, int32_t *tri) {
  if (!c) return GI_ERR_ARG;
  if (!c->have_scene) return fail(c, GI_ERR_STATE, "no scene loaded");
  if (n < 0 || (n > 0 && (!org || !dir || !hit || !t || !point || !normal || !material || !tri)))
    return fail(c, GI_ERR_ARG, "intersect probe: missing array");
  const int64_t ntris = (int64_t)c->scene.tris.size();
  if (hint)
    for (int64_t i = 0; i < n; i++)
      if (hint[i] < -1 || hint[i] >= ntris) return fail(c, GI_ERR_ARG, "intersect probe: hint out of range");
  if (n == 0) return GI_OK;
  DeviceScope scope(c->device);
  DBuf dorg, ddir, dhint, dhit, dt, dp, dn, dm, dtri;
  HIPCHK(c, upload(dorg, org, (size_t)n * 24, c->stream));
  HIPCHK(c, upload(ddir, dir, (size_t)n * 24, c->stream));
  if (hint) HIPCHK(c, upload(dhint, hint, (size_t)n * 4, c->stream));
  HIPCHK(c, dhit.ensure((size_t)n * 4));
  HIPCHK(c, dt.ensure((size_t)n * 8));
  HIPCHK(c, dp.ensure((size_t)n * 24));
  HIPCHK(c, dn.ensure((size_t)n * 24));
  HIPCHK(c, dm.ensure((size_t)n * 4));
  HIPCHK(c, dtri.ensure((size_t)n * 4));
  if (!launch_intersect_probe(make_view(c), instance, n, dorg.as<double>(), ddir.as<double>(),
                              hint ? dhint.as<int32_t>() : nullptr, dhit.as<int32_t>(),
                              dt.as<double>(), dp.as<double>(), dn.as<double>(), dm.as<int32_t>(),
                              dtri.as<int32_t>(), c->stream))
    return fail(c, GI_ERR_ARG, "intersect probe: the instance does not hold the scene's shape kinds");
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(hit, dhit.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(t, dt.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(point, dp.p, (size_t)n * 24, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(normal, dn.p, (size_t)n * 24, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(material, dm.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(tri, dtri.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GI_OK;
}

int gi_illum_probe(gi_ctx *c, int64_t n, const double *p_scene, const int32_t *light,
                   const double *r12, const double *p_light_in, int use_mask, int instance,
                   double *p_light_out, int32_t *lit) {
  if (!c) return GI_ERR_ARG;
  if (!c->have_scene) return fail(c, GI_ERR_STATE, "no scene loaded");
  if (n < 0 || (n > 0 && (!p_scene || !light || !p_light_out || !lit)))
    return fail(c, GI_ERR_ARG, "illum probe: missing array");
  const auto &lights = c->scene.lights;
  for (int64_t i = 0; i < n; i++) {
    const int li = light[i];
    if (li < -1 || li >= (int)lights.size()) return fail(c, GI_ERR_ARG, "illum probe: light out of range");
    if (li < 0) {
      if (use_mask) return fail(c, GI_ERR_ARG, "illum probe: the mask needs a light");
      if (!p_light_in) return fail(c, GI_ERR_ARG, "illum probe: light -1 needs p_light_in");
    } else {
      if (lights[li].kind != LK_AREA && lights[li].kind != LK_RECT)
        return fail(c, GI_ERR_ARG, "illum probe: sample coefficients and the mask need an area or rect light");
      if (!r12) return fail(c, GI_ERR_ARG, "illum probe: a light needs r12");
    }
  }
  if (n == 0) return GI_OK;
  DeviceScope scope(c->device);
  DBuf dps, dl, dr, dpi, dpo, dv;
  HIPCHK(c, upload(dps, p_scene, (size_t)n * 24, c->stream));
  HIPCHK(c, upload(dl, light, (size_t)n * 4, c->stream));
  if (r12) HIPCHK(c, upload(dr, r12, (size_t)n * 16, c->stream));
  if (p_light_in) HIPCHK(c, upload(dpi, p_light_in, (size_t)n * 24, c->stream));
  HIPCHK(c, dpo.ensure((size_t)n * 24));
  HIPCHK(c, dv.ensure((size_t)n * 4));
  if (!launch_illum_probe(make_view(c), instance, n, dps.as<double>(), dl.as<int32_t>(),
                          r12 ? dr.as<double>() : nullptr, p_light_in ? dpi.as<double>() : nullptr,
                          use_mask ? 1 : 0, dpo.as<double>(), dv.as<int32_t>(), c->stream))
    return fail(c, GI_ERR_ARG, "illum probe: the instance does not hold the scene's shape kinds");
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(p_light_out, dpo.p, (size_t)n * 24, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(lit, dv.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GI_OK;
}

int gi_scene_slab_boxes(const char *scene_path, int64_t capacity, double *boxes, int64_t *count) {
  if (!scene_path || !count) return GI_ERR_ARG;
  HostScene H;
  std::string err;
  if (!load_scene(scene_path, false, H, err)) return GI_ERR_IO;
  int64_t n = 0;
  auto put = [&](int kind, int node, const double *lo, const double *hi) {
    if (boxes && n < capacity) {
      double *o = boxes + 20 * n;
      int ntx = 0;
      const DNode *tx = nullptr;
      for (int k = node; k >= 0; k = H.nodes[k].parent)
        if (!H.nodes[k].identity) { ntx++; tx = &H.nodes[k]; }
      o[0] = kind;
      o[1] = ntx <= 1 ? 1.0 : 0.0;
      for (int i = 0; i < 3; i++) { o[2 + i] = lo[i]; o[5 + i] = hi[i]; }
      for (int i = 0; i < 12; i++) o[8 + i] = (ntx == 1) ? tx->Tinv[i] : (i % 5 == 0 ? 1.0 : 0.0);
    }
    n++;
  };
  for (const DElement &el : H.elems) {
    put(0, el.node, el.pmin, el.pmax);
    for (int s = el.shape_first; s < el.shape_first + el.shape_count; s++) {
      const DShape &sh = H.shapes[s];
      if (sh.kind != SK_MESH || sh.bvh_first < 0) continue;
      const int end = H.bvh[sh.bvh_first].skip;
      for (int b = 0; b < end; b++) put(1, el.node, H.bvh[sh.bvh_first + b].lo, H.bvh[sh.bvh_first + b].hi);
    }
  }
  *count = n;
  if (boxes && capacity < n) return GI_ERR_ARG;
  return GI_OK;
}

int gi_scene_triangle_planes(gi_ctx *c, int64_t capacity, double *planes, int64_t *count) {
  if (!c || !count) return GI_ERR_ARG;
  if (!c->have_scene) return fail(c, GI_ERR_STATE, "no scene loaded");
  const HostScene &H = c->scene;
  *count = (int64_t)H.tris.size();
  if (!planes) return GI_OK;
  if (capacity < *count) return fail(c, GI_ERR_ARG, "triangle planes: capacity too small");
  auto up = [&](int node, double *p) {  // a point of `node`'s frame in world coordinates
    for (int k = node; k >= 0; k = H.nodes[k].parent) {
      const DNode &a = H.nodes[k];
      if (a.identity) continue;
      const double x = p[0], y = p[1], z = p[2];
      for (int r = 0; r < 3; r++) p[r] = a.T[4 * r] * x + a.T[4 * r + 1] * y + a.T[4 * r + 2] * z + a.T[4 * r + 3];
    }
  };
  for (const DElement &el : H.elems)
    for (int s = el.shape_first; s < el.shape_first + el.shape_count; s++) {
      const DShape &sh = H.shapes[s];
      const int cnt = sh.kind == SK_TRI ? 1 : (sh.kind == SK_MESH ? sh.tri_count : 0);
      for (int i = 0; i < cnt; i++) {
        const DTri &tr = H.tris[sh.tri_first + i];
        // three points of the plane: p0 and p0 plus two tangents (-edge-plane normals lie in it)
        double q[3][3];
        for (int r = 0; r < 3; r++) {
          q[0][r] = tr.p0[r];
          q[1][r] = tr.p0[r] + tr.ev[0][r];
          q[2][r] = tr.p0[r] + tr.ev[1][r];
        }
        for (int k = 0; k < 3; k++) up(el.node, q[k]);
        const double a[3] = {q[1][0] - q[0][0], q[1][1] - q[0][1], q[1][2] - q[0][2]};
        const double b[3] = {q[2][0] - q[0][0], q[2][1] - q[0][1], q[2][2] - q[0][2]};
        double nn[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const double l = std::sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
        double *o = planes + 4 * (size_t)(sh.tri_first + i);
        for (int r = 0; r < 3; r++) o[r] = l > 0 ? nn[r] / l : 0.0;
        o[3] = -(o[0] * q[0][0] + o[1] * q[0][1] + o[2] * q[0][2]);
      }
    }
  return GI_OK;
}

}  // extern "C"
