// gi_photons.cpp -- the photon maps: tracing (MapPhotons, photonmap.cpp:260-436), the host kd
// build, the upload / device build of a map and its replication over a device set.
#include <cfloat>
#include <chrono>
#include <cmath>
#include "gi_ctx.h"

namespace {

// RNRgb_to_RGBE / RGBE_to_RNRgb (graphics_utils.cpp:50-77), host side
void rgbe_enc(const double c[3], uint8_t *out) {
  double mx = 0;
  for (int i = 0; i < 3; i++)
    if (c[i] > mx) mx = c[i];
  if (!(mx > 0)) { out[0] = out[1] = out[2] = out[3] = 0; return; }
  int e;
  double m = frexp(mx, &e);
  out[0] = (uint8_t)(256.0 * c[0] / mx * m);
  out[1] = (uint8_t)(256.0 * c[1] / mx * m);
  out[2] = (uint8_t)(256.0 * c[2] / mx * m);
  out[3] = (uint8_t)(e + 128);
}
void rgbe_dec(const uint8_t *in, double c[3]) {
  if (!in[3]) { c[0] = c[1] = c[2] = 0; return; }
  double inv = ldexp(1.0, ((int)in[3]) - 128 - 8);
  for (int i = 0; i < 3; i++) c[i] = (double)in[i] * inv;
}

// ---------------------------------------------------------------------------------------
// photon map: host kd build of an implicit complete tree (leaf l holds photons
// [start(l), start(l + 1)), gi_layout.h kd_leaf_start); split = median of the node's range
// along its longest bbox axis.
// Any kd-tree gives the same k-NN set (up to ties at the k-th distance, broken here by
// (d2, kd-order index)); the reference's tree is R3Kdtree.cpp:1552-1671.
// ---------------------------------------------------------------------------------------
void kd_rec(HostMap &M, int node, int a, int b, int depth_par) {
  int64_t n = (int64_t)M.storage.size();
  int L = M.nleaves;
  if (node >= L) return;
  int64_t lo = kd_leaf_start(n, M.levels, a), hi = kd_leaf_start(n, M.levels, b);
  int midleaf = (a + b) / 2;
  int64_t mid = kd_leaf_start(n, M.levels, midleaf);
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int64_t i = lo; i < hi; i++) {
    const float *p = M.storage[M.perm[i]].pos;
    for (int k = 0; k < 3; k++) { mn[k] = std::min(mn[k], p[k]); mx[k] = std::max(mx[k], p[k]); }
  }
  int axis = 0;
  float ext = mx[0] - mn[0];
  if (mx[1] - mn[1] > ext) { axis = 1; ext = mx[1] - mn[1]; }
  if (mx[2] - mn[2] > ext) axis = 2;
  float split = 0.f;
  if (hi > lo && mid < hi) {
    std::nth_element(M.perm.begin() + lo, M.perm.begin() + mid, M.perm.begin() + hi,
                     [&](int x, int y) { return M.storage[x].pos[axis] < M.storage[y].pos[axis]; });
    split = M.storage[M.perm[mid]].pos[axis];
  } else if (hi > lo) {
    split = mx[axis];
  }
  M.nodes[8 * node + 3] = split;
  int ai = axis;
  memcpy(&M.nodes[8 * node + 7], &ai, 4);
  if (depth_par > 0) {
    std::thread t([&]() { kd_rec(M, 2 * node, a, midleaf, depth_par - 1); });
    kd_rec(M, 2 * node + 1, midleaf, b, depth_par - 1);
    t.join();
  } else {
    kd_rec(M, 2 * node, a, midleaf, 0);
    kd_rec(M, 2 * node + 1, midleaf, b, 0);
  }
}

void kd_build(HostMap &M, int leaf_size, int threads) {
  int64_t n = (int64_t)M.storage.size();
  M.nleaves = 1;
  M.levels = 0;
  while ((int64_t)M.nleaves * leaf_size < n) { M.nleaves *= 2; M.levels++; }
  M.perm.resize(n);
  for (int64_t i = 0; i < n; i++) M.perm[i] = (int32_t)i;
  const int L = M.nleaves;
  M.nodes.assign(8 * 2 * (size_t)L, 0.0f);
  int par = 0;
  while ((1 << par) < threads && par < 4) par++;
  if (n > 0) kd_rec(M, 1, 0, L, par);
  M.pos4.resize(4 * (size_t)n);
  M.rgbe.resize(n);
  for (int k = 0; k < 3; k++) { M.bmin[k] = FLT_MAX; M.bmax[k] = -FLT_MAX; }
  for (int64_t i = 0; i < n; i++) {
    const gi_photon &p = M.storage[M.perm[i]];
    uint32_t w = (uint32_t)p.dir | ((uint32_t)p.flags << 16);
    M.pos4[4 * i] = p.pos[0];
    M.pos4[4 * i + 1] = p.pos[1];
    M.pos4[4 * i + 2] = p.pos[2];
    memcpy(&M.pos4[4 * i + 3], &w, 4);
    memcpy(&M.rgbe[i], p.rgbe, 4);
    for (int k = 0; k < 3; k++) {
      M.bmin[k] = std::min(M.bmin[k], p.pos[k]);
      M.bmax[k] = std::max(M.bmax[k], p.pos[k]);
    }
  }
  // tight boxes: leaves from their photons, internal nodes as the union of their children
  // (an empty leaf gets lo = +inf, hi = -inf: its box distance is +inf)
  for (int l = 0; l < L; l++) {
    float *b = &M.nodes[8 * (size_t)(L + l)];
    b[0] = b[1] = b[2] = INFINITY;
    b[4] = b[5] = b[6] = -INFINITY;
    int64_t s0 = kd_leaf_start(n, M.levels, l), s1 = kd_leaf_start(n, M.levels, l + 1);
    for (int64_t i = s0; i < s1; i++)
      for (int k = 0; k < 3; k++) {
        b[k] = std::min(b[k], M.pos4[4 * i + k]);
        b[4 + k] = std::max(b[4 + k], M.pos4[4 * i + k]);
      }
  }
  for (int v = L - 1; v >= 1; v--) {
    float *b = &M.nodes[8 * (size_t)v];
    const float *c0 = &M.nodes[8 * (size_t)(2 * v)], *c1 = &M.nodes[8 * (size_t)(2 * v + 1)];
    for (int k = 0; k < 3; k++) {
      b[k] = std::min(c0[k], c1[k]);
      b[4 + k] = std::max(c0[4 + k], c1[4 + k]);
    }
  }
}

int upload_map(gi_ctx *c, int mi) {
  HostMap &H = c->hmap[mi];
  DevMap &D = c->res.dmap[mi];
  int64_t n = (int64_t)H.storage.size();
  if (int rc = check_kd_shape(c, H.nleaves, H.levels)) return rc;
  HIPCHK(c, upload(D.pos4, H.pos4.data(), H.pos4.size() * 4, c->stream));
  HIPCHK(c, upload(D.rgbe, H.rgbe.data(), H.rgbe.size() * 4, c->stream));
  HIPCHK(c, upload(D.nodes, H.nodes.data(), H.nodes.size() * 4, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  D.n = n;
  D.nleaves = H.nleaves;
  D.levels = H.levels;
  D.dk_k = -1;
  c->map_valid[mi] = n > 0;
  return GI_OK;
}

// the device build (f1): the emission-ordered photons go up once, the tree, the kd-order
// arrays and the permutation come back (perm only to the host, for the test seams' indices)
int build_map_device(gi_ctx *c, int mi, bool upload_storage = true) {
  HostMap &H = c->hmap[mi];
  DevMap &D = c->res.dmap[mi];
  const int64_t n = (int64_t)H.storage.size();
  static_assert(sizeof(gi_photon) == sizeof(KdPhoton), "photon record layout");
  if (upload_storage)  // else kd_ph already holds H.storage (traced on this device)
    HIPCHK(c, upload(c->s.kd_ph, H.storage.data(), (size_t)n * sizeof(gi_photon), c->stream));
  int64_t L = 1;
  while (L * c->leaf_size[mi] < n) L *= 2;
  HIPCHK(c, D.pos4.ensure((size_t)n * 16));
  HIPCHK(c, D.rgbe.ensure((size_t)n * 4));
  HIPCHK(c, D.nodes.ensure((size_t)L * 16 * 4));
  H.perm.resize(n);
  H.pos4.clear();
  H.rgbe.clear();
  H.nodes.clear();
  HIPCHK(c, kd_build_device(c->s.kd_ph.as<KdPhoton>(), n, c->leaf_size[mi], c->s.kdb, D.pos4.as<float>(),
                            D.rgbe.as<uint32_t>(), D.nodes.as<float>(),
                            reinterpret_cast<uint32_t *>(H.perm.data()), &H.nleaves, &H.levels,
                            c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = check_kd_shape(c, H.nleaves, H.levels)) return rc;
  D.n = n;
  D.nleaves = H.nleaves;
  D.levels = H.levels;
  D.dk_k = -1;
  c->map_valid[mi] = n > 0;
  return GI_OK;
}

// kd tree + device arrays of map mi from its emission-ordered photons (hmap[mi].storage)
int build_map(gi_ctx *c, int mi) {
  if (c->gpu_kd) return build_map_device(c, mi);
  kd_build(c->hmap[mi], c->leaf_size[mi], std::max(1, c->P.threads));
  return upload_map(c, mi);
}

int set_map(gi_ctx *c, int mi, const gi_photon *ph, int64_t n) {
  HostMap &H = c->hmap[mi];
  H = HostMap();
  H.storage.assign(ph, ph + n);
  return build_map(c, mi);
}

// map mi from n emission-ordered photons already in device buffer `dev` (traced here): one copy
// to the host (the map's storage order, gi_get_photon_map) and, for the device build, `dev`
// becomes the build's input buffer without a re-upload
int set_map_device(gi_ctx *c, int mi, DBuf &dev, int64_t n) {
  HostMap &H = c->hmap[mi];
  H = HostMap();
  H.storage.resize(n);
  if (n) {
    HIPCHK(c, hipMemcpyAsync(H.storage.data(), dev.p, (size_t)n * sizeof(gi_photon),
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (!c->gpu_kd) return build_map(c, mi);
  std::swap(c->s.kd_ph, dev);
  return build_map_device(c, mi, false);
}

// grow a device buffer to `want` bytes keeping its first `used` bytes
hipError_t grow_keep(DBuf &b, size_t used, size_t want, hipStream_t st) {
  if (want <= b.cap && b.p) return hipSuccess;
  DBuf nb;
  hipError_t e = nb.ensure(std::max(want, b.cap + b.cap / 2));
  if (e != hipSuccess) return e;
  if (used) e = hipMemcpyAsync(nb.p, b.p, used, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  std::swap<DBuf>(b, nb);  // the old buffer is freed with nb
  return e;
}

// LightPower, graphics_utils.cpp:223-258
double light_power(const HostScene &S, const DLight &L) {
  const double PI = 3.14159265358979323846;
  double area = 1.0, flux = 4.0 * PI;
  if (L.kind == LK_DIR) {
    area = PI * pow(S.radius, 2.0);
    flux = 1.0;
  } else if (L.kind == LK_AREA) {
    area = PI * pow(L.radius, 2.0);
    flux /= 2.0;
  } else if (L.kind == LK_RECT) {
    double a1[3], a2[3];
    for (int i = 0; i < 3; i++) { a1[i] = L.a1[i] * L.len1; a2[i] = L.a2[i] * L.len2; }
    double cx = a1[1] * a2[2] - a1[2] * a2[1], cy = a1[2] * a2[0] - a1[0] * a2[2],
           cz = a1[0] * a2[1] - a1[1] * a2[0];
    area = sqrt((cx * cx) + (cy * cy) + (cz * cz));
    flux /= 2.0;
  } else if (L.kind == LK_SPOT) {
    double s = L.dropoff;
    flux = (2.0 * PI) / (s + 1.0) * (1.0 - pow(cos(L.cutoff), s + 1.0));
  }
  return (L.color[0] + L.color[1] + L.color[2]) * area * flux;
}

// trace photons [e0, e0+n) of one light on this context's device and append the stored ones in
// emission order: to `host` when given (device sets concatenate their parts there), else to the
// device map being built (pacc / pacc_n).
//
// One pass (PhotonTrace, photontracer.cpp:28-176): every stored photon takes a slot from one
// atomic per wave (StorePhoton's local buffer + flush, photon_utils.cpp:19-65, re-cut as a wave
// ballot + prefix) with the key (emission index, store ordinal); a radix sort of the keys and a
// gather restore emission order, so the map is the same photon for photon as the count pass +
// scan + re-trace (GI_PHOTON_2PASS=1) it replaces. A launch that stores more photons than the
// slots it was given is re-run with room (the RNG is keyed by emission index: same photons).
int trace_batch_dev(gi_ctx *c, int caustic, int light, int64_t e0, int64_t n,
                    std::vector<gi_photon> *host) {
  const int64_t CH = 1 << 22;
  for (int64_t s = 0; s < n; s += CH) {
    int64_t m = std::min(CH, n - s);
    PhotonArgs a;
    memset(&a, 0, sizeof a);
    a.S = make_view(c);
    a.F = make_flags(c->P);
    a.light = light;
    a.caustic = caustic;
    a.e0 = e0 + s;
    a.n = m;
    uint32_t total = 0;
    gi_photon_dev *sorted = nullptr;  // emission-ordered photons of this launch (device)
    if (c->photon_2pass) {
      HIPCHK(c, c->s.pcounts.ensure((size_t)m * 4));
      HIPCHK(c, c->s.poffs.ensure((size_t)(m + 1) * 4));
      a.counts = c->s.pcounts.as<uint32_t>();
      a.offsets = c->s.poffs.as<uint32_t>();
      launch_photons(a, PM_COUNT, c->stream);
      HIPCHK(c, hipGetLastError());
      ScanTemp t = scan_temp(c, m);
      HIPCHK(c, launch_scan(c->s.pcounts.as<uint32_t>(), c->s.poffs.as<uint32_t>(), m, t, c->stream));
      HIPCHK(c, hipMemcpyAsync(&total, c->s.poffs.as<uint32_t>() + m, 4, hipMemcpyDeviceToHost,
                               c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      if (total == 0) continue;
      HIPCHK(c, c->s.pbuf.ensure((size_t)total * sizeof(gi_photon_dev)));
      a.out = c->s.pbuf.as<gi_photon_dev>();
      launch_photons(a, PM_EMIT, c->stream);
      HIPCHK(c, hipGetLastError());
      sorted = c->s.pbuf.as<gi_photon_dev>();
    } else {
      int obits = 1;
      while (obits < 40 && (1LL << obits) < (int64_t)c->P.max_photon_depth) obits++;
      int jbits = 1;
      while ((1LL << jbits) < m) jbits++;
      double want = (double)m * (c->prate[caustic] * 1.25 + 0.02) + 4096.0;
      uint32_t cap = (uint32_t)std::min(want, 4.0e9);
      HIPCHK(c, c->s.pcursor.ensure(4));
      for (;;) {
        HIPCHK(c, c->s.pbuf.ensure((size_t)cap * sizeof(gi_photon_dev)));
        HIPCHK(c, c->s.pkeys.ensure((size_t)cap * 8));
        HIPCHK(c, hipMemsetAsync(c->s.pcursor.p, 0, 4, c->stream));
        a.out = c->s.pbuf.as<gi_photon_dev>();
        a.keys = c->s.pkeys.as<uint64_t>();
        a.cursor = c->s.pcursor.as<uint32_t>();
        a.cap = cap;
        a.obits = obits;
        launch_photons(a, PM_APPEND, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&total, c->s.pcursor.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (total <= cap) break;
        if ((double)total * 1.1 + 4096.0 > 4.0e9)
          return fail(c, GI_ERR_ALLOC, "photon launch stores more than 2^32 photons");
        cap = (uint32_t)((double)total * 1.1 + 4096.0);
      }
      c->prate[caustic] = (double)total / (double)m;
      if (total == 0) continue;
      uint64_t *skeys = nullptr;
      uint32_t *slots = nullptr;
      HIPCHK(c, key_order(c->s.pkeys.as<uint64_t>(), total, jbits + obits, c->s.psort, &skeys,
                          &slots, c->stream));
      gi_photon_dev *dst;
      if (host) {
        HIPCHK(c, c->s.ptmp.ensure((size_t)total * sizeof(gi_photon_dev)));
        dst = c->s.ptmp.as<gi_photon_dev>();
      } else {
        HIPCHK(c, grow_keep(c->s.pacc, (size_t)c->pacc_n * sizeof(gi_photon_dev),
                            (size_t)(c->pacc_n + total) * sizeof(gi_photon_dev), c->stream));
        dst = c->s.pacc.as<gi_photon_dev>() + c->pacc_n;
      }
      launch_photon_gather(c->s.pbuf.as<gi_photon_dev>(), slots, total, dst, c->stream);
      HIPCHK(c, hipGetLastError());
      sorted = dst;
    }
    if (host) {
      size_t old = host->size();
      host->resize(old + total);
      HIPCHK(c, hipMemcpyAsync(host->data() + old, sorted, (size_t)total * sizeof(gi_photon),
                               hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    } else if (sorted != c->s.pacc.as<gi_photon_dev>() + c->pacc_n) {  // 2-pass: append the launch
      HIPCHK(c, grow_keep(c->s.pacc, (size_t)c->pacc_n * sizeof(gi_photon_dev),
                          (size_t)(c->pacc_n + total) * sizeof(gi_photon_dev), c->stream));
      HIPCHK(c, hipMemcpyAsync(c->s.pacc.as<gi_photon_dev>() + c->pacc_n, sorted,
                               (size_t)total * sizeof(gi_photon_dev), hipMemcpyDeviceToDevice,
                               c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      c->pacc_n += total;
    } else {
      c->pacc_n += total;
    }
  }
  return GI_OK;
}

// trace photons [e0, e0+n) of one light: on a device set the range is cut into one contiguous
// piece per device (the RNG is keyed by emission index, so the concatenation in device order
// is the one-device result photon for photon)
int trace_batch(gi_ctx *c, int caustic, int light, int64_t e0, int64_t n,
                std::vector<gi_photon> *out) {
  const int nd = 1 + (int)c->peers.size();
  if (nd == 1 || n < 4096 * (int64_t)nd) return trace_batch_dev(c, caustic, light, e0, n, out);
  std::vector<std::vector<gi_photon>> part(nd);
  int rc = on_devices(c, [&](int k, gi_ctx *d) -> int {
    int64_t a = e0 + n * k / nd, b = e0 + n * (k + 1) / nd;
    return trace_batch_dev(d, caustic, light, a, b - a, &part[k]);
  });
  if (rc) return rc;
  for (auto &p : part) out->insert(out->end(), p.begin(), p.end());
  return GI_OK;
}

// adaptive emission rounds of Threadable_PhotonTracer (photonmap.cpp:145-257), one emitter.
// The map grows in `map` (device sets) or, when `map` is null, on this device (pacc / pacc_n).
int trace_map(gi_ctx *c, int caustic, int64_t goal, const std::vector<double> &powers,
              double total_power, std::vector<gi_photon> *map, int64_t &emitted) {
  int64_t stored = 0;
  if (!map) c->pacc_n = 0;
  emitted = 0;
  double rate = caustic ? (double)c->P.max_photon_depth : 4.0;
  double slowdown = 1.0;
  int attempts = 10;
  int nl = (int)c->scene.lights.size();
  while (stored < goal && attempts > 0) {
    int emit_goal = (int)((double)(int)(goal - stored) / rate / slowdown + 1);
    int64_t assigned = 0;
    for (int i = 0; i < nl; i++) {
      int num = (int)ceil(emit_goal * (powers[i] / total_power));
      if (c->scene.lights[i].active && num) {
        int rc = trace_batch(c, caustic, i, emitted + assigned, num, map);
        if (rc) return rc;
      }
      assigned += num;
    }
    emitted += assigned;
    stored = map ? (int64_t)map->size() : c->pacc_n;
    if (c->progress && goal > 0) c->progress(caustic ? 2 : 1, (double)stored / goal, c->progress_user);
    if (stored > 0 && emitted > 0) {
      rate = (double)stored / emitted;
      double frac = caustic ? (double)stored / goal : (double)stored / emitted;
      slowdown = (frac < 0.75) ? 2.0 : 1.0;
    } else {
      rate /= 2.0;
      attempts--;
    }
  }
  return GI_OK;
}

// the first device's photon maps (host copies + kd trees) and parameters onto the others
int replicate_maps(gi_ctx *c) {
  if (c->peers.empty()) return GI_OK;
  return on_devices(c, [&](int k, gi_ctx *d) -> int {
    if (k == 0) return GI_OK;
    d->P = c->P;
    for (int m = 0; m < 2; m++) {
      d->hmap[m] = c->hmap[m];
      // a host-built tree is uploaded; a device-built one is rebuilt on each device (the build
      // is a deterministic function of the photons: the same tree everywhere)
      int rc = d->hmap[m].pos4.empty() && !d->hmap[m].storage.empty() ? build_map_device(d, m)
                                                                        : upload_map(d, m);
      if (rc) return rc;
    }
    return (int)GI_OK;
  });
}

}  // namespace

extern "C" {

// MapPhotons, photonmap.cpp:260-436
int gi_map_photons(gi_ctx *c, gi_photon_stats *st) {
  if (!c) return GI_ERR_ARG;
  hipSetDevice(c->device);
  int rc = check_ready(c);
  if (rc) return rc;
  auto t0 = std::chrono::steady_clock::now();
  gi_params &P = c->P;
  for (int m = 0; m < 2; m++) { c->hmap[m] = HostMap(); c->map_valid[m] = false; }
  int nl = (int)c->scene.lights.size();
  int64_t gem = 0, cem = 0;
  if (st) memset(st, 0, sizeof *st);
  if (nl <= 0) return GI_OK;
  std::vector<double> powers(nl, 0.0);
  double total = 0;
  for (int i = 0; i < nl; i++) {
    if (!c->scene.lights[i].active) continue;
    powers[i] = light_power(c->scene, c->scene.lights[i]);
    total += powers[i];
  }
  if (total <= 0) return GI_OK;
  // one device: the maps grow on the device across the emission rounds (pacc; the global map is
  // then held in pglob while the caustic map is traced); device sets: on the host
  const bool on_dev = c->peers.empty();
  std::vector<gi_photon> gph, cph;
  int64_t gn = 0, cn = 0;
  if (P.indirect_illum || P.direct_photon_illum) {
    rc = trace_map(c, 0, P.global_photon_count, powers, total, on_dev ? nullptr : &gph, gem);
    if (rc) return rc;
    gn = on_dev ? c->pacc_n : (int64_t)gph.size();
    if (on_dev) std::swap(c->s.pglob, c->s.pacc);
  }
  if (P.caustic_illum) {
    rc = trace_map(c, 1, P.caustic_photon_count, powers, total, on_dev ? nullptr : &cph, cem);
    if (rc) return rc;
    cn = on_dev ? c->pacc_n : (int64_t)cph.size();
  }
  auto t1 = std::chrono::steady_clock::now();
  // power rescale (Q9), photonmap.cpp:339-361: RGBE -> colour * total / emitted -> RGBE
  auto rescale = [&](std::vector<gi_photon> &v, DBuf &dv, int64_t n, int64_t emitted) -> int {
    double pp = total / (double)emitted;
    if (on_dev) {
      launch_photon_rescale(dv.as<gi_photon_dev>(), n, pp, c->stream);
      HIPCHK(c, hipGetLastError());
      return GI_OK;
    }
    for (auto &p : v) {
      double col[3];
      rgbe_dec(p.rgbe, col);
      for (int i = 0; i < 3; i++) col[i] *= pp;
      rgbe_enc(col, p.rgbe);
    }
    return GI_OK;
  };
  if ((P.indirect_illum || P.direct_photon_illum) && gn > 0) {
    P.global_photon_count = (int)gn;
    if ((rc = rescale(gph, c->s.pglob, gn, gem))) return rc;
  } else if (P.indirect_illum || P.direct_photon_illum) {
    P.indirect_illum = 0;
    P.direct_photon_illum = 0;
  }
  if (P.caustic_illum && cn > 0) {
    P.caustic_photon_count = (int)cn;
    if ((rc = rescale(cph, c->s.pacc, cn, cem))) return rc;
  } else if (P.caustic_illum) {
    P.caustic_illum = 0;
  }
  if (on_dev) {
    rc = set_map_device(c, GI_MAP_GLOBAL, c->s.pglob, gn);
    if (rc) return rc;
    rc = set_map_device(c, GI_MAP_CAUSTIC, c->s.pacc, cn);
    if (rc) return rc;
    // tracing scratch is not needed by the render
    DBuf *rel[] = {&c->s.pbuf, &c->s.pkeys, &c->s.ptmp, &c->s.pacc, &c->s.pglob};
    for (DBuf *b : rel) b->release();
    c->s.psort = KeySortScratch();
    c->pacc_n = 0;
  } else {
    rc = set_map(c, GI_MAP_GLOBAL, gph.data(), (int64_t)gph.size());
    if (rc) return rc;
    rc = set_map(c, GI_MAP_CAUSTIC, cph.data(), (int64_t)cph.size());
    if (rc) return rc;
  }
  auto t2 = std::chrono::steady_clock::now();
  // irradiance cache, photonmap.cpp:381-413: irradiance = own power + EstimateIrradiance
  if (P.irradiance_cache && (P.indirect_illum || P.direct_photon_illum) && gn > 0) {
    HostMap &H = c->hmap[GI_MAP_GLOBAL];
    int64_t n = (int64_t)H.storage.size();
    std::vector<float> q(4 * n);
    for (int64_t i = 0; i < n; i++) {
      q[4 * i] = H.storage[i].pos[0];
      q[4 * i + 1] = H.storage[i].pos[1];
      q[4 * i + 2] = H.storage[i].pos[2];
      q[4 * i + 3] = 0;
    }
    std::vector<double> irr(3 * n);
    {
      DBuf dq, dout;  // freed before the map is set again
      HIPCHK(c, upload(dq, q.data(), q.size() * 4, c->stream));
      HIPCHK(c, dout.ensure((size_t)n * 24));
      KnnArgs k = knn_args(c, GI_MAP_GLOBAL);
      k.mode = KNN_MODE_IRRADIANCE;
      k.qpos = dq.as<float4>();
      k.out = dout.as<double>();
      k.stats = nullptr;
      // Morton order, as for the render's queries: the chunk kernel's 64-query chunks are then
      // spatial neighbourhoods (emission order scatters them over the scene)
      uint32_t *iperm = nullptr;
      HIPCHK(c, morton_order(dq.as<float4>(), n, c->sbmin, c->sbmax, c->s.map[0].sorter, &iperm, c->stream));
      k.perm = iperm;
      rc = run_knn(c, k, n, nullptr);
      if (rc) return rc;
      HIPCHK(c, hipMemcpyAsync(irr.data(), dout.p, (size_t)n * 24, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    std::vector<gi_photon> cached = H.storage;
    for (int64_t i = 0; i < n; i++) {
      double col[3];
      rgbe_dec(cached[i].rgbe, col);
      for (int j = 0; j < 3; j++) col[j] += irr[3 * i + j];
      rgbe_enc(col, cached[i].rgbe);
    }
    rc = set_map(c, GI_MAP_GLOBAL, cached.data(), n);
    if (rc) return rc;
  }
  rc = replicate_maps(c);
  if (rc) return rc;
  auto t3 = std::chrono::steady_clock::now();
  // the k-NN kernels' per-photon K-th distance bounds (ensure_dk), for the estimate sizes and
  // distances the render will use: part of building the maps, so timed here and not inside
  // the first RenderImage
  rc = on_devices(c, [&](int, gi_ctx *d) -> int {
    for (int m = 0; m < 2; m++) {
      if (!d->map_valid[m] || d->res.dmap[m].n == 0) continue;
      KnnArgs k = knn_args(d, m);
      // beyond the LDS kernels: the per-lane global-heap kernel or the range estimate, no bounds
      if (k.K <= 0 || (int64_t)k.K + 64 > 1024) continue;
      int r = ensure_dk(d, k);
      if (r) return r;
    }
    return (int)GI_OK;
  });
  if (rc) return rc;
  auto t4 = std::chrono::steady_clock::now();
  if (st) {
    st->global_stored = (int64_t)c->hmap[0].storage.size();
    st->caustic_stored = (int64_t)c->hmap[1].storage.size();
    st->global_emitted = gem;
    st->caustic_emitted = cem;
    st->trace_s = std::chrono::duration<double>(t1 - t0).count();
    // kd_s: the tree builds, their replication and the k-NN bound pass
    st->kd_s = std::chrono::duration<double>((t2 - t1) + (t4 - t3)).count();
    st->irradiance_s = std::chrono::duration<double>(t3 - t2).count();
    st->total_s = std::chrono::duration<double>(t4 - t0).count();
  }
  return GI_OK;
}

int gi_set_photon_map(gi_ctx *c, int map, const gi_photon *ph, int64_t n) {
  if (!c || map < 0 || map > 1 || (n > 0 && !ph)) return GI_ERR_ARG;
  hipSetDevice(c->device);
  int rc = set_map(c, map, ph, n);
  if (rc) return rc;
  return replicate_maps(c);
}

int gi_get_photon_map(gi_ctx *c, int map, gi_photon *out, int64_t cap, int64_t *n) {
  if (!c || map < 0 || map > 1) return GI_ERR_ARG;
  const auto &v = c->hmap[map].storage;
  if (n) *n = (int64_t)v.size();
  if (out) {
    if ((int64_t)v.size() > cap) return fail(c, GI_ERR_ARG, "capacity too small");
    memcpy(out, v.data(), v.size() * sizeof(gi_photon));
  }
  return GI_OK;
}

int gi_get_kd_tree(gi_ctx *c, int map, float *nodes, int64_t node_floats, int32_t *perm,
                   int64_t perm_cap, int32_t *nleaves, int64_t *n) {
  if (!c || map < 0 || map > 1) return GI_ERR_ARG;
  hipSetDevice(c->device);
  const HostMap &H = c->hmap[map];
  const DevMap &D = c->res.dmap[map];
  const int64_t nn = (int64_t)H.storage.size();
  if (int rc = check_kd_shape(c, H.nleaves, H.levels)) return rc;
  if (n) *n = nn;
  if (nleaves) *nleaves = H.nleaves;
  const int64_t nf = (int64_t)16 * H.nleaves;
  if (nodes) {
    if (node_floats < nf) return fail(c, GI_ERR_ARG, "node capacity too small");
    if (D.nodes.p && D.nodes.cap >= (size_t)nf * 4) {
      HIPCHK(c, hipMemcpyAsync(nodes, D.nodes.p, (size_t)nf * 4, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    } else {
      memset(nodes, 0, (size_t)nf * 4);
    }
  }
  if (perm) {
    if (perm_cap < nn) return fail(c, GI_ERR_ARG, "capacity too small");
    memcpy(perm, H.perm.data(), (size_t)nn * 4);
  }
  return GI_OK;
}

}  // extern "C"
