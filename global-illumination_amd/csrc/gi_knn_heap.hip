// gi_knn_heap.hip -- the two k-NN kernels that keep no candidates in LDS: the per-lane kernel
// with its heaps in global scratch (kind 0: any estimate size) and the cached-radiance lookup
// (kind 9, -cache). The estimate itself is gi_estimate.h's.
#include <hip/hip_runtime.h>
#include "gi_device.h"
#include "gi_kernels.h"
#include "gi_estimate.h"

namespace gi {

// ---------------------------------------------------------------------------------------
// k-NN radiance estimate (R3Kdtree::FindClosestQuick R3Kdtree.cpp:688-784 + EstimateRadiance
// photon_utils.cpp:72-162). One query per lane; stackless nearest-first traversal of the
// implicit complete kd-tree (parent = node>>1, sibling = node^1); per-lane max-heap of the K
// best (d2, index) pairs in LDS laid out [slot][lane] (conflict-free b32 accesses) or, for
// K > 64, in a global scratch laid out the same way.
// ---------------------------------------------------------------------------------------
struct HeapRef {
  float *d2;
  int32_t *idx;
  int stride;  // elements between consecutive slots of one lane
};

__device__ __forceinline__ bool heap_less(float da, int ia, float db, int ib) {
  return da < db || (da == db && ia < ib);
}

// 0-based binary max-heap on (d2, idx)
__device__ __forceinline__ void heap_push(HeapRef h, int &size, float d, int id) {
  int c = size++;
  while (c > 0) {
    int p = (c - 1) >> 1;
    float pd = h.d2[p * h.stride];
    int pi = h.idx[p * h.stride];
    if (!heap_less(pd, pi, d, id)) break;
    h.d2[c * h.stride] = pd;
    h.idx[c * h.stride] = pi;
    c = p;
  }
  h.d2[c * h.stride] = d;
  h.idx[c * h.stride] = id;
}
__device__ __forceinline__ void heap_replace_top(HeapRef h, int size, float d, int id) {
  int c = 0;
  while (true) {
    int l = 2 * c + 1;
    if (l >= size) break;
    float ld = h.d2[l * h.stride];
    int li = h.idx[l * h.stride];
    int r = l + 1;
    if (r < size) {
      float rd = h.d2[r * h.stride];
      int ri = h.idx[r * h.stride];
      if (heap_less(ld, li, rd, ri)) { l = r; ld = rd; li = ri; }
    }
    if (!heap_less(d, id, ld, li)) break;
    h.d2[c * h.stride] = ld;
    h.idx[c * h.stride] = li;
    c = l;
  }
  h.d2[c * h.stride] = d;
  h.idx[c * h.stride] = id;
}

// Find the K best photons of query (qx,qy,qz) within r2; returns heap size.
// "While-while" structure: each lane walks internal nodes until it holds its next leaf
// (or finishes); only then does the wave run the leaf loop, for all lanes at once. A single
// loop mixing descend and leaf steps would re-run the 64-photon leaf loop whenever any one
// lane reached a leaf (measured ~15x instruction overhead from divergence).
__device__ __forceinline__ int knn_search(const KdView &M, float qx, float qy, float qz, float r2,
                                          int K, HeapRef h, uint32_t &visited) {
  int size = 0;
  float maxd2 = r2;
  float topd = 0.f;
  int topi = 0;
  if (M.n == 0) return 0;
  const KdNode *nodes = reinterpret_cast<const KdNode *>(M.nodes);
  const float4 *pos = reinterpret_cast<const float4 *>(M.pos4);
  const int L = M.nleaves;
  int node = 1;
  bool live = true;
  while (true) {
    // walk to the next leaf whose tight box is within the current bound
    int leaf = -1;
    while (live) {
      KdNode nd = nodes[node];
      if (kd_box_d2(nd.lo, nd.hi, qx, qy, qz) <= maxd2) {
        if (node < L) {
          float q = kd_axis_q(__float_as_int(nd.hi.w), qx, qy, qz);
          node = 2 * node + ((q - nd.lo.w >= 0.0f) ? 1 : 0);
          continue;
        }
        leaf = node - L;
        break;
      }
      live = kd_next(nodes, node, qx, qy, qz);
    }
    if (leaf < 0) break;
    int64_t s0, s1;
    kd_leaf_range(M, leaf, s0, s1);
    for (int64_t ii = s0; ii < s1; ii += 4) {
      float4 p[4];
#pragma unroll
      for (int u = 0; u < 4; u++) p[u] = pos[(ii + u < s1) ? ii + u : s1 - 1];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        float d2 = photon_d2(qx, qy, qz, p[u].x, p[u].y, p[u].z);
        if (ii + u < s1 && d2 <= maxd2) {
          int id = (int)(ii + u);
          if (size < K) {
            heap_push(h, size, d2, id);
            if (size == K) {
              topd = h.d2[0];
              topi = h.idx[0];
              maxd2 = topd;
            }
          } else if (heap_less(d2, id, topd, topi)) {
            heap_replace_top(h, size, d2, id);
            topd = h.d2[0];
            topi = h.idx[0];
            maxd2 = topd;
          }
        }
      }
    }
    visited += (uint32_t)(s1 - s0);
    live = kd_next(nodes, node, qx, qy, qz);
  }
  return size;
}

// Each lane answers a.qpl Morton-consecutive queries (q = (block*qpl + it)*64 + lane). After
// the first, the search starts from a proven bound instead of r^2: the K photons found for
// the previous query p all lie within d_K(p) + |q - p| of q (triangle inequality), so
// d_K(q)^2 <= (d_K(p) + |q - p|)^2. A 1e-5 relative margin covers the fp32 metric's
// rounding; the bound only prunes, the result set is unchanged.
// The heaps live in global scratch, so any K works: this is the path for estimate sizes beyond
// the LDS kernels (K + 64 > 1024 photons per query-per-wave candidate buffer).
__global__ __launch_bounds__(64) void knn_kernel(KnnArgs a) {
  int lane = threadIdx.x;
  uint64_t nfound_total = 0, visited_total = 0, nq_done = 0;
  HeapRef h;
  {
    int64_t t = (int64_t)blockIdx.x * 64 + lane;
    h.d2 = a.gheap_d2 + t;
    h.idx = a.gheap_idx + t;
    h.stride = (int)((int64_t)gridDim.x * 64);
  }
  float px = 0.f, py = 0.f, pz = 0.f, pk2 = -1.0f;  // previous query and its K-th d2
  for (int it = 0; it < a.qpl; it++) {
    int64_t q = ((int64_t)blockIdx.x * a.qpl + it) * 64 + lane;
    if (q >= a.nq) break;
    int64_t qg = a.q0 + q;
    int64_t qi = a.perm ? (int64_t)a.perm[qg] : qg;
    float4 qp = a.qpos[qi];
    if (__float_as_uint(qp.w) == QMETA_NONE) continue;  // empty deterministic slot
    float bound = a.r2f;
    if (pk2 >= 0.0f) {
      double dx = (double)qp.x - px, dy = (double)qp.y - py, dz = (double)qp.z - pz;
      double rb = (sqrt((double)pk2) + sqrt(dx * dx + dy * dy + dz * dz)) * (1.0 + 1e-5);
      float b2 = __double2float_ru(rb * rb);
      if (b2 < bound) bound = b2;
    }
    uint32_t visited = 0;
    int num = knn_search(a.map, qp.x, qp.y, qp.z, bound, a.K, h, visited);
    px = qp.x; py = qp.y; pz = qp.z;
    pk2 = (num == a.K) ? h.d2[0] : -1.0f;
    nfound_total += num;
    visited_total += visited;
    nq_done += 1;
    if (a.mode == KNN_MODE_LIST) {
      for (int s = 0; s < a.K; s++) {
        a.out_idx[qi * a.K + s] = (s < num) ? h.idx[s * h.stride] : -1;
        a.out_d2[qi * a.K + s] = (s < num) ? h.d2[s * h.stride] : -1.0f;
      }
      a.out_n[qi] = num;
    } else {
      C3 o = rgb(0.0, 0.0, 0.0);
      double maxd2 = kEps;
      if (num > 0) {
        if (num < a.K) {
          maxd2 = a.rmax * a.rmax;
        } else {
          for (int s = 0; s < num; s++) {
            double d = (double)h.d2[s * h.stride];
            if (d > maxd2) maxd2 = d;
          }
        }
        if (a.mode == KNN_MODE_IRRADIANCE) {
          for (int s = 0; s < num; s++) irradiance_add(a.map.rgbe[h.idx[s * h.stride]], o);
          o = irradiance_finish(o, maxd2);
        } else {
          const EstQuery Q(a, qi, qp.w, maxd2);
          double tw = 0;
          for (int s = 0; s < num; s++) {
            uint32_t id = (uint32_t)h.idx[s * h.stride];
            double ix, iy, iz;
            lut_dir(a, photon_dcode(a, id), ix, iy, iz);
            double perp = Q.perp(ix, iy, iz);
            if (Q.wrong_side(perp)) continue;
            C3 p;
            Q.general_term(a, Q.E, ix, iy, iz, perp, a.map.rgbe[id], (double)h.d2[s * h.stride], p, tw);
            o = o + p;
          }
          est_finish(a, a.filter, Q.sh, num, maxd2, tw, o);
        }
      }
      est_store(a, qi, num, maxd2, o);
    }
  }
  if (a.stats) {
    wave_add(&a.stats[ST_KNN + a.stat_off], nq_done);
    wave_add(&a.stats[ST_KNN_PHOTONS + a.stat_off], nfound_total);
    wave_add(&a.stats[ST_KNN_VISITED + a.stat_off], visited_total);
  }
}

// EstimateCachedRadiance (photon_utils.cpp:165-205) with FindClosest (R3Kdtree.cpp:317-445):
// nearest photon at distance >= previous + 1e-6 until one passes the side test (Q8 guarded).
__global__ __launch_bounds__(64) void cached_kernel(KnnArgs a) {
  int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
  uint64_t nq_done = 0;
  if (q < a.nq && __float_as_uint(a.qpos[q].w) != QMETA_NONE) {
    float4 qp = a.qpos[q];
    nq_done = 1;
    const QShade &sh = a.qshade[q];
    uint32_t meta = __float_as_uint(qp.w);
    uint32_t sign = meta & 3u;
    const DMaterial &m = a.mats[qmeta_mat(meta)];
    double N0 = sh.n[0], N1 = sh.n[1], N2 = sh.n[2];
    double out0 = 0, out1 = 0, out2 = 0;
    double closest = 0;
    const KdNode *nodes = reinterpret_cast<const KdNode *>(a.map.nodes);
    const float4 *pos = reinterpret_cast<const float4 *>(a.map.pos4);
    const int L = a.map.nleaves;
    for (int guard = 0; guard < 1 << 20 && a.map.n > 0; guard++) {
      double mn = closest + kEps;
      float min2 = (float)(mn * mn);
      float best2 = a.r2f;
      int best = -1;
      int node = 1;
      while (true) {
        KdNode nd = nodes[node];
        if (kd_box_d2(nd.lo, nd.hi, qp.x, qp.y, qp.z) <= best2) {
          if (node < L) {
            float qq = kd_axis_q(__float_as_int(nd.hi.w), qp.x, qp.y, qp.z);
            node = 2 * node + ((qq - nd.lo.w >= 0.0f) ? 1 : 0);
            continue;
          }
          int leaf = node - L;
          int64_t s0, s1;
          kd_leaf_range(a.map, leaf, s0, s1);
          for (int64_t ii = s0; ii < s1; ii++) {
            float4 p = pos[ii];
            float d2 = photon_d2(qp.x, qp.y, qp.z, p.x, p.y, p.z);
            if (d2 >= min2 && d2 <= best2 && (d2 < best2 || best < 0 || (int)ii < best)) {
              best2 = d2;
              best = (int)ii;
            }
          }
        }
        while (node != 1) {
          const KdNode &pn = nodes[node >> 1];
          float qq = kd_axis_q(__float_as_int(pn.hi.w), qp.x, qp.y, qp.z);
          int near_is_right = (qq - pn.lo.w >= 0.0f) ? 1 : 0;
          if ((node & 1) == near_is_right) break;
          node >>= 1;
        }
        if (node == 1) break;
        node ^= 1;
      }
      closest = sqrt((double)best2);
      if (best < 0) break;
      // EstimateCachedRadiance's term is its own function in the reference: pow is called
      // whatever the material and there is no filter, so it shares the direction lookup, the
      // side test and the decode with the estimate, not the general term
      double ix, iy, iz;
      lut_dir(a, photon_dcode(a, (uint32_t)best), ix, iy, iz);
      double perp = N0 * ix + N1 * iy + N2 * iz;
      if (wrong_side(sign, perp)) continue;
      C3 p = rgbe_decode(a.map.rgbe[best]);
      double ca = sh.ex[0] * -ix + sh.ex[1] * -iy + sh.ex[2] * -iz;
      if (ca < 0) ca = 0;
      double ap = fabs(perp);
      double pw = gm::pow(ca, m.n);
      double p0 = p.r * (ap * m.kd[0] + pw * m.ks[0]);
      double p1 = p.g * (ap * m.kd[1] + pw * m.ks[1]);
      double p2 = p.b * (ap * m.kd[2] + pw * m.ks[2]);
      out0 = p0 * sh.w[0];
      out1 = p1 * sh.w[1];
      out2 = p2 * sh.w[2];
      break;
    }
    a.out[3 * q] = out0;
    a.out[3 * q + 1] = out1;
    a.out[3 * q + 2] = out2;
  }
  if (a.stats) wave_add(&a.stats[ST_KNN + a.stat_off], nq_done);
}

static inline unsigned nblk(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

void launch_knn(const KnnArgs &a, hipStream_t st) {
  if (a.nq == 0) return;
  knn_kernel<<<nblk(a.nq, 64 * a.qpl), 64, 0, st>>>(a);
}
void launch_cached(const KnnArgs &a, hipStream_t st) {
  if (a.nq == 0) return;
  cached_kernel<<<nblk(a.nq, 64), 64, 0, st>>>(a);
}

}  // namespace gi
