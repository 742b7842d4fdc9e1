// gi_range.hip -- fixed-radius radiance / irradiance estimate (k-NN kind 10) for chunks of 64
// Morton-adjacent queries.
//
// EstimateRadiance / EstimateIrradiance (photon_utils.cpp:72-162, 209-246) for an estimate size
// no query reaches (K > n photons in the map): every photon with d2 <= r2 counts and the
// normalisation is max_dist^2. That is a range sum: nothing is selected, so there are no
// bracket passes, no heaps, no overflow and no fallback list. One wave per chunk:
//   1. gather: one wave-uniform kd walk (walk_within, box-to-box pruning against r2) stages
//      every photon within r of the chunk's query box B into LDS (position, dir bits, rgbe),
//      ballot-compacted, leaves left to right.
//   2. fold: when the staging arrays are full (and once more after the walk), lane j adds the
//      staged photons within r of its own query j to its running sums, in staged order; the
//      arrays restart and the walk goes on. A lane therefore adds its photons in ascending
//      kd-order position whatever the tile size and whatever else its chunk holds.
//   3. finish: est_finish with maxd2 = r^2 and the count of in-range photons, est_store.
#include <hip/hip_runtime.h>
#include "gi_device.h"
#include "gi_kernels.h"
#include "gi_estimate.h"
#include "gi_chunk.h"

namespace gi {

#ifndef RANGE_CAPC
#define RANGE_CAPC 256         // photons staged per tile: 20 B each, 5.4 KB of LDS per wave
#endif
#ifndef RANGE_WPE
#define RANGE_WPE 4            // occupancy target (waves per SIMD)
#endif
static_assert(RANGE_CAPC % 64 == 0, "a staged batch of up to 64 photons always fits an empty tile");

// how a lane's query sums its photons
enum { RP_IRRADIANCE = 0, RP_DISK = 1, RP_GENERAL = 2, RP_MISS = 3 };

template <int MODE, bool GEN>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RANGE_WPE)))
void knn_range_kernel(KnnArgs a) {
  constexpr int CAPC = RANGE_CAPC;
  __shared__ __attribute__((aligned(16))) float cand_lds[4 * CAPC];
  __shared__ uint32_t crgbe[CAPC];
  __shared__ uint32_t stk[64];
  const Cands<CAPC> cpos{cand_lds};
  const float4 *pos = reinterpret_cast<const float4 *>(a.map.pos4);
  const int L = a.map.nleaves;
  const int64_t N = a.map.n;
  const int lane = threadIdx.x;
  const float r2f = a.r2f;
  const double maxd2 = a.rmax * a.rmax;
  uint64_t st_q = 0, st_found = 0, st_vis = 0;
  for (int64_t chunk = blockIdx.x; chunk * 64 < a.nq; chunk += gridDim.x) {
    bool valid;
    int64_t qi;
    float4 qp;
    chunk_load_query(a, chunk, lane, valid, qi, qp);
    const uint64_t vmask = __ballot(valid);
    if (vmask == 0) continue;
    // idle lanes take the first valid lane's query: their set-up reads stay inside the arrays,
    // and they accept and store nothing
    const int L0 = __ffsll((long long)vmask) - 1;
    const int64_t qs = valid ? qi : __shfl(qi, L0, 64);
    const float qw = valid ? qp.w : __shfl(qp.w, L0, 64);
    float bl[3], bh[3];
    bl[0] = wminf(valid ? qp.x : INFINITY); bh[0] = wmaxf(valid ? qp.x : -INFINITY);
    bl[1] = wminf(valid ? qp.y : INFINITY); bh[1] = wmaxf(valid ? qp.y : -INFINITY);
    bl[2] = wminf(valid ? qp.z : INFINITY); bh[2] = wmaxf(valid ? qp.z : -INFINITY);
    const float qx = qp.x, qy = qp.y, qz = qp.z;

    // per-lane running sums; num counts the in-range photons before the side test
    C3 o = rgb(0.0, 0.0, 0.0);
    double tw = 0.0;
    int num = 0;
    uint32_t count = 0;   // photons staged in the current tile (wave-uniform)
    uint64_t staged = 0;  // ... in all tiles of the chunk

    auto run = [&](auto term) {
      // the staged tile into the lanes' sums, in staged order. Groups of 8: the d2 of a group
      // from six broadcast reads; a photon some lane accepts is then read once for the wave
      // (its slot is wave-uniform: LDS broadcasts, one direction-table row) and added by the
      // lanes that accept it.
      auto fold = [&]() {
        if (lane < 8 && (count & 7u) != 0u && count + lane < ((count + 7u) & ~7u))
          cpos.put(count + lane, make_float4(INFINITY, INFINITY, INFINITY, 0.0f));
        __syncthreads();
        for (uint32_t s0 = 0; s0 < count; s0 += 8) {
          float dg[8];
          cand_d2x8(cpos, s0, qx, qy, qz, dg);
          uint32_t mine = 0, any = 0;
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const bool acc = valid && dg[u] >= 0.0f && dg[u] <= r2f;  // inclusive, as kd_quick
            mine |= acc ? (1u << u) : 0u;
            any |= __ballot(acc) ? (1u << u) : 0u;
          }
          num += __popc(mine);
          while (any) {  // wave-uniform
            const uint32_t u = (uint32_t)__ffs(any) - 1u;
            any &= any - 1u;
            const uint32_t slot = s0 + u;
            const float4 p = cpos.get(slot);
            const uint32_t e = crgbe[slot];
            term((mine >> u) & 1u, p, e);
          }
        }
        __syncthreads();
        staged += count;
        count = 0;
      };
      if (N > 0) {
        walk_within(a.map.nodes, L, r2f, stk,
            [&](const KdNode &b) {
              return gap2(b.lo.x, b.lo.y, b.lo.z, b.hi.x, b.hi.y, b.hi.z, bl, bh);
            },
            [&](int leaf) {
              int64_t s0, s1;
              kd_leaf_range(a.map, leaf, s0, s1);
              for (int64_t b = s0; b < s1; b += 64) {
                int64_t ii = b + lane;
                bool take = false;
                float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
                uint32_t e = 0u;
                if (ii < s1) {
                  p = pos[ii];
                  e = a.map.rgbe[ii];  // issued with the position: no second round trip per leaf
                  take = gap2(p.x, p.y, p.z, p.x, p.y, p.z, bl, bh) <= r2f;
                }
                uint64_t m = __ballot(take);
                uint32_t nn = (uint32_t)__popcll(m);
                if (count + nn > (uint32_t)CAPC) fold();  // the tile is full: fold it, restart
                if (take) {
                  uint32_t off = count + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                  cpos.put(off, p);
                  crgbe[off] = e;
                }
                count += nn;
              }
              return false;
            });
        fold();
      }
    };

    if constexpr (MODE == KNN_MODE_IRRADIANCE) {
      run([&](bool acc, const float4 &, uint32_t e) {
        if (acc) irradiance_add(e, o);
      });
      if (num > 0) o = irradiance_finish(o, maxd2);
    } else {
      const EstQuery Q(a, qs, qw, maxd2);
      const int path = (a.filter == 0 && Q.diff_only) ? RP_DISK : (GEN ? RP_GENERAL : RP_MISS);
      const V E = Q.E;
      run([&](bool acc, const float4 &p, uint32_t e) {
        double ix, iy, iz;
        lut_dir(a, __float_as_uint(p.w) & 0xffffu, ix, iy, iz);  // one row for the wave
        const double perp = Q.perp(ix, iy, iz);
        if (!acc || Q.wrong_side(perp)) return;
        if (path == RP_DISK) {
          // the chunk kernels' form: the terms summed from +0, kd applied once to the sums
          o = o + disk_term(perp, e);
        } else if constexpr (GEN) {
          if (path == RP_GENERAL) {
            const double d2 = (double)metric(qx, qy, qz, p);
            C3 t;
            Q.general_term(a, E, ix, iy, iz, perp, e, d2, t, tw);
            o = o + t;
          }
        }
      });
      if (num > 0) {
        if (path == RP_DISK) o = o * ldc(Q.m.kd);
        else if (path == RP_MISS) o = est_gen_miss(a);
        est_finish(a, a.filter, Q.sh, num, maxd2, tw, o);
      }
    }
    if (valid) {
      if (num == 0) o = rgb(0.0, 0.0, 0.0);
      est_store(a, qi, num, maxd2, o);
      st_q += 1;
      st_found += (uint64_t)num;
      st_vis += staged;
    }
  }
  if (a.stats) {
    wave_add(&a.stats[ST_KNN + a.stat_off], st_q);
    wave_add(&a.stats[ST_KNN_PHOTONS + a.stat_off], st_found);
    wave_add(&a.stats[ST_KNN_VISITED + a.stat_off], st_vis);
  }
}

// fixed-radius estimate (needs K > a.map.n: every query's photon count stays below K, so the
// normalisation is r^2 throughout)
bool launch_knn_range(const KnnArgs &a, hipStream_t st) {
  if (a.nq == 0) return true;
  if ((a.mode != KNN_MODE_RADIANCE && a.mode != KNN_MODE_IRRADIANCE) || (int64_t)a.K <= a.map.n)
    return false;
  const unsigned grid = knn_chunk_grid(a.nq);
  if (a.mode == KNN_MODE_IRRADIANCE) knn_range_kernel<KNN_MODE_IRRADIANCE, false><<<grid, 64, 0, st>>>(a);
  else if (a.general) knn_range_kernel<KNN_MODE_RADIANCE, true><<<grid, 64, 0, st>>>(a);
  else knn_range_kernel<KNN_MODE_RADIANCE, false><<<grid, 64, 0, st>>>(a);
  return true;
}

}  // namespace gi
