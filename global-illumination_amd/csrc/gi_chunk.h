// gi_chunk.h -- what the kernels that give one wave a chunk of 64 adjacent queries share
// (gi_knn_chunk.hip, gi_range.hip): the chunk's query load, the LDS candidate arrays and their
// broadcast reads, the box-to-box gap in the photon metric's operation order, and the
// wave-uniform kd walk.
#pragma once
#include "gi_kernels.h"
#include "gi_estimate.h"

namespace gi {

__device__ __forceinline__ float wmaxf(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wminf(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ float metric(float qx, float qy, float qz, const float4 &p) {
  return photon_d2(qx, qy, qz, p.x, p.y, p.z);
}

// The chunk's LDS candidates, structure of arrays: x[CAPC], y[CAPC], z[CAPC], w[CAPC] (w = the
// photon's dir | flags bits). The select loops read four consecutive candidates' x (y, z) with
// one broadcast ds_read_b128 (4 LDS cycles; a float4 per candidate would be a ds_read_b96 at 8
// cycles each, MI355X_MICROARCH.md LDS table).
template <int CAPC>
struct Cands {
  float *b;
  __device__ __forceinline__ float4 get(uint32_t s) const {
    return make_float4(b[s], b[CAPC + s], b[2 * CAPC + s], b[3 * CAPC + s]);
  }
  __device__ __forceinline__ void put(uint32_t s, const float4 &p) const {
    b[s] = p.x; b[CAPC + s] = p.y; b[2 * CAPC + s] = p.z; b[3 * CAPC + s] = p.w;
  }
  __device__ __forceinline__ float wbits(uint32_t s) const { return b[3 * CAPC + s]; }
  // candidates s0 .. s0 + 3 (s0 % 4 == 0) of coordinate c
  __device__ __forceinline__ float4 quad(int c, uint32_t s0) const {
    return *reinterpret_cast<const float4 *>(b + c * CAPC + s0);
  }
  __device__ __forceinline__ float d2(float qx, float qy, float qz, uint32_t s) const {
    return metric(qx, qy, qz, make_float4(b[s], b[CAPC + s], b[2 * CAPC + s], 0.0f));
  }
};

// d2 of the 8 candidates s0 .. s0 + 7 (s0 % 8 == 0, s0 + 8 <= CAPC): six broadcast reads
template <int CAPC>
__device__ __forceinline__ void cand_d2x8(const Cands<CAPC> &C, uint32_t s0, float qx, float qy,
                                          float qz, float (&d)[8]) {
  const float4 x0 = C.quad(0, s0), x1 = C.quad(0, s0 + 4);
  const float4 y0 = C.quad(1, s0), y1 = C.quad(1, s0 + 4);
  const float4 z0 = C.quad(2, s0), z1 = C.quad(2, s0 + 4);
  // metric() in packed pairs, each operation on all four pairs before the next one: no packed
  // result is read by the next instruction (the dependent v_pk_* pairs otherwise take s_nop)
  typedef float f2 __attribute__((ext_vector_type(2)));
  const f2 qx2 = {qx, qx}, qy2 = {qy, qy}, qz2 = {qz, qz};
  const f2 X[4] = {{x0.x, x0.y}, {x0.z, x0.w}, {x1.x, x1.y}, {x1.z, x1.w}};
  const f2 Y[4] = {{y0.x, y0.y}, {y0.z, y0.w}, {y1.x, y1.y}, {y1.z, y1.w}};
  const f2 Z[4] = {{z0.x, z0.y}, {z0.z, z0.w}, {z1.x, z1.y}, {z1.z, z1.w}};
  f2 dx[4], dy[4], dz[4], r[4];
#pragma unroll
  for (int i = 0; i < 4; i++) dx[i] = qx2 - X[i];
#pragma unroll
  for (int i = 0; i < 4; i++) dy[i] = qy2 - Y[i];
#pragma unroll
  for (int i = 0; i < 4; i++) dz[i] = qz2 - Z[i];
#pragma unroll
  for (int i = 0; i < 4; i++) r[i] = dx[i] * dx[i];
#pragma unroll
  for (int i = 0; i < 4; i++) r[i] = __builtin_elementwise_fma(dy[i], dy[i], r[i]);
#pragma unroll
  for (int i = 0; i < 4; i++) r[i] = __builtin_elementwise_fma(dz[i], dz[i], r[i]);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    d[2 * i] = r[i].x;
    d[2 * i + 1] = r[i].y;
  }
}

// squared gap between a point/box and box B, same fp32 operation order as the photon metric
__device__ __forceinline__ float gap2(float lx, float ly, float lz, float hx, float hy, float hz,
                                      const float *bl, const float *bh) {
  float gx = fmaxf(fmaxf(lx - bh[0], bl[0] - hx), 0.0f);
  float gy = fmaxf(fmaxf(ly - bh[1], bl[1] - hy), 0.0f);
  float gz = fmaxf(fmaxf(lz - bh[2], bl[2] - hz), 0.0f);
  return __builtin_fmaf(gz, gz, __builtin_fmaf(gy, gy, __fmul_rn(gx, gx)));
}

// Wave-uniform walk over every kd leaf whose node box passes boxd(node) <= bound, with a
// per-wave LDS stack (stk, >= tree depth entries): an expansion reads both children's boxes
// (scalar loads, ld_node) and pushes one, so backtracking reads nothing from memory. leaf(l)
// returns true to stop the walk. Returns the number of node records read.
//
// Two levels per round trip: an expansion whose children are internal also reads the four grandchildren (128
// contiguous bytes, issued with the children's 64): two levels per dependent round trip. A
// grandchild is taken when its parent and its own box pass, as two single-level expansions
// would take it, and the in-grandchildren are pushed right to left, so leaves are still visited
// left to right: the callers' LDS candidate order, and so every estimate sum, is unchanged.
// Stack: at most three entries per two levels.
//
// Leaf sweep: a node with at most 2^CHUNK_SWEEP_H leaves below it is not expanded further; its
// leaf boxes are read in one vector load (lane i: leaf i) and the passing leaves are visited in
// index order. A leaf's tight box lies inside every ancestor's and boxd is monotone under
// containment (the same fp operation sequence, every rounding monotone), so the leaves that
// pass are exactly those the node-by-node walk reaches, in the same left-to-right order: the
// candidate order, and every result, are unchanged; the bottom levels' dependent node loads
// become one round trip per subtree.
#ifndef CHUNK_SWEEP_H
#define CHUNK_SWEEP_H 6
#endif
static_assert(CHUNK_SWEEP_H >= 0 && CHUNK_SWEEP_H <= 6, "leaf sweep: one leaf per lane of a 64-wide wave");
template <typename BoxD, typename Leaf>
__device__ __forceinline__ uint32_t walk_within(const float *nodes, int L, float bound, uint32_t *stk,
                                                BoxD boxd, Leaf leaf, int root = 1) {
  const int levels = 31 - __clz(L);
  const int lane = threadIdx.x & 63;
  uint32_t reads = 1;
  int sp = 0;
  int node = (boxd(ld_node(nodes, root)) <= bound) ? root : 0;
  while (node) {
    node = __builtin_amdgcn_readfirstlane(node);
    const int h = levels - (31 - __clz(node));
    if (h <= CHUNK_SWEEP_H) {
      const int lf0 = node << h;
      bool in = false;
      if (lane < (1 << h)) in = boxd(reinterpret_cast<const KdNode *>(nodes)[lf0 + lane]) <= bound;
      reads += 1u << h;
      uint64_t m = __ballot(in);
      while (m) {
        const int li = __ffsll((long long)m) - 1;
        m &= m - 1ull;
        if (leaf(lf0 + li - L)) return reads;
      }
    } else {
      const int c = 2 * node;
      KdNode c0 = ld_node(nodes, c), c1 = ld_node(nodes, c + 1);
      if (h > CHUNK_SWEEP_H + 1) {
        KdNode g0 = ld_node(nodes, 2 * c), g1 = ld_node(nodes, 2 * c + 1);
        KdNode g2 = ld_node(nodes, 2 * c + 2), g3 = ld_node(nodes, 2 * c + 3);
        reads += 6;
        const bool in0 = boxd(c0) <= bound, in1 = boxd(c1) <= bound;
        const bool i0 = in0 && boxd(g0) <= bound, i1 = in0 && boxd(g1) <= bound;
        const bool i2 = in1 && boxd(g2) <= bound, i3 = in1 && boxd(g3) <= bound;
        const int nxt = i0 ? 2 * c : (i1 ? 2 * c + 1 : (i2 ? 2 * c + 2 : (i3 ? 2 * c + 3 : 0)));
        // every lane stores the same values
        if (i3 && nxt != 2 * c + 3) stk[sp++] = (uint32_t)(2 * c + 3);
        if (i2 && nxt != 2 * c + 2) stk[sp++] = (uint32_t)(2 * c + 2);
        if (i1 && nxt != 2 * c + 1) stk[sp++] = (uint32_t)(2 * c + 1);
        if (nxt) { node = nxt; continue; }
      } else {
        reads += 2;
        bool in0 = boxd(c0) <= bound, in1 = boxd(c1) <= bound;
        if (in0 && in1) {
          stk[sp] = (uint32_t)(c + 1);  // every lane stores the same value
          sp++;
        }
        if (in0) { node = c; continue; }
        if (in1) { node = c + 1; continue; }
      }
    }
    node = 0;
    if (sp > 0) {
      sp--;
      node = (int)__builtin_amdgcn_readfirstlane((int)stk[sp]);
    }
  }
  return reads;
}

__device__ __forceinline__ void chunk_load_query(const KnnArgs &a, int64_t chunk, int lane, bool &valid,
                                                 int64_t &qi, float4 &qp) {
  int64_t qs = chunk * 64 + lane;
  valid = qs < a.nq;
  qi = 0;
  qp = make_float4(0.f, 0.f, 0.f, 0.f);
  if (valid) {
    qi = a.perm ? (int64_t)a.perm[a.q0 + qs] : a.q0 + qs;
    qp = a.qpos[qi];
    valid = __float_as_uint(qp.w) != QMETA_NONE;
  }
}

}  // namespace gi
