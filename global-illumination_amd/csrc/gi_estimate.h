// gi_estimate.h -- the photon metric and the radiance estimate, each defined once for every
// k-NN kernel (gi_knn.hip, gi_knn_chunk.hip, gi_knn_heap.hip).
//
// EstimateRadiance / EstimateIrradiance (photon_utils.cpp:72-162, 209-246) as the pieces a kernel
// strings together: set-up (EstQuery), a loop that loads a photon and calls a term, the
// kernel's own reduction, est_finish, est_store. A kernel owns how it finds maxd2, the order
// in which it visits photons, its prefetch grouping and its reduction; those set its bits and
// its speed. Everything else is here, so the image comparisons pin one copy.
#pragma once
#include "gi_kernels.h"

namespace gi {

// photon metric: the reference's squared distance in fp32, one fixed operation order (the k-NN
// sets are exact because every kernel and the oracle share it). cand_d2x8 (gi_knn_chunk.hip)
// is the same formula on packed pairs.
__device__ __forceinline__ float photon_d2(float qx, float qy, float qz, float px, float py, float pz) {
  float dx = qx - px, dy = qy - py, dz = qz - pz;
  return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, __fmul_rn(dx, dx)));
}

// pow behind a call: the estimates' specular and Gaussian-filter branches would otherwise inline
// one fp64 pow per unrolled photon (code size, registers) for paths most scenes never take
static __device__ __noinline__ double pow_call(double x, double y) { return gm::pow(x, y); }

// RGBE word -> power (RGBE_to_RNRgb, graphics_utils.cpp:64-77); exponent byte 0: black
__device__ __forceinline__ C3 rgbe_decode(uint32_t e) {
  uint32_t ee = e >> 24;
  double inv = ee ? ldexp(1.0, (int)ee - 128 - 8) : 0.0;
  return rgb(ee ? (double)(e & 255u) * inv : 0.0, ee ? (double)((e >> 8) & 255u) * inv : 0.0,
             ee ? (double)((e >> 16) & 255u) * inv : 0.0);
}

// a photon's direction code and its direction-table entry
__device__ __forceinline__ uint32_t photon_dcode(const KnnArgs &a, uint32_t id) {
  return __float_as_uint(a.map.pos4[4 * (int64_t)id + 3]) & 0xffffu;
}
__device__ __forceinline__ void lut_dir(const KnnArgs &a, uint32_t dcode, double &ix, double &iy, double &iz) {
  ix = a.lut[3 * dcode];
  iy = a.lut[3 * dcode + 1];
  iz = a.lut[3 * dcode + 2];
}

// the side test (photon_utils.cpp:120-123): a photon that arrived on the other side of the
// surface than the query looks at does not count
__device__ __forceinline__ bool wrong_side(uint32_t sign, double perp) {
  return (sign == 2u && perp < 0) || (sign == 1u && perp > 0);
}

// The disk-filter term of a material without a specular term, before kd: power * |N . I|. It
// does not depend on the query's material, so queries with one normal and side can share it
// (chunk_estimate_shared); kd then multiplies the sums once per query.
__device__ __forceinline__ C3 disk_term(double perp, uint32_t e) { return rgbe_decode(e) * fabs(perp); }

// EstimateIrradiance's sum: the photons' power, no side test
__device__ __forceinline__ void irradiance_add(uint32_t e, C3 &o) {
  if (e >> 24) o = o + rgbe_decode(e);
}
__device__ __forceinline__ C3 irradiance_finish(C3 o, double maxd2) { return o / (kPi * maxd2); }

// Per-query set-up of EstimateRadiance, from the query's slot, its meta word (qpos.w) and the
// squared radius of its photon set.
struct EstQuery {
  const QShade &sh;
  const DMaterial &m;
  uint32_t sign;       // side the query looks at (meta bits 0-1)
  double N0, N1, N2;   // surface normal
  V E;                 // exact reflection direction
  bool spec;
  // without the specular term, ap * kd + 0 * ks == ap * kd up to the sign of a zero (for
  // finite ks), and the sums start at +0, so dropping the 0 * ks products changes no result
  bool diff_only;
  double c1 = 1.0, c2 = 1.0;  // filter constants (cone: 1 / (k r); Gauss: e^-b, 1 / (2 r^2))

  __device__ __forceinline__ EstQuery(const KnnArgs &a, int64_t qi, float meta_w, double maxd2)
      : sh(a.qshade[qi]), m(a.mats[qmeta_mat(__float_as_uint(meta_w))]) {
    sign = __float_as_uint(meta_w) & 3u;
    N0 = sh.n[0]; N1 = sh.n[1]; N2 = sh.n[2];
    E = ld3(sh.ex);
    spec = (m.flags & MF_SPECULAR) || (m.n < 0);
    diff_only = !spec && isfinite(m.ks[0]) && isfinite(m.ks[1]) && isfinite(m.ks[2]);
    if (a.filter == 1) c1 = 1.0 / (a.fk * sqrt(maxd2));
    else if (a.filter == 2) {
      c1 = pow_call(2.7182818284590452354, -a.fb);
      c2 = 1.0 / (2.0 * maxd2);
    }
  }

  __device__ __forceinline__ double perp(double ix, double iy, double iz) const {
    return N0 * ix + N1 * iy + N2 * iz;
  }
  __device__ __forceinline__ bool wrong_side(double perp) const { return gi::wrong_side(sign, perp); }

  // The disk-filter term of a material without a specular term, power * |N . I| * kd, with kd
  // inside each term (query-per-wave and per-lane kernels). The chunk kernels use disk_term
  // below and apply kd once to the sums; the bits differ, so both forms stay.
  __device__ __forceinline__ C3 disk_term_kd(double perp, uint32_t e) const {
    C3 p = rgbe_decode(e);
    double ap = fabs(perp);
    p.r *= ap * m.kd[0];
    p.g *= ap * m.kd[1];
    p.b *= ap * m.kd[2];
    return p;
  }

  // The general term: power * (|N . I| kd + pow(ca, n) ks) * filter weight of d2. E is the
  // exact reflection direction: this->E, or the caller's own ld3(sh.ex) where its general loop
  // begins (the chunk kernels: held from the set-up on it costs them spilled registers). The Gauss
  // filter's weight is added to tw for the normalisation (inside its branch, not returned: a
  // returned weight made the compiler merge the cone and Gauss multiplies and moved the
  // query-per-wave instances' register allocation).
  __device__ __forceinline__ void general_term(const KnnArgs &a, const V &E, double ix, double iy, double iz,
                                               double perp, uint32_t e, double d2, C3 &p, double &tw) const {
    p = rgbe_decode(e);
    double ca = E.x * -ix + E.y * -iy + E.z * -iz;
    if (ca < 0) ca = 0;
    double ap = fabs(perp);
    if (diff_only) {
      p.r *= ap * m.kd[0];
      p.g *= ap * m.kd[1];
      p.b *= ap * m.kd[2];
    } else {
      double pw = spec ? pow_call(ca, m.n) : 0.0;
      p.r *= ap * m.kd[0] + pw * m.ks[0];
      p.g *= ap * m.kd[1] + pw * m.ks[1];
      p.b *= ap * m.kd[2] + pw * m.ks[2];
    }
    if (a.filter == 1) {
      double f = (1.0 - c1 * sqrt(d2));
      p.r *= f; p.g *= f; p.b *= f;
    } else if (a.filter == 2) {
      double w = (1.0 - (1.0 - pow_call(c1, c2 * d2)) / (1.0 - c1));
      p.r *= w; p.g *= w; p.b *= w;
      tw += w;
    }
  }
};

// An instance without the general form (KnnArgs::general == 0) met a query that needs it: the
// host's check failed. Count it (the host re-runs with the general instances, gi_host.cpp
// render_common) and make the result unmistakable meanwhile.
__device__ __forceinline__ C3 est_gen_miss(const KnnArgs &a) {
  if (a.stats) atomicAdd(a.stats + ST_GEN_MISS, 1ull);
  return rgb(__builtin_nan(""), __builtin_nan(""), __builtin_nan(""));
}

// The normalisation of the summed terms (photon_utils.cpp:149-158) for `filter` (a.filter, or a
// literal where the caller knows it), times the path weight; zero where it is undefined.
__device__ __forceinline__ void est_finish(const KnnArgs &a, int filter, const QShade &sh, int num,
                                           double maxd2, double tw, C3 &o) {
  bool ok = true;
  if (filter == 0 && maxd2 > 0) {
    o = o / (kPi * maxd2);
  } else if (filter == 1 && maxd2 > 0) {
    o = o / ((1.0 - 2.0 / 3.0 / a.fk) * kPi * maxd2);
  } else if (filter == 2 && tw > 0 && maxd2 > 0) {
    o = o * (a.fa * (num / tw) / (kPi * maxd2));
  } else {
    ok = false;
  }
  if (ok) {
    o.r *= sh.w[0]; o.g *= sh.w[1]; o.b *= sh.w[2];
  } else {
    o.r = o.g = o.b = 0;
  }
}

__device__ __forceinline__ void est_store(const KnnArgs &a, int64_t qi, int num, double maxd2, C3 o) {
  a.out[3 * qi] = o.r;
  a.out[3 * qi + 1] = o.g;
  a.out[3 * qi + 2] = o.b;
  if (a.out_n) a.out_n[qi] = num;
  if (a.out_maxd2) a.out_maxd2[qi] = (num > 0) ? (float)maxd2 : 0.0f;
}

}  // namespace gi
