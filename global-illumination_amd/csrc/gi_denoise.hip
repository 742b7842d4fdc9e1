// gi_denoise.hip -- per-pixel feature planes and the edge-avoiding a-trous denoise pass (gfx950).
// No reference counterpart (the reference writes the noisy frame only). DESIGN.md "Feature
// planes and denoise pass" holds the definitions; tests/denoise_ref.py restates them in numpy
// and both kernels match it bit for bit: every operation here is one of + - * / max sqrt in
// fp64 on float32 inputs, compiled with -ffp-contract=off.
//
//   feature_trace_kernel   one thread per sample ray: closest hit (scene_intersect, as the
//                          R3Scene::Intersects test seam calls it), normal, distance, material
//   feature_reduce_kernel  one thread per pixel: its samples summed in sample order
//   denoise_level_kernel   one a-trous level (5 x 5 B3 taps at step 2^l), thread per pixel
//   vdenoise_level_kernel  the same for radiance frames, the colour stop scaled by each pixel's
//                          own variance (DESIGN.md "Variance-guided denoise";
//                          tests/vdenoise_ref.py), with its pack / unpack kernels
#include <hip/hip_runtime.h>
#include "gi_denoise.h"

namespace gi {

static inline unsigned nblk(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

// ---------------------------------------------------------------------------------------
// feature planes
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void feature_trace_kernel(FeatureArgs a) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= a.nsamp) return;
  const double2 *r = reinterpret_cast<const double2 *>(a.rays + s);
  const double2 r0 = r[0], r1 = r[1], r2 = r[2];
  const V org = {r0.x, r0.y, r1.x}, dir = {r1.y, r2.x, r2.y};
  Hit h;
  FeatSample f;
  f.n[0] = f.n[1] = f.n[2] = 0.0;
  f.d = 0.0;
  f.mat = -2;
  f.hit = 0;
  if (scene_intersect(a.S, org, dir, h)) {
    const V d = h.p - org;
    f.n[0] = h.n.x; f.n[1] = h.n.y; f.n[2] = h.n.z;
    f.d = sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
    f.mat = h.mat;
    f.hit = 1;
  }
  a.samples[s] = f;
}

__global__ __launch_bounds__(256) void feature_reduce_kernel(FeatureArgs a) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.npix) return;
  const FeatSample *f = a.samples + p * a.spp;
  double nx = 0.0, ny = 0.0, nz = 0.0, d = 0.0, ar = 0.0, ag = 0.0, ab = 0.0;
  int hits = 0;
  for (int k = 0; k < a.spp; k++) {
    if (!f[k].hit) continue;
    const DMaterial &m = a.S.mats[f[k].mat];
    nx += f[k].n[0]; ny += f[k].n[1]; nz += f[k].n[2];
    d += f[k].d;
    ar += m.kd[0]; ag += m.kd[1]; ab += m.kd[2];
    hits++;
  }
  float4 o0 = make_float4(0.f, 0.f, 0.f, 0.f), o1 = o0;
  if (hits) {
    const double hn = (double)hits;
    o0 = make_float4((float)(nx / hn), (float)(ny / hn), (float)(nz / hn), (float)(d / hn));
    o1 = make_float4((float)(ar / hn), (float)(ag / hn), (float)(ab / hn),
                     (float)(hn / (double)a.spp));
  }
  a.planes[2 * p] = o0;
  a.planes[2 * p + 1] = o1;
}

void launch_feature_trace(const FeatureArgs &a, hipStream_t st) {
  if (a.nsamp > 0) feature_trace_kernel<<<nblk(a.nsamp, 128), 128, 0, st>>>(a);
}
void launch_feature_reduce(const FeatureArgs &a, hipStream_t st) {
  if (a.npix > 0) feature_reduce_kernel<<<nblk(a.npix, 256), 256, 0, st>>>(a);
}

// ---------------------------------------------------------------------------------------
// denoise: one a-trous level
// ---------------------------------------------------------------------------------------
// Block 64 x 4: a wave is 64 consecutive x of one row, so each tap is one coalesced row segment
// of three 16-B loads per lane (colour, {normal, depth}, {albedo, coverage}). The 25 taps are
// unrolled (j = -2..2 rows outer, i = -2..2 inner: the summation order of the definition); the
// taps of neighbouring lanes and rows overlap, which the L1 / L2 serve. No LDS, no atomics.
__global__ __launch_bounds__(256) void denoise_level_kernel(DenoiseArgs a) {
  // blocks in a 1-D grid, row-major over the (W / 64) x (H / 4) block tiles: any H fits
  const unsigned nbx = (unsigned)((a.W + 63) / 64);
  const int x = (int)((blockIdx.x % nbx) * 64 + threadIdx.x);
  const int y = (int)((blockIdx.x / nbx) * 4 + threadIdx.y);
  if (x >= a.W || y >= a.H) return;
  const size_t p = (size_t)y * a.W + x;
  const float4 cp = a.src[p], np = a.planes[2 * p], ap = a.planes[2 * p + 1];
  const bool cov_p = ap.w > 0.0f;
  const double kk[3] = {0.375, 0.25, 0.0625};
  double sw = 0.0, sr = 0.0, sg = 0.0, sb = 0.0;
#pragma unroll
  for (int j = -2; j <= 2; j++) {
#pragma unroll
    for (int i = -2; i <= 2; i++) {
      const int qx = x + a.step * i, qy = y + a.step * j;
      if (qx < 0 || qx >= a.W || qy < 0 || qy >= a.H) continue;
      const double h = kk[i < 0 ? -i : i] * kk[j < 0 ? -j : j];
      double w;
      float4 cq;
      if (i == 0 && j == 0) {
        cq = cp;
        w = h;
      } else {
        const size_t q = (size_t)qy * a.W + qx;
        cq = a.src[q];
        const float4 nq = a.planes[2 * q], aq = a.planes[2 * q + 1];
        const bool cov_q = aq.w > 0.0f;
        if (cov_p != cov_q) continue;  // w = 0
        const double dr = (double)cp.x - (double)cq.x, dg = (double)cp.y - (double)cq.y,
                     db = (double)cp.z - (double)cq.z;
        const double xc = (dr * dr + dg * dg + db * db) / a.sc2;
        if (cov_p) {
          double m = (double)np.x * (double)nq.x + (double)np.y * (double)nq.y +
                     (double)np.z * (double)nq.z;
          m = fmax(0.0, m);
          for (int e = 0; e < a.npow; e++) m = m * m;
          const double xz = ((double)np.w - (double)nq.w) /
                            (a.sigma_depth * ((double)np.w + (double)nq.w));
          const double er = (double)ap.x - (double)aq.x, eg = (double)ap.y - (double)aq.y,
                       eb = (double)ap.z - (double)aq.z;
          const double xa = (er * er + eg * eg + eb * eb) / a.sa2;
          w = (h * m) / (((1.0 + xc) * (1.0 + xz * xz)) * (1.0 + xa));
        } else {
          w = h / (1.0 + xc);
        }
      }
      sw += w;
      sr += w * (double)cq.x;
      sg += w * (double)cq.y;
      sb += w * (double)cq.z;
    }
  }
  a.dst[p] = make_float4((float)(sr / sw), (float)(sg / sw), (float)(sb / sw), 0.0f);
}

__global__ __launch_bounds__(256) void denoise_pack_kernel(const float *rgbf, int64_t npix,
                                                           float4 *img) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < npix) img[p] = make_float4(rgbf[3 * p], rgbf[3 * p + 1], rgbf[3 * p + 2], 0.0f);
}
__global__ __launch_bounds__(256) void denoise_unpack_kernel(const float4 *img, int64_t npix,
                                                             float *rgbf) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const float4 c = img[p];
  rgbf[3 * p] = c.x; rgbf[3 * p + 1] = c.y; rgbf[3 * p + 2] = c.z;
}

// ---------------------------------------------------------------------------------------
// variance-guided denoise of radiance frames: one level
// ---------------------------------------------------------------------------------------
// Same shape as denoise_level_kernel (block 64 x 4, thread per pixel, three 16-B loads per tap,
// 25 taps unrolled in the defined order, no LDS, no atomics); the image's fourth float carries the
// variance of the pixel's luminance. The colour stop's bandwidth is the pixel's own: il = 1 /
// (sigma_lum^2 g + floor) with g the 3 x 3 prefiltered variance, computed inline from nine step-1
// taps that the level's own centre rows have in cache (no pre-pass plane, no launch of its own).
// Every weight is one quotient: the depth stop is folded into numerator and denominator, the
// albedo stop multiplies by 1 / sigma_albedo^2.
__device__ __forceinline__ double luma(const float4 c) {
  return 0.2126 * (double)c.x + 0.7152 * (double)c.y + 0.0722 * (double)c.z;
}

__global__ __launch_bounds__(256) void vdenoise_level_kernel(VDenoiseArgs a) {
  const unsigned nbx = (unsigned)((a.W + 63) / 64);
  const int x = (int)((blockIdx.x % nbx) * 64 + threadIdx.x);
  const int y = (int)((blockIdx.x / nbx) * 4 + threadIdx.y);
  if (x >= a.W || y >= a.H) return;
  const size_t p = (size_t)y * a.W + x;
  const float4 cp = a.src[p], np = a.planes[2 * p], ap = a.planes[2 * p + 1];
  const bool cov_p = ap.w > 0.0f;
  // prefiltered variance -> inverse squared bandwidth of the luminance stop
  const double k3[2] = {0.5, 0.25};
  double sh = 0.0, sg = 0.0;
#pragma unroll
  for (int j = -1; j <= 1; j++) {
#pragma unroll
    for (int i = -1; i <= 1; i++) {
      const int qx = x + i, qy = y + j;
      if (qx < 0 || qx >= a.W || qy < 0 || qy >= a.H) continue;
      const double h3 = k3[i < 0 ? -i : i] * k3[j < 0 ? -j : j];
      const float vq = (i == 0 && j == 0) ? cp.w : a.src[(size_t)qy * a.W + qx].w;
      sh += h3;
      sg += h3 * (double)vq;
    }
  }
  const double il = 1.0 / (a.sl2 * (sg / sh) + a.vfloor);
  const double yp = luma(cp);
  const double kk[3] = {0.375, 0.25, 0.0625};
  double sw = 0.0, sr = 0.0, sgr = 0.0, sb = 0.0, sv = 0.0;
#pragma unroll
  for (int j = -2; j <= 2; j++) {
#pragma unroll
    for (int i = -2; i <= 2; i++) {
      const int qx = x + a.step * i, qy = y + a.step * j;
      if (qx < 0 || qx >= a.W || qy < 0 || qy >= a.H) continue;
      const double h = kk[i < 0 ? -i : i] * kk[j < 0 ? -j : j];
      double w;
      float4 cq;
      if (i == 0 && j == 0) {
        cq = cp;
        w = h;
      } else {
        const size_t q = (size_t)qy * a.W + qx;
        cq = a.src[q];
        const float4 nq = a.planes[2 * q], aq = a.planes[2 * q + 1];
        const bool cov_q = aq.w > 0.0f;
        if (cov_p != cov_q) continue;  // w = 0
        const double dy = yp - luma(cq);
        const double xl = (dy * dy) * il;
        if (cov_p) {
          double m = (double)np.x * (double)nq.x + (double)np.y * (double)nq.y +
                     (double)np.z * (double)nq.z;
          m = fmax(0.0, m);
          for (int e = 0; e < a.npow; e++) m = m * m;
          const double dz = (double)np.w - (double)nq.w, zs = (double)np.w + (double)nq.w;
          const double zz = a.sd2 * (zs * zs);
          const double er = (double)ap.x - (double)aq.x, eg = (double)ap.y - (double)aq.y,
                       eb = (double)ap.z - (double)aq.z;
          const double xa = (er * er + eg * eg + eb * eb) * a.isa2;
          w = ((h * m) * zz) / (((1.0 + xl) * (zz + dz * dz)) * (1.0 + xa));
        } else {
          w = h / (1.0 + xl);
        }
      }
      sw += w;
      sr += w * (double)cq.x;
      sgr += w * (double)cq.y;
      sb += w * (double)cq.z;
      sv += (w * w) * (double)cq.w;
    }
  }
  a.dst[p] = make_float4((float)(sr / sw), (float)(sgr / sw), (float)(sb / sw),
                         (float)(sv / (sw * sw)));
}

// v0 of three channel variances of the mean (floats): the accumulator's luminance-variance form
__device__ __forceinline__ float lum_variance(float vr, float vg, float vb) {
  return (float)((0.2126 * 0.2126) * (double)vr + (0.7152 * 0.7152) * (double)vg +
                 (0.0722 * 0.0722) * (double)vb);
}

__global__ __launch_bounds__(256) void vdenoise_pack_kernel(const float *mean, const float *var3,
                                                            int64_t npix, float4 *img) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  img[p] = make_float4(mean[3 * p], mean[3 * p + 1], mean[3 * p + 2],
                       lum_variance(var3[3 * p], var3[3 * p + 1], var3[3 * p + 2]));
}

// straight from the accumulator: the floats radiance_resolve_kernel hands to gi_accum_get
__global__ __launch_bounds__(256) void vdenoise_pack_accum_kernel(const double *acc,
                                                                  const int64_t *counts,
                                                                  int64_t npix, float4 *img) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const double *f = acc + p * 6;
  const int64_t np = counts[p];
  const double n = (double)np, n1 = (double)(np - 1);
  float v[3];
  for (int c = 0; c < 3; c++) v[c] = np < 2 ? 0.0f : (float)(f[3 + c] / n1 / n);
  img[p] = make_float4((float)f[0], (float)f[1], (float)f[2], lum_variance(v[0], v[1], v[2]));
}

__global__ __launch_bounds__(256) void vdenoise_unpack_kernel(const float4 *img, int64_t npix,
                                                              float *rgbf, float *vlum) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const float4 c = img[p];
  if (rgbf) { rgbf[3 * p] = c.x; rgbf[3 * p + 1] = c.y; rgbf[3 * p + 2] = c.z; }
  if (vlum) vlum[p] = c.w;
}

void launch_vdenoise_level(const VDenoiseArgs &a, hipStream_t st) {
  if (a.W <= 0 || a.H <= 0) return;
  const dim3 block(64, 4);
  const int64_t nb = (int64_t)((a.W + 63) / 64) * ((a.H + 3) / 4);  // < 2^31: W * H is
  vdenoise_level_kernel<<<dim3((unsigned)nb), block, 0, st>>>(a);
}
void launch_vdenoise_pack(const float *mean, const float *var3, int64_t npix, float4 *img,
                          hipStream_t st) {
  if (npix > 0) vdenoise_pack_kernel<<<nblk(npix, 256), 256, 0, st>>>(mean, var3, npix, img);
}
void launch_vdenoise_pack_accum(const double *acc, const int64_t *counts, int64_t npix, float4 *img,
                                hipStream_t st) {
  if (npix > 0) vdenoise_pack_accum_kernel<<<nblk(npix, 256), 256, 0, st>>>(acc, counts, npix, img);
}
void launch_vdenoise_unpack(const float4 *img, int64_t npix, float *rgbf, float *vlum,
                            hipStream_t st) {
  if (npix > 0) vdenoise_unpack_kernel<<<nblk(npix, 256), 256, 0, st>>>(img, npix, rgbf, vlum);
}

void launch_denoise_level(const DenoiseArgs &a, hipStream_t st) {
  if (a.W <= 0 || a.H <= 0) return;
  const dim3 block(64, 4);
  const int64_t nb = (int64_t)((a.W + 63) / 64) * ((a.H + 3) / 4);  // < 2^31: W * H is
  denoise_level_kernel<<<dim3((unsigned)nb), block, 0, st>>>(a);
}
void launch_denoise_pack(const float *rgbf, int64_t npix, float4 *img, hipStream_t st) {
  if (npix > 0) denoise_pack_kernel<<<nblk(npix, 256), 256, 0, st>>>(rgbf, npix, img);
}
void launch_denoise_unpack(const float4 *img, int64_t npix, float *rgbf, hipStream_t st) {
  if (npix > 0) denoise_unpack_kernel<<<nblk(npix, 256), 256, 0, st>>>(img, npix, rgbf);
}

}  // namespace gi
