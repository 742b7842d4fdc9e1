// gi_radiance.hip -- unclamped radiance frames, the accumulator over passes and the tone map
// (gfx950). No reference counterpart (the reference keeps the clamped 8-bit frame only).
// DESIGN.md "Radiance frames, accumulation and tone map" holds the definitions;
// tests/radiance_ref.py restates them in numpy and every kernel matches it bit for bit: each
// operation here is one of + - * / sqrt in fp64, left to right, compiled with -ffp-contract=off.
//
//   reduce_radiance_kernel   one thread per output pixel of a batch: the samples reduce_kernel
//                            clamps, unclamped; their box-filtered mean m and M2 = sum (s - m)^2
//   accum_merge_kernel       one thread per pixel: a finished pass folded into the accumulator
//   radiance_resolve_kernel  {m, M2} of n samples -> float mean and variance of the mean
//   accum_noise_kernel       relative standard error of luminance, block tree sum
//   count_stats_kernel       smallest and summed per-pixel sample count
//   tile_error_kernel        adaptive passes: the same error per tile, one wave per tile
//   tile_select_kernel       ... and the tile mask (thresholds, 8-neighbour dilation)
//   accum_reproject_kernel   the accumulator carried into a new camera (tests/reproject_ref.py)
//   accum_fold_states_kernel exported accumulator states folded into the accumulator, K at a time
//                            (tests/accum_state_ref.py)
//   tonemap_kernel           exposure, extended Reinhard curve, clamp
#include <hip/hip_runtime.h>
#include "gi_radiance.h"

namespace gi {

static inline unsigned nblk(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

// sample j of batch pixel pix: reduce_kernel's value before its clamp
__device__ __forceinline__ void radiance_sample(const RadianceArgs &a, int pix, int j, double &s0,
                                                double &s1, double &s2) {
  s0 = 0; s1 = 0; s2 = 0;
  for (int k = 0; k < a.dof_test; k++) {
    const int64_t b = ((int64_t)pix * a.S + j) * a.dof_test + k;
    s0 += a.prim_rgb[3 * b];
    s1 += a.prim_rgb[3 * b + 1];
    s2 += a.prim_rgb[3 * b + 2];
  }
  s0 /= a.dof_test; s1 /= a.dof_test; s2 /= a.dof_test;
}

// The second loop reads the pixel's primaries again (S * dof_test * 24 B, just read: L2) rather
// than keeping S samples in registers, so S is not bounded.
__global__ __launch_bounds__(64) void reduce_radiance_kernel(RadianceArgs a) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= a.npix) return;
  const int2 pc = a.pixels[pix];
  const int64_t o = (int64_t)pc.y * a.out_w + pc.x;
  double *smp = a.samples ? a.samples + o * a.S * 3 : nullptr;
  double acc0 = 0, acc1 = 0, acc2 = 0;
  for (int j = 0; j < a.S; j++) {
    double s0, s1, s2;
    radiance_sample(a, pix, j, s0, s1, s2);
    if (smp) {
      smp[3 * j] = s0;
      smp[3 * j + 1] = s1;
      smp[3 * j + 2] = s2;
    }
    acc0 += s0; acc1 += s1; acc2 += s2;
  }
  const double m0 = a.bw * acc0, m1 = a.bw * acc1, m2 = a.bw * acc2;
  double q0 = 0, q1 = 0, q2 = 0;
  for (int j = 0; j < a.S; j++) {
    double s0, s1, s2;
    radiance_sample(a, pix, j, s0, s1, s2);
    q0 += (s0 - m0) * (s0 - m0);
    q1 += (s1 - m1) * (s1 - m1);
    q2 += (s2 - m2) * (s2 - m2);
  }
  double *f = a.frame + o * 6;
  f[0] = m0; f[1] = m1; f[2] = m2;
  f[3] = q0; f[4] = q1; f[5] = q2;
}

// Chan et al.'s pairwise update of (count, mean, M2); an empty accumulator takes the pass as is
// (each pixel under its own count: a masked pass leaves the pixels outside its list behind)
__global__ __launch_bounds__(256) void accum_merge_kernel(AccumArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.npix) return;
  int64_t p = i;
  if (a.pixels) {
    const int2 pc = a.pixels[i];
    p = (int64_t)pc.y * a.width + pc.x;
  }
  const double *f = a.pass + p * 6;
  double *g = a.acc + p * 6;
  const int64_t N = a.counts[p];
  a.counts[p] = N + a.S;
  if (N == 0) {
    for (int c = 0; c < 6; c++) g[c] = f[c];
    return;
  }
  const double S = (double)a.S, N1 = (double)(N + a.S), NS = (double)N * S;
  for (int c = 0; c < 3; c++) {
    const double d = f[c] - g[c];
    g[c] = g[c] + (d * S) / N1;
    g[3 + c] = (g[3 + c] + f[3 + c]) + ((d * d) * NS) / N1;
  }
}

__global__ __launch_bounds__(256) void radiance_resolve_kernel(ResolveArgs a) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.npix) return;
  const double *f = a.frame + p * 6;
  const int64_t np = a.counts ? a.counts[p] : a.n;
  const double n = (double)np, n1 = (double)(np - 1);
  for (int c = 0; c < 3; c++) {
    if (a.mean) a.mean[3 * p + c] = (float)f[c];
    if (a.variance) a.variance[3 * p + c] = np < 2 ? 0.0f : (float)(f[3 + c] / n1 / n);
  }
}

// e_p: relative standard error of luminance of accumulator record f under np >= 2 samples
__device__ __forceinline__ double pixel_error(const double *f, int64_t np) {
  const double n = (double)np, n1 = (double)(np - 1);
  const double Y = 0.2126 * f[0] + 0.7152 * f[1] + 0.0722 * f[2];
  const double v = (0.2126 * 0.2126) * (f[3] / n1 / n) + (0.7152 * 0.7152) * (f[4] / n1 / n) +
                   (0.0722 * 0.0722) * (f[5] / n1 / n);
  return sqrt(v) / (Y + 0.01);
}

__global__ __launch_bounds__(NOISE_BLOCK) void accum_noise_kernel(NoiseArgs a) {
  __shared__ double x[NOISE_BLOCK];
  const int t = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * NOISE_BLOCK + t;
  double e = 0.0;
  if (p < a.npix) {
    const int64_t np = a.counts[p];
    if (np >= 2) e = pixel_error(a.acc + p * 6, np);
  }
  x[t] = e;
  __syncthreads();
  for (int h = NOISE_BLOCK / 2; h >= 1; h >>= 1) {
    if (t < h) x[t] += x[t + h];
    __syncthreads();
  }
  if (t == 0) a.partial[blockIdx.x] = x[0];
}

__global__ __launch_bounds__(256) void count_stats_kernel(CountArgs a) {
  __shared__ int64_t mn[256], sm[256];
  const int t = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * 256 + t;
  mn[t] = p < a.npix ? a.counts[p] : INT64_MAX;
  sm[t] = p < a.npix ? a.counts[p] : 0;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (t < h) {
      mn[t] = mn[t + h] < mn[t] ? mn[t + h] : mn[t];
      sm[t] += sm[t + h];
    }
    __syncthreads();
  }
  if (t == 0) {
    a.partial[2 * blockIdx.x] = mn[0];
    a.partial[2 * blockIdx.x + 1] = sm[0];
  }
}

// One wave per tile. Consecutive lanes take consecutive slots, so they run along the tile's rows
// (at T = 8 a tile row is one 384-B run of accumulator records). The lane sums and the wave tree
// are in the order gi_radiance.h states: lane l's x[l + h] comes from lane l + h by a shuffle, and
// only the lanes l < h of a step are read afterwards (the others add a value nobody uses).
__global__ __launch_bounds__(64 * TILE_WAVES) void tile_error_kernel(TileArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * TILE_WAVES + (threadIdx.x >> 6);
  if (t >= (int64_t)a.tiles_x * a.tiles_y) return;  // the whole wave
  const int x0 = (int)(t % a.tiles_x) * a.T, y0 = (int)(t / a.tiles_x) * a.T;
  const int nx = min(a.T, a.width - x0), ny = min(a.T, a.height - y0);
  double x = 0.0;
  int64_t nmin = INT64_MAX;
  for (int q = lane; q < a.T * a.T; q += 64) {
    const int yy = q / a.T, xx = q - yy * a.T;
    double e = 0.0;
    if (xx < nx && yy < ny) {
      const int64_t p = (int64_t)(y0 + yy) * a.width + (x0 + xx);
      const int64_t np = a.counts[p];
      nmin = np < nmin ? np : nmin;
      if (np >= 2) e = pixel_error(a.acc + p * 6, np);
    }
    x += e;
  }
  for (int h = 32; h >= 1; h >>= 1) {
    x += __shfl_down(x, h, 64);
    const int64_t o = __shfl_down((long long)nmin, h, 64);
    nmin = o < nmin ? o : nmin;
  }
  if (lane == 0) {
    a.tile_error[t] = x / (double)(nx * ny);
    a.tile_nmin[t] = nmin;
  }
}

__global__ __launch_bounds__(256) void tile_select_kernel(SelectArgs a) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)a.tiles_x * a.tiles_y) return;
  const int tx = (int)(t % a.tiles_x), ty = (int)(t / a.tiles_x);
  const bool below_max = a.max_samples == 0 || a.tile_nmin[t] < a.max_samples;
  bool active = a.tile_nmin[t] < a.min_samples || (a.tile_error[t] > a.threshold && below_max);
  if (!active && a.dilate && below_max) {
    for (int dy = -1; dy <= 1; dy++)
      for (int dx = -1; dx <= 1; dx++) {
        const int ux = tx + dx, uy = ty + dy;
        if ((dx == 0 && dy == 0) || ux < 0 || uy < 0 || ux >= a.tiles_x || uy >= a.tiles_y) continue;
        const int64_t u = (int64_t)uy * a.tiles_x + ux;
        if (a.tile_error[u] > a.threshold && (a.max_samples == 0 || a.tile_nmin[u] < a.max_samples))
          active = true;
      }
  }
  a.mask[t] = active ? 1 : 0;
}

// The history of pixel (x, y) of the current frame, gi.h "reprojection across views" step by step.
// A gather: the four taps of neighbouring lanes are neighbouring records of the old accumulator
// (48 B each) and of the old planes (32 B each), so a wave reads a few contiguous runs; the old
// buffers are only read, the new ones only written. The fp64 divisions are IEEE ones (the
// restatement must see the same bits), which is what the kernel's time goes to beside its bytes.
__global__ __launch_bounds__(REPROJECT_BX * REPROJECT_BY) void accum_reproject_kernel(ReprojectArgs a) {
  const int bx = (a.W + REPROJECT_BX - 1) / REPROJECT_BX;  // blocks per row of blocks
  const int x = (int)(blockIdx.x % bx) * REPROJECT_BX + threadIdx.x;
  const int y = (int)(blockIdx.x / bx) * REPROJECT_BY + threadIdx.y;
  const bool inside = x < a.W && y < a.H;
  double o[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int64_t nn = 0;
  if (inside) {
    const int64_t p = (int64_t)y * a.W + x;
    const float4 f0 = a.cur[2 * p], f1 = a.cur[2 * p + 1];
    const double W = (double)a.W, H = (double)a.H;
    double hs = 0.0, sm[3] = {0.0, 0.0, 0.0}, sv[3] = {0.0, 0.0, 0.0};
    int64_t nmin = INT64_MAX;
    if (f1.w != 0.0f) {
      const double dx = (double)(2 * x + 1 - a.W) / W;
      const double dy = (double)(2 * y + 1 - a.H) / H;
      double D[3], v[3];
      for (int k = 0; k < 3; k++) D[k] = ((a.org1[k] + a.right1[k] * dx) + a.up1[k] * dy) - a.eye1[k];
      const double l = sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
      const double z = (double)f0.w;
      for (int k = 0; k < 3; k++) {
        const double d = l == 0.0 ? D[k] : D[k] / l;  // normalize (gi_device.h)
        v[k] = (a.eye1[k] + d * z) - a.eye0[k];
      }
      const double al = ((v[0] * a.G[0] + v[1] * a.G[1]) + v[2] * a.G[2]) / a.GG;
      if (al > 0.0) {
        const double sx = (((v[0] * a.right0[0] + v[1] * a.right0[1]) + v[2] * a.right0[2]) / a.RR) / al;
        const double sy = (((v[0] * a.up0[0] + v[1] * a.up0[1]) + v[2] * a.up0[2]) / a.UU) / al;
        const double u = ((sx + 1.0) * W) * 0.5 - 0.5, t = ((sy + 1.0) * H) * 0.5 - 0.5;
        const double x0 = floor(u), y0 = floor(t);
        const double fx = u - x0, fy = t - y0;
        const double r = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        const double n0 = (double)f0.x, n1 = (double)f0.y, n2 = (double)f0.z;
        const double npp = (n0 * n0 + n1 * n1) + n2 * n2;
        const double a0 = (double)f1.x, a1 = (double)f1.y, a2 = (double)f1.z;
        for (int j = 0; j < 2; j++)
          for (int i = 0; i < 2; i++) {
            const double tx = x0 + (double)i, ty = y0 + (double)j;
            // in doubles: a projection far outside the frame (or a NaN) never becomes an index
            if (!(tx >= 0.0 && tx <= W - 1.0 && ty >= 0.0 && ty <= H - 1.0)) continue;
            const double h = (i ? fx : 1.0 - fx) * (j ? fy : 1.0 - fy);
            if (!(h >= 0.0009765625)) continue;  // 2^-10
            const int64_t q = (int64_t)ty * a.W + (int64_t)tx;
            const int64_t nq = a.counts[q];
            if (nq < 2) continue;
            const float4 g0 = a.prev[2 * q], g1 = a.prev[2 * q + 1];
            if (!(g1.w > 0.0f)) continue;
            if (!(fabs(r - (double)g0.w) <= a.depth_tol * r)) continue;
            const double m0 = (double)g0.x, m1 = (double)g0.y, m2 = (double)g0.z;
            const double c = (n0 * m0 + n1 * m1) + n2 * m2;
            const double nqq = (m0 * m0 + m1 * m1) + m2 * m2;
            if (!(c > 0.0 && c * c >= ((a.nmin2 * npp) * nqq))) continue;
            const double e0 = a0 - (double)g1.x, e1 = a1 - (double)g1.y, e2 = a2 - (double)g1.z;
            if (!((e0 * e0 + e1 * e1) + e2 * e2 <= a.atol2)) continue;
            const double *g = a.acc + q * 6;
            const double q1 = (double)(nq - 1);
            hs += h;
            for (int k = 0; k < 3; k++) {
              sm[k] += h * g[k];
              sv[k] += h * (g[3 + k] / q1);
            }
            nmin = nq < nmin ? nq : nmin;
          }
      }
    }
    if (nmin != INT64_MAX) {
      nn = nmin < a.max_history ? nmin : a.max_history;
      const double n1 = (double)(nn - 1);
      for (int k = 0; k < 3; k++) {
        o[k] = sm[k] / hs;
        o[3 + k] = (sv[k] / hs) * n1;
      }
    }
    double *g = a.acc_out + p * 6;
    for (int k = 0; k < 6; k++) g[k] = o[k];
    a.counts_out[p] = nn;
  }
  // per wave: a lane outside the frame adds nothing
  const int kept = __popcll(__ballot(nn > 0));
  long long s = nn;
  for (int h = 32; h >= 1; h >>= 1) s += __shfl_down(s, h, 64);
  if (threadIdx.x == 0) {
    const int64_t wv = (int64_t)blockIdx.x * REPROJECT_BY + threadIdx.y;
    a.partial[2 * wv] = kept;
    a.partial[2 * wv + 1] = s;
  }
}

// The records of pixels [p0, p0 + np) of a {mu, A} plane, read as one contiguous run (lane i takes
// double i of the run, then i + FOLD_BLOCK, ...: 512 B per wave instruction, where a thread that
// read its own 48-B record would touch 3 KiB per instruction) and handed to their threads through
// LDS. Every thread of the block calls it.
__device__ __forceinline__ void fold_stage(const double *plane, int64_t p0, int np, double *x,
                                           double *r) {
  const int t = threadIdx.x;
  const double *run = plane + p0 * 6;
  __syncthreads();  // x's readers of the stage before are done
  for (int i = t; i < np * 6; i += FOLD_BLOCK) x[i] = run[i];
  __syncthreads();
  if (t < np)
    for (int c = 0; c < 6; c++) r[c] = x[t * 6 + c];
}

// gi.h "accumulator state": the fold of b into a per pixel, in accum_merge_kernel's operation order
// with (S, m, M2) = (n_b, mu_b, A_b); an empty b leaves a as it is, an empty a takes b as it is.
__global__ __launch_bounds__(FOLD_BLOCK) void accum_fold_states_kernel(FoldArgs a) {
  __shared__ double x[FOLD_BLOCK * 6];
  const int t = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * FOLD_BLOCK;
  const int64_t left = a.npix - p0;
  const int np = left < FOLD_BLOCK ? (int)left : FOLD_BLOCK;
  const bool live = t < np;
  double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, f[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  fold_stage(a.acc, p0, np, x, g);
  int64_t n = live ? a.counts[p0 + t] : 0;
  for (int s = 0; s < a.nstates; s++) {
    const uint8_t *state = a.states + (int64_t)s * a.stride_bytes;
    fold_stage(reinterpret_cast<const double *>(state), p0, np, x, f);
    const int64_t nb = live ? reinterpret_cast<const int64_t *>(state + a.npix * 48)[p0 + t] : 0;
    if (nb != 0 && n == 0) {
      for (int c = 0; c < 6; c++) g[c] = f[c];
      n = nb;
    } else if (nb != 0) {
      const double Nb = (double)nb, N1 = (double)(n + nb), NS = (double)n * Nb;
      for (int c = 0; c < 3; c++) {
        const double d = f[c] - g[c];
        g[c] = g[c] + (d * Nb) / N1;
        g[3 + c] = (g[3 + c] + f[3 + c]) + ((d * d) * NS) / N1;
      }
      n = n + nb;
    }
  }
  __syncthreads();
  if (live) {
    for (int c = 0; c < 6; c++) x[t * 6 + c] = g[c];
    a.counts[p0 + t] = n;
  }
  __syncthreads();
  double *run = a.acc + p0 * 6;
  for (int i = t; i < np * 6; i += FOLD_BLOCK) run[i] = x[i];
}

__global__ __launch_bounds__(256) void tonemap_kernel(TonemapArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.nval) return;
  const double x = a.exposure * (double)a.in[i];
  double y = x;
  if (a.white > 0.0) y = (x * (1.0 + x / (a.white * a.white))) / (1.0 + x);
  y = y < 0.0 ? 0.0 : (y > 1.0 ? 1.0 : y);
  a.out[i] = (float)y;
}

void launch_reduce_radiance(const RadianceArgs &a, hipStream_t st) {
  if (a.npix > 0) reduce_radiance_kernel<<<nblk(a.npix, 64), 64, 0, st>>>(a);
}
void launch_accum_merge(const AccumArgs &a, hipStream_t st) {
  if (a.npix > 0) accum_merge_kernel<<<nblk(a.npix, 256), 256, 0, st>>>(a);
}
void launch_radiance_resolve(const ResolveArgs &a, hipStream_t st) {
  if (a.npix > 0) radiance_resolve_kernel<<<nblk(a.npix, 256), 256, 0, st>>>(a);
}
void launch_accum_noise(const NoiseArgs &a, hipStream_t st) {
  if (a.npix > 0) accum_noise_kernel<<<nblk(a.npix, NOISE_BLOCK), NOISE_BLOCK, 0, st>>>(a);
}
void launch_count_stats(const CountArgs &a, hipStream_t st) {
  if (a.npix > 0) count_stats_kernel<<<nblk(a.npix, 256), 256, 0, st>>>(a);
}
void launch_tile_error(const TileArgs &a, hipStream_t st) {
  const int64_t nt = (int64_t)a.tiles_x * a.tiles_y;
  if (nt > 0) tile_error_kernel<<<nblk(nt, TILE_WAVES), 64 * TILE_WAVES, 0, st>>>(a);
}
void launch_tile_select(const SelectArgs &a, hipStream_t st) {
  const int64_t nt = (int64_t)a.tiles_x * a.tiles_y;
  if (nt > 0) tile_select_kernel<<<nblk(nt, 256), 256, 0, st>>>(a);
}
void launch_accum_reproject(const ReprojectArgs &a, hipStream_t st) {
  if (a.W <= 0 || a.H <= 0) return;
  const unsigned grid = (unsigned)(reproject_waves(a.W, a.H) / REPROJECT_BY);  // row-major blocks
  accum_reproject_kernel<<<grid, dim3(REPROJECT_BX, REPROJECT_BY), 0, st>>>(a);
}
void launch_accum_fold_states(const FoldArgs &a, hipStream_t st) {
  if (a.npix > 0 && a.nstates > 0)
    accum_fold_states_kernel<<<nblk(a.npix, FOLD_BLOCK), FOLD_BLOCK, 0, st>>>(a);
}
void launch_tonemap(const TonemapArgs &a, hipStream_t st) {
  if (a.nval > 0) tonemap_kernel<<<nblk(a.nval, 256), 256, 0, st>>>(a);
}

}  // namespace gi
