// gi_radiance.h -- argument blocks and launchers of the radiance-frame, accumulator and tone-map
// kernels (gi_radiance.hip). Blocks of their own: RenderArgs keeps its size.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gi {

// reduce_radiance_kernel: one thread per output pixel of a batch, beside reduce_kernel and on its
// inputs. frame: six doubles per pixel of the whole image, {m.rgb, M2.rgb}
struct RadianceArgs {
  const double *prim_rgb;   // [npix * S * dof_test * 3] of this batch (RenderArgs::prim_rgb)
  const int2 *pixels;       // [npix] output pixels of this batch (RenderArgs::pixels)
  int32_t npix;
  int32_t S;                // samples per pixel: af * af, or spp in ray mode
  int32_t dof_test;
  int32_t out_w;
  double bw;                // reduce_kernel's box weight: 1.0 / af / af, or 1.0 / spp
  double *frame;            // [W * H * 6]
  double *samples;          // [W * H * S * 3] or null
};

// accum_merge_kernel: fold the pass frame {m, M2} of S samples into the accumulator {mu, A} of N
struct AccumArgs {
  int64_t npix;
  int64_t N;                // samples the accumulator holds before this pass
  int64_t S;
  const double *pass;       // [npix * 6]
  double *acc;              // [npix * 6]
};

// radiance_resolve_kernel: mean = (float)m, variance = (float)(M2 / (n - 1) / n), 0 when n < 2
struct ResolveArgs {
  int64_t npix;
  int64_t n;
  const double *frame;      // [npix * 6]
  float *mean, *variance;   // [npix * 3] each, either may be null
};

// accum_noise_kernel: relative standard error of luminance per pixel, summed per block of
// NOISE_BLOCK consecutive pixels by an LDS tree; one partial per block
constexpr int NOISE_BLOCK = 256;
struct NoiseArgs {
  int64_t npix;
  int64_t n;
  const double *acc;        // [npix * 6]
  double *partial;          // [ceil(npix / NOISE_BLOCK)]
};

// tonemap_kernel: one thread per channel value
struct TonemapArgs {
  int64_t nval;             // W * H * 3
  double exposure, white;
  const float *in;
  float *out;
};

void launch_reduce_radiance(const RadianceArgs &a, hipStream_t st);
void launch_accum_merge(const AccumArgs &a, hipStream_t st);
void launch_radiance_resolve(const ResolveArgs &a, hipStream_t st);
void launch_accum_noise(const NoiseArgs &a, hipStream_t st);
void launch_tonemap(const TonemapArgs &a, hipStream_t st);

}  // namespace gi
