// gi_denoise.h -- argument blocks and launchers of the feature-plane and denoise kernels
// (gi_denoise.hip). Blocks of their own: RenderArgs keeps its size (gi_kernels.h RaySlice).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gi_device.h"
#include "gi_kernels.h"

namespace gi {

// per sample ray: what the pixel reduction sums (DESIGN.md "Feature planes")
struct FeatSample {
  double n[3];   // hit normal as scene_intersect returns it (not flipped)
  double d;      // |hit - org|
  int32_t mat;   // material of the hit
  int32_t hit;
};
static_assert(sizeof(FeatSample) == 40, "feature sample record is 40 bytes");

// feature_trace_kernel: one thread per sample ray; feature_reduce_kernel: one per pixel, its
// spp samples in order. planes: two float4 per pixel {normal, depth}, {albedo, coverage},
// byte-identical to gi_pixel_features (gi.h)
struct FeatureArgs {
  SceneView S;
  int64_t nsamp;            // npix * spp
  int64_t npix;
  int32_t spp;
  const gi_ray_dev *rays;   // [nsamp]
  FeatSample *samples;      // [nsamp]
  float4 *planes;           // [npix * 2]
};

// one a-trous level: dst = filtered src (float4 {r, g, b, unused} per pixel)
struct DenoiseArgs {
  int32_t W, H;
  int32_t step;             // 2^level
  int32_t npow;             // normal weight squared this many times
  double sc2;               // (sigma_color / 2^level)^2
  double sigma_depth;
  double sa2;               // sigma_albedo^2
  const float4 *src;
  const float4 *planes;     // [W * H * 2], as FeatureArgs::planes
  float4 *dst;
};

// one level of the variance-guided filter (gi.h gi_denoise_radiance): dst = filtered src, float4
// {r, g, b, v} per pixel, v the variance of the pixel's luminance
struct VDenoiseArgs {
  int32_t W, H;
  int32_t step;             // 2^level
  int32_t npow;             // normal weight squared this many times
  double sl2;               // sigma_lum^2
  double vfloor;            // variance_floor
  double sd2;               // sigma_depth^2
  double isa2;              // 1 / sigma_albedo^2
  const float4 *src;
  const float4 *planes;     // [W * H * 2], as FeatureArgs::planes
  float4 *dst;
};

void launch_vdenoise_level(const VDenoiseArgs &a, hipStream_t st);
// W*H*3 mean and W*H*3 channel variances (floats) -> float4 {r, g, b, v0} per pixel
void launch_vdenoise_pack(const float *mean, const float *var3, int64_t npix, float4 *img,
                          hipStream_t st);
// the same from the accumulator's {mu, A} (six doubles per pixel) and per-pixel counts
void launch_vdenoise_pack_accum(const double *acc, const int64_t *counts, int64_t npix, float4 *img,
                                hipStream_t st);
// float4 per pixel -> W*H*3 floats (rgbf) and W*H floats (vlum); either may be null
void launch_vdenoise_unpack(const float4 *img, int64_t npix, float *rgbf, float *vlum,
                            hipStream_t st);

void launch_feature_trace(const FeatureArgs &a, hipStream_t st);
void launch_feature_reduce(const FeatureArgs &a, hipStream_t st);
void launch_denoise_level(const DenoiseArgs &a, hipStream_t st);
// W*H*3 floats <-> float4 per pixel
void launch_denoise_pack(const float *rgbf, int64_t npix, float4 *img, hipStream_t st);
void launch_denoise_unpack(const float4 *img, int64_t npix, float *rgbf, hipStream_t st);

}  // namespace gi
