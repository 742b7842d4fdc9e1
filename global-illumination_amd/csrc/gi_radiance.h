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

// accum_merge_kernel: fold the pass frame {m, M2} of S samples into the accumulator {mu, A}, each
// pixel under its own count n_p (counts[p] += S). pixels == null: thread i folds pixel i of the
// frame; else thread i folds pixel pixels[i] (a masked pass's list) and the others stay as they are
struct AccumArgs {
  int64_t npix;             // pixels to fold: the frame's, or the list's
  int64_t S;
  const double *pass;       // [W * H * 6]
  double *acc;              // [W * H * 6]
  int64_t *counts;          // [W * H] samples each pixel holds
  const int2 *pixels;       // [npix] or null
  int32_t width;            // frame width (with a list)
};

// radiance_resolve_kernel: mean = (float)m, variance = (float)(M2 / (n - 1) / n), 0 when n < 2;
// n = counts[p] when counts is given (the accumulator), else the frame's n (one pass)
struct ResolveArgs {
  int64_t npix;
  int64_t n;
  const int64_t *counts;    // [npix] or null
  const double *frame;      // [npix * 6]
  float *mean, *variance;   // [npix * 3] each, either may be null
};

// accum_noise_kernel: relative standard error of luminance per pixel, summed per block of
// NOISE_BLOCK consecutive pixels by an LDS tree; one partial per block
constexpr int NOISE_BLOCK = 256;
struct NoiseArgs {
  int64_t npix;
  const int64_t *counts;    // [npix] samples per pixel (a pixel below 2 adds 0)
  const double *acc;        // [npix * 6]
  double *partial;          // [ceil(npix / NOISE_BLOCK)]
};

// count_stats_kernel: smallest count and sum of counts per block of 256 pixels (integers: any
// order gives the same result); partial = {min, sum} per block
struct CountArgs {
  int64_t npix;
  const int64_t *counts;    // [npix]
  int64_t *partial;         // [ceil(npix / 256) * 2]
};

// tile_error_kernel (adaptive passes): one wave per tile of T x T pixels, TILE_WAVES tiles per
// block. Slot q = y_in_tile * T + x_in_tile holds the pixel's error (accum_noise_kernel's e_p
// under its own count; 0 outside the image or below two samples); lane l sums the slots
// q = l, l + 64, ... in that order, then x[l] += x[l + h] for h = 32 .. 1; error = x[0] / pixels
// of the tile inside the image. nmin = the smallest count of those pixels.
constexpr int TILE_WAVES = 4;
struct TileArgs {
  int32_t width, height, T, tiles_x, tiles_y;
  const double *acc;        // [W * H * 6]
  const int64_t *counts;    // [W * H]
  double *tile_error;       // [tiles]
  int64_t *tile_nmin;       // [tiles]
};

// tile_select_kernel: one thread per tile, the selection of gi.h "adaptive passes"
struct SelectArgs {
  int32_t tiles_x, tiles_y, dilate;
  int64_t min_samples, max_samples;
  double threshold;
  const double *tile_error;
  const int64_t *tile_nmin;
  uint8_t *mask;            // [tiles] 1 = active
};

// accum_reproject_kernel (gi.h "reprojection across views"): one thread per pixel of the current
// frame, block 64 x 4 (a wave is 64 pixels of one row). The thread gathers its history from up to
// four pixels of the old accumulator and writes the new record and count; a pixel without history
// gets zeros. Wave v = block * 4 + threadIdx.y (blocks row-major over the frame) writes partial[2 v]
// = its pixels that kept history and partial[2 v + 1] = the sum of their new counts (integers:
// any order gives the same sums). The host precomputes what is the same for every pixel.
constexpr int REPROJECT_BX = 64, REPROJECT_BY = 4;
struct ReprojectArgs {
  int32_t W, H;
  int64_t max_history;
  double depth_tol;
  double nmin2;             // normal_min * normal_min
  double atol2;             // albedo_tol * albedo_tol
  double eye1[3], org1[3], right1[3], up1[3];  // the current view
  double eye0[3], right0[3], up0[3];           // the previous view
  double G[3];              // far_org0 - eye0
  double GG, RR, UU;        // G . G, far_right0 . far_right0, far_up0 . far_up0
  const double *acc;        // [W * H * 6] the old accumulator
  const int64_t *counts;    // [W * H]
  const float4 *prev;       // [W * H * 2] planes of the old frame: {normal, depth}, {albedo, coverage}
  const float4 *cur;        // [W * H * 2] planes of the current frame
  double *acc_out;          // [W * H * 6]
  int64_t *counts_out;      // [W * H]
  int64_t *partial;         // [waves * 2]
};
inline int64_t reproject_waves(int w, int h) {
  return (int64_t)((w + REPROJECT_BX - 1) / REPROJECT_BX) * ((h + REPROJECT_BY - 1) / REPROJECT_BY) *
         REPROJECT_BY;
}

// accum_fold_states_kernel (gi.h "accumulator state"): nstates packed states, state s at states +
// s * stride_bytes ({mu, A} plane of npix * 48 B, then the count plane of npix * 8 B), folded into
// the accumulator in the order s = 0 .. nstates - 1. One thread per pixel, FOLD_BLOCK consecutive
// pixels per block; the running value stays in registers, so the accumulator is read once and
// written once and each state is read once. stride_bytes is a multiple of 8.
constexpr int FOLD_BLOCK = 256;
struct FoldArgs {
  int64_t npix;
  int32_t nstates;
  int64_t stride_bytes;
  const uint8_t *states;    // [nstates * stride_bytes]
  double *acc;              // [npix * 6]
  int64_t *counts;          // [npix]
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
void launch_count_stats(const CountArgs &a, hipStream_t st);
void launch_tile_error(const TileArgs &a, hipStream_t st);
void launch_tile_select(const SelectArgs &a, hipStream_t st);
void launch_accum_reproject(const ReprojectArgs &a, hipStream_t st);
void launch_accum_fold_states(const FoldArgs &a, hipStream_t st);
void launch_tonemap(const TonemapArgs &a, hipStream_t st);

}  // namespace gi
