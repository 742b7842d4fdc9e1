// gi_frames.cpp -- what works on finished frames and has no counterpart in the reference:
// feature planes and the denoisers, radiance frames, the accumulator with its state calls, its
// adaptive passes and reprojection, tone mapping.
#include <cmath>
#include <functional>
#include <limits>
#include "gi_ctx.h"
#include "gi_denoise.h"
#include "gi_radiance.h"

extern "C" {

// ---- feature planes and denoise pass (gi_denoise.hip; no reference counterpart) ---------
// Planes of npix_total pixels of spp samples each, in chunks of whole pixels of at most 2^22
// samples (one pixel where spp is above that). fill(s0, n) leaves samples [s0, s0 + n) of the
// frame in c->s.d_rays.
static int feature_planes(gi_ctx *c, int64_t npix_total, int64_t spp, gi_pixel_features *out,
                          const std::function<int(int64_t, int64_t)> &fill) {
  static_assert(sizeof(gi_pixel_features) == 2 * sizeof(float4), "planes are two float4 per pixel");
  const int64_t chunk_px = std::min(npix_total, std::max<int64_t>(1, ((int64_t)1 << 22) / spp));
  HIPCHK(c, c->s.d_rays.ensure((size_t)(chunk_px * spp) * sizeof(gi_ray)));
  HIPCHK(c, c->s.feat_samples.ensure((size_t)(chunk_px * spp) * sizeof(FeatSample)));
  HIPCHK(c, c->s.feat_planes.ensure((size_t)chunk_px * sizeof(gi_pixel_features)));
  FeatureArgs a;
  memset(&a, 0, sizeof a);
  a.S = make_view(c);
  a.spp = (int32_t)spp;
  a.samples = c->s.feat_samples.as<FeatSample>();
  a.planes = c->s.feat_planes.as<float4>();
  for (int64_t p0 = 0; p0 < npix_total; p0 += chunk_px) {
    a.npix = std::min(chunk_px, npix_total - p0);
    a.nsamp = a.npix * spp;
    int rc = fill(p0 * spp, a.nsamp);
    if (rc) return rc;
    a.rays = c->s.d_rays.as<gi_ray_dev>();
    launch_feature_trace(a, c->stream);
    HIPCHK(c, hipGetLastError());
    launch_feature_reduce(a, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out + p0, c->s.feat_planes.p, (size_t)a.npix * sizeof(gi_pixel_features),
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return GI_OK;
}

int gi_camera_features(gi_ctx *c, int aa, int w, int h, gi_pixel_features *out) {
  if (!c) return GI_ERR_ARG;
  DeviceScope dev(c->device);
  int rc = check_ready(c);
  if (rc) return rc;
  if (!out) return fail(c, GI_ERR_ARG, "null feature buffer");
  if (aa < 0 || aa > 15 || w <= 0 || h <= 0) return fail(c, GI_ERR_ARG, "bad image size");
  const gi_params &P = c->P;
  const int af = 1 << aa, dof = std::max(1, P.dof_test);
  const int64_t spp = (int64_t)af * af * dof;
  if (spp >= ((int64_t)1 << 31)) return fail(c, GI_ERR_ARG, "4^aa * dof_test must be below 2^31");
  CameraRaysArgs ca;
  memset(&ca, 0, sizeof ca);
  ca.cam = make_view(c).cam;
  ca.seed = P.seed;
  ca.dof = P.depth_of_field;
  ca.dof_test = dof;
  ca.af = af;
  ca.W = w * af;
  ca.H = h * af;
  ca.out_w = w;
  // the frame's rays from camera_rays_kernel itself: the rays gi_camera_rays exports
  return feature_planes(c, (int64_t)w * h, spp, out, [&](int64_t s0, int64_t n) -> int {
    HIPCHK(c, c->s.d_ray_ids.ensure((size_t)n * 8));
    ca.rays = c->s.d_rays.as<gi_ray_dev>();
    ca.ids = c->s.d_ray_ids.as<uint64_t>();
    ca.first = s0;
    ca.n = n;
    launch_camera_rays(ca, c->stream);
    HIPCHK(c, hipGetLastError());
    return GI_OK;
  });
}

int gi_ray_features(gi_ctx *c, int w, int h, int spp, const gi_ray *rays, gi_pixel_features *out) {
  if (!c) return GI_ERR_ARG;
  DeviceScope dev(c->device);
  int rc = check_ready(c);
  if (rc) return rc;
  if (!rays) return fail(c, GI_ERR_ARG, "null ray buffer");
  if (!out) return fail(c, GI_ERR_ARG, "null feature buffer");
  if (spp < 1) return fail(c, GI_ERR_ARG, "spp must be at least 1");
  if (w <= 0 || h <= 0) return fail(c, GI_ERR_ARG, "bad image size");
  if ((int64_t)w * h >= ((int64_t)1 << 31) / spp + (((int64_t)1 << 31) % spp != 0))
    return fail(c, GI_ERR_ARG, "width * height * spp must be below 2^31");
  return feature_planes(c, (int64_t)w * h, spp, out, [&](int64_t s0, int64_t n) -> int {
    HIPCHK(c, hipMemcpyAsync(c->s.d_rays.p, rays + s0, (size_t)n * sizeof(gi_ray),
                             hipMemcpyHostToDevice, c->stream));
    return GI_OK;
  });
}

void gi_denoise_params_default(gi_denoise_params *p) {
  if (!p) return;
  p->levels = 5;
  p->normal_power_log2 = 5;
  p->sigma_color = 1.0;
  p->sigma_depth = 0.05;
  p->sigma_albedo = 0.1;
}

int gi_denoise(gi_ctx *c, int w, int h, const float *rgbf, const gi_pixel_features *feat,
               const gi_denoise_params *pp, float *out_rgbf, uint8_t *out_rgb8, double *kernel_ms) {
  if (!c) return GI_ERR_ARG;
  if (!rgbf || !feat || (!out_rgbf && !out_rgb8)) return fail(c, GI_ERR_ARG, "null image buffer");
  if (w <= 0 || h <= 0 || (int64_t)w * h >= ((int64_t)1 << 31))
    return fail(c, GI_ERR_ARG, "bad image size");
  gi_denoise_params P;
  gi_denoise_params_default(&P);
  if (pp) P = *pp;
  if (P.levels < 1 || P.levels > 8) return fail(c, GI_ERR_ARG, "denoise: levels outside 1..8");
  if (P.normal_power_log2 < 0 || P.normal_power_log2 > 8)
    return fail(c, GI_ERR_ARG, "denoise: normal_power_log2 outside 0..8");
  for (double s : {P.sigma_color, P.sigma_depth, P.sigma_albedo})
    if (!std::isfinite(s) || !(s > 0.0))
      return fail(c, GI_ERR_ARG, "denoise: sigmas must be finite and positive");
  DeviceScope dev(c->device);
  const size_t npix = (size_t)w * h;
  HIPCHK(c, upload(c->s.dn_rgbf, rgbf, npix * 12, c->stream));
  HIPCHK(c, upload(c->s.dn_planes, feat, npix * sizeof(gi_pixel_features), c->stream));
  HIPCHK(c, c->s.dn_img[0].ensure(npix * sizeof(float4)));
  HIPCHK(c, c->s.dn_img[1].ensure(npix * sizeof(float4)));
  launch_denoise_pack(c->s.dn_rgbf.as<float>(), (int64_t)npix, c->s.dn_img[0].as<float4>(), c->stream);
  HIPCHK(c, hipGetLastError());
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (kernel_ms) {
    HIPCHK(c, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) {
      hipEventDestroy(e0);
      return fail(c, GI_ERR_HIP, "denoise: hipEventCreate failed");
    }
    (void)hipEventRecord(e0, c->stream);
  }
  DenoiseArgs a;
  memset(&a, 0, sizeof a);
  a.W = w;
  a.H = h;
  a.npow = P.normal_power_log2;
  a.sigma_depth = P.sigma_depth;
  a.sa2 = P.sigma_albedo * P.sigma_albedo;
  a.planes = c->s.dn_planes.as<float4>();
  int cur = 0;
  hipError_t le = hipSuccess;
  for (int l = 0; l < P.levels && le == hipSuccess; l++) {
    const double sc = P.sigma_color / (double)(1 << l);
    a.step = 1 << l;
    a.sc2 = sc * sc;
    a.src = c->s.dn_img[cur].as<float4>();
    a.dst = c->s.dn_img[cur ^ 1].as<float4>();
    launch_denoise_level(a, c->stream);
    le = hipGetLastError();
    cur ^= 1;
  }
  if (kernel_ms) (void)hipEventRecord(e1, c->stream);
  if (le == hipSuccess) {
    launch_denoise_unpack(c->s.dn_img[cur].as<float4>(), (int64_t)npix, c->s.dn_rgbf.as<float>(), c->stream);
    le = hipGetLastError();
  }
  std::vector<float> stage;
  float *dst = out_rgbf;
  if (!dst) {
    stage.resize(npix * 3);
    dst = stage.data();
  }
  if (le == hipSuccess)
    le = hipMemcpyAsync(dst, c->s.dn_rgbf.p, npix * 12, hipMemcpyDeviceToHost, c->stream);
  if (le == hipSuccess) le = hipStreamSynchronize(c->stream);
  if (kernel_ms) {
    float ms = 0.f;
    if (le == hipSuccess) le = hipEventElapsedTime(&ms, e0, e1);
    *kernel_ms = ms;
    hipEventDestroy(e0);
    hipEventDestroy(e1);
  }
  HIPCHK(c, le);
  if (out_rgb8) return gi_quantize(w, h, dst, out_rgb8);
  return GI_OK;
}

// ---- radiance frames, accumulator and tone map (gi_radiance.hip; no reference counterpart) ----
// One render with the radiance reduction on: c->s.rad_frame then holds the finished pass {m, M2}
// (written once per pixel by the render that completed: a re-render after ST_GEN_MISS overwrites
// every pixel, a batch re-run under the slot guard never reached its reduction).
// pix (camera passes only): render these output pixels instead of the whole frame; rad_frame keeps
// what it held at the others.
// layers (whole frames only): the light-path layers' {m, M2} planes into c->s.lay_frame as well
// (and their samples into c->s.lay_samples), under rad_frame's contract.
static int radiance_pass(gi_ctx *c, int aa, int w, int h, bool want_samples, gi_render_stats *st,
                         const RaySrc *rsrc, int64_t *S_out,
                         const std::vector<int32_t> *pix = nullptr, bool layers = false) {
  hipSetDevice(c->device);
  int rc = check_ready(c);
  if (rc) return rc;
  if (aa < 0 || aa > 15 || w <= 0 || h <= 0) return fail(c, GI_ERR_ARG, "bad image size");
  const int64_t S = rsrc ? (int64_t)rsrc->spp : (int64_t)1 << (2 * aa);
  const size_t npix = (size_t)w * h;
  if ((int64_t)npix >= ((int64_t)1 << 31) / S + (((int64_t)1 << 31) % S != 0))
    return fail(c, GI_ERR_ARG, "width * height * samples per pixel must be below 2^31");
  HIPCHK(c, c->s.rad_frame.ensure(npix * 48));
  if (want_samples) HIPCHK(c, c->s.rad_samples.ensure(npix * (size_t)S * 24));
  if (layers) {
    HIPCHK(c, c->s.lay_frame.ensure(GI_LAYER_COUNT * npix * 48));
    if (want_samples) HIPCHK(c, c->s.lay_samples.ensure(GI_LAYER_COUNT * npix * (size_t)S * 24));
    c->lay_npix = npix;
  }
  c->rad_want_samples = want_samples;
  c->lay_on = layers;
  c->rad_on = true;
  rc = pix ? render_common(c, aa, w, h, *pix, nullptr, nullptr, st, false)
           : render_frame(c, aa, w, h, nullptr, nullptr, st, rsrc);
  c->rad_on = false;
  c->lay_on = false;
  *S_out = S;
  return rc;
}

// {m, M2} of n samples per pixel (counts: of counts[p], the accumulator's) -> host float mean /
// variance of the mean (either may be null)
static int radiance_resolve(gi_ctx *c, const double *frame, size_t npix, int64_t n, float *mean,
                            float *variance, const int64_t *counts = nullptr) {
  if (!mean && !variance) return GI_OK;
  HIPCHK(c, c->s.rad_mean.ensure(npix * 12));
  HIPCHK(c, c->s.rad_var.ensure(npix * 12));
  ResolveArgs a;
  memset(&a, 0, sizeof a);
  a.npix = (int64_t)npix;
  a.n = n;
  a.counts = counts;
  a.frame = frame;
  a.mean = mean ? c->s.rad_mean.as<float>() : nullptr;
  a.variance = variance ? c->s.rad_var.as<float>() : nullptr;
  launch_radiance_resolve(a, c->stream);
  HIPCHK(c, hipGetLastError());
  if (mean) HIPCHK(c, hipMemcpyAsync(mean, c->s.rad_mean.p, npix * 12, hipMemcpyDeviceToHost, c->stream));
  if (variance)
    HIPCHK(c, hipMemcpyAsync(variance, c->s.rad_var.p, npix * 12, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GI_OK;
}

// layers: the outputs hold GI_LAYER_COUNT + 1 planes, the layers' and then the frame's own
static int render_radiance(gi_ctx *c, int aa, int w, int h, const RaySrc *rsrc, float *mean,
                           float *variance, double *samples, gi_render_stats *st,
                           bool layers = false) {
  if (!c->peers.empty())
    return fail(c, GI_ERR_UNSUPPORTED, "radiance frames are for one-device contexts");
  if (!mean && !variance && !samples) return fail(c, GI_ERR_ARG, "null image buffer");
  int64_t S = 0;
  int rc = radiance_pass(c, aa, w, h, samples != nullptr, st, rsrc, &S, nullptr, layers);
  if (rc) return rc;
  const size_t npix = (size_t)w * h;
  const size_t nsmp = npix * (size_t)S * 3;  // doubles of one plane of samples
  const int total = layers ? GI_LAYER_TOTAL : 0;
  if (samples) {
    if (layers)
      HIPCHK(c, hipMemcpyAsync(samples, c->s.lay_samples.p, GI_LAYER_COUNT * nsmp * 8,
                               hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(samples + total * nsmp, c->s.rad_samples.p, nsmp * 8, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  for (int l = 0; l < total; l++) {
    rc = radiance_resolve(c, c->s.lay_frame.as<double>() + l * npix * 6, npix, S,
                          mean ? mean + l * npix * 3 : nullptr, variance ? variance + l * npix * 3 : nullptr);
    if (rc) return rc;
  }
  return radiance_resolve(c, c->s.rad_frame.as<double>(), npix, S, mean ? mean + total * npix * 3 : nullptr,
                          variance ? variance + total * npix * 3 : nullptr);
}

// gi_render_rays' argument checks
static int check_ray_args(gi_ctx *c, int w, int h, int spp, const gi_ray *rays) {
  if (!rays) return fail(c, GI_ERR_ARG, "null ray buffer");
  if (spp < 1) return fail(c, GI_ERR_ARG, "spp must be at least 1");
  if (w <= 0 || h <= 0) return fail(c, GI_ERR_ARG, "bad image size");
  if ((int64_t)w * h >= ((int64_t)1 << 31) / spp + (((int64_t)1 << 31) % spp != 0))
    return fail(c, GI_ERR_ARG, "width * height * spp must be below 2^31");
  return GI_OK;
}

int gi_render_radiance(gi_ctx *c, int aa, int w, int h, float *mean, float *variance,
                       double *samples, gi_render_stats *st) {
  if (!c) return GI_ERR_ARG;
  return render_radiance(c, aa, w, h, nullptr, mean, variance, samples, st);
}

int gi_render_rays_radiance(gi_ctx *c, int w, int h, int spp, const gi_ray *rays,
                            const uint64_t *ids, float *mean, float *variance, double *samples,
                            gi_render_stats *st) {
  if (!c) return GI_ERR_ARG;
  if (!c->peers.empty())
    return fail(c, GI_ERR_UNSUPPORTED, "radiance frames are for one-device contexts");
  int rc = check_ray_args(c, w, h, spp, rays);
  if (rc) return rc;
  const RaySrc src{rays, ids, spp};
  return render_radiance(c, 0, w, h, &src, mean, variance, samples, st);
}

int gi_render_layers(gi_ctx *c, int aa, int w, int h, float *mean, float *variance, double *samples,
                     gi_render_stats *st) {
  if (!c) return GI_ERR_ARG;
  return render_radiance(c, aa, w, h, nullptr, mean, variance, samples, st, true);
}

int gi_render_rays_layers(gi_ctx *c, int w, int h, int spp, const gi_ray *rays, const uint64_t *ids,
                          float *mean, float *variance, double *samples, gi_render_stats *st) {
  if (!c) return GI_ERR_ARG;
  if (!c->peers.empty())
    return fail(c, GI_ERR_UNSUPPORTED, "radiance frames are for one-device contexts");
  int rc = check_ray_args(c, w, h, spp, rays);
  if (rc) return rc;
  const RaySrc src{rays, ids, spp};
  return render_radiance(c, 0, w, h, &src, mean, variance, samples, st, true);
}

int gi_layers_timing(gi_ctx *c, int on, double *ms) {
  if (!c) return GI_ERR_ARG;
  if (ms) *ms = c->lay_ms;
  c->lay_time = on != 0;
  if (on) c->lay_ms = 0.0;
  return GI_OK;
}

int gi_accum_reset(gi_ctx *c, int w, int h) {
  if (!c) return GI_ERR_ARG;
  if (!c->peers.empty())
    return fail(c, GI_ERR_UNSUPPORTED, "the accumulator is for one-device contexts");
  if (w <= 0 || h <= 0 || (int64_t)w * h >= ((int64_t)1 << 31))
    return fail(c, GI_ERR_ARG, "bad image size");
  DeviceScope dev(c->device);
  c->acc_valid = false;
  const size_t npix = (size_t)w * h;
  HIPCHK(c, c->res.acc.ensure(npix * 48));
  HIPCHK(c, c->res.acc_cnt.ensure(npix * 8));
  if (c->res.acc2.p) {  // the reprojection's second buffer follows the accumulator's size
    HIPCHK(c, c->res.acc2.ensure(npix * 48));
    HIPCHK(c, c->res.acc2_cnt.ensure(npix * 8));
  }
  HIPCHK(c, hipMemsetAsync(c->res.acc.p, 0, npix * 48, c->stream));
  HIPCHK(c, hipMemsetAsync(c->res.acc_cnt.p, 0, npix * 8, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->acc_w = w;
  c->acc_h = h;
  c->acc_n = 0;
  c->acc_uniform = true;
  c->acc_valid = true;
  return GI_OK;
}

static int check_accum(gi_ctx *c) {
  if (!c->peers.empty())
    return fail(c, GI_ERR_UNSUPPORTED, "the accumulator is for one-device contexts");
  if (!c->acc_valid) return fail(c, GI_ERR_STATE, "no accumulator (gi_accum_reset)");
  return GI_OK;
}

// the layer contexts of a layered pass (gi.h): checked before anything is rendered
static int check_layer_ctxs(gi_ctx *c, gi_ctx *const *layers) {
  if (!layers) return fail(c, GI_ERR_ARG, "layers: null context list");
  for (int l = 0; l < GI_LAYER_COUNT; l++) {
    gi_ctx *L = layers[l];
    if (!L) continue;
    if (L == c) return fail(c, GI_ERR_ARG, "layers: a layer context is the rendering context");
    for (int m = 0; m < l; m++)
      if (layers[m] == L) return fail(c, GI_ERR_ARG, "layers: a layer context is listed twice");
    if (!L->peers.empty() || L->device != c->device)
      return fail(c, GI_ERR_ARG, "layers: a layer context is a one-device context on the same device");
    if (!L->acc_valid) return fail(c, GI_ERR_STATE, "a layer context has no accumulator (gi_accum_reset)");
    if (L->acc_w != c->acc_w || L->acc_h != c->acc_h)
      return fail(c, GI_ERR_ARG, "layers: a layer context's accumulator is not the accumulator's size");
  }
  return GI_OK;
}

// one finished pass (c->s.rad_frame, S samples per pixel) into the accumulator; layers (optional):
// its layer planes (c->s.lay_frame) by the same update into those contexts' accumulators, which
// live on this device (every accumulator call ends synchronised, so this stream may write them)
static int accum_pass(gi_ctx *c, int aa, const RaySrc *rsrc, gi_render_stats *st,
                      gi_ctx *const *layers = nullptr) {
  int rc = check_accum(c);
  if (rc) return rc;
  int64_t S = 0;
  rc = radiance_pass(c, aa, c->acc_w, c->acc_h, false, st, rsrc, &S, nullptr, layers != nullptr);
  if (rc) return rc;
  AccumArgs a;
  memset(&a, 0, sizeof a);
  a.npix = (int64_t)c->acc_w * c->acc_h;
  a.S = S;
  a.pass = c->s.rad_frame.as<double>();
  a.acc = c->res.acc.as<double>();
  a.counts = c->res.acc_cnt.as<int64_t>();
  launch_accum_merge(a, c->stream);
  HIPCHK(c, hipGetLastError());
  for (int l = 0; layers && l < GI_LAYER_COUNT; l++) {
    gi_ctx *L = layers[l];
    if (!L) continue;
    a.pass = c->s.lay_frame.as<double>() + (size_t)l * a.npix * 6;
    a.acc = L->res.acc.as<double>();
    a.counts = L->res.acc_cnt.as<int64_t>();
    launch_accum_merge(a, c->stream);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->acc_n += S;  // every pixel's count while acc_uniform, else unused
  for (int l = 0; layers && l < GI_LAYER_COUNT; l++)
    if (layers[l]) layers[l]->acc_n += S;
  return GI_OK;
}

int gi_accum_add_image(gi_ctx *c, int aa, gi_render_stats *st) {
  if (!c) return GI_ERR_ARG;
  return accum_pass(c, aa, nullptr, st);
}

int gi_accum_add_rays(gi_ctx *c, int spp, const gi_ray *rays, const uint64_t *ids,
                      gi_render_stats *st) {
  if (!c) return GI_ERR_ARG;
  int rc = check_accum(c);
  if (!rc) rc = check_ray_args(c, c->acc_w, c->acc_h, spp, rays);
  if (rc) return rc;
  const RaySrc src{rays, ids, spp};
  return accum_pass(c, 0, &src, st);
}

int gi_accum_add_image_layers(gi_ctx *c, int aa, gi_ctx *const layers[GI_LAYER_COUNT],
                              gi_render_stats *st) {
  if (!c) return GI_ERR_ARG;
  int rc = check_accum(c);
  if (!rc) rc = check_layer_ctxs(c, layers);
  if (rc) return rc;
  return accum_pass(c, aa, nullptr, st, layers);
}

int gi_accum_add_rays_layers(gi_ctx *c, int spp, const gi_ray *rays, const uint64_t *ids,
                             gi_ctx *const layers[GI_LAYER_COUNT], gi_render_stats *st) {
  if (!c) return GI_ERR_ARG;
  int rc = check_accum(c);
  if (!rc) rc = check_layer_ctxs(c, layers);
  if (!rc) rc = check_ray_args(c, c->acc_w, c->acc_h, spp, rays);
  if (rc) return rc;
  const RaySrc src{rays, ids, spp};
  return accum_pass(c, 0, &src, st, layers);
}

// smallest and summed per-pixel sample count of the accumulator (either output optional)
static int count_stats(gi_ctx *c, int64_t *smallest, int64_t *total) {
  const size_t npix = (size_t)c->acc_w * c->acc_h;
  const size_t nb = (npix + 255) / 256;
  HIPCHK(c, c->s.acc_part.ensure(nb * 16));
  CountArgs a;
  memset(&a, 0, sizeof a);
  a.npix = (int64_t)npix;
  a.counts = c->res.acc_cnt.as<int64_t>();
  a.partial = c->s.acc_part.as<int64_t>();
  launch_count_stats(a, c->stream);
  HIPCHK(c, hipGetLastError());
  std::vector<int64_t> part(nb * 2);
  HIPCHK(c, hipMemcpyAsync(part.data(), c->s.acc_part.p, nb * 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int64_t mn = part[0], sum = 0;
  for (size_t b = 0; b < nb; b++) {
    mn = std::min(mn, part[2 * b]);
    sum += part[2 * b + 1];
  }
  if (smallest) *smallest = mn;
  if (total) *total = sum;
  return GI_OK;
}

int gi_accum_get_counts(gi_ctx *c, int64_t *counts, int64_t *total) {
  if (!c) return GI_ERR_ARG;
  if (int rc = check_accum(c)) return rc;
  DeviceScope dev(c->device);
  const size_t npix = (size_t)c->acc_w * c->acc_h;
  if (counts) {
    HIPCHK(c, hipMemcpyAsync(counts, c->res.acc_cnt.p, npix * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (total) return count_stats(c, nullptr, total);
  return GI_OK;
}

// ---- accumulator state (gi.h "accumulator state"; accum_fold_states_kernel) -----------------
static bool any_negative(const int64_t *counts, size_t npix) {
  for (size_t p = 0; p < npix; p++)
    if (counts[p] < 0) return true;
  return false;
}

// nstates packed states in device memory of c's device folded into the accumulator, in order
static int fold_states(gi_ctx *c, int nstates, const void *packed, int64_t stride, double *kernel_ms) {
  FoldArgs a;
  memset(&a, 0, sizeof a);
  a.npix = (int64_t)c->acc_w * c->acc_h;
  a.nstates = nstates;
  a.stride_bytes = stride;
  a.states = (const uint8_t *)packed;
  a.acc = c->res.acc.as<double>();
  a.counts = c->res.acc_cnt.as<int64_t>();
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (kernel_ms) {
    HIPCHK(c, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) {
      hipEventDestroy(e0);
      return fail(c, GI_ERR_HIP, "accumulator merge: hipEventCreate failed");
    }
    (void)hipEventRecord(e0, c->stream);
  }
  launch_accum_fold_states(a, c->stream);
  hipError_t le = hipGetLastError();
  if (kernel_ms) (void)hipEventRecord(e1, c->stream);
  if (le == hipSuccess) le = hipStreamSynchronize(c->stream);
  if (kernel_ms) {
    float ms = 0.f;
    if (le == hipSuccess) le = hipEventElapsedTime(&ms, e0, e1);
    *kernel_ms = ms;
    hipEventDestroy(e0);
    hipEventDestroy(e1);
  }
  HIPCHK(c, le);
  c->acc_uniform = false;  // every pixel under its own count from here on
  return GI_OK;
}

int gi_accum_export(gi_ctx *c, double *state, int64_t *counts) {
  if (!c) return GI_ERR_ARG;
  if (int rc = check_accum(c)) return rc;
  if (!state && !counts) return fail(c, GI_ERR_ARG, "null state buffers");
  DeviceScope dev(c->device);
  const size_t npix = (size_t)c->acc_w * c->acc_h;
  if (state) HIPCHK(c, hipMemcpyAsync(state, c->res.acc.p, npix * 48, hipMemcpyDeviceToHost, c->stream));
  if (counts)
    HIPCHK(c, hipMemcpyAsync(counts, c->res.acc_cnt.p, npix * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GI_OK;
}

int gi_accum_import(gi_ctx *c, int w, int h, const double *state, const int64_t *counts) {
  if (!c) return GI_ERR_ARG;
  if (!c->peers.empty())
    return fail(c, GI_ERR_UNSUPPORTED, "the accumulator is for one-device contexts");
  if (w <= 0 || h <= 0 || (int64_t)w * h >= ((int64_t)1 << 31))
    return fail(c, GI_ERR_ARG, "bad image size");
  if (!state || !counts) return fail(c, GI_ERR_ARG, "null state buffers");
  const size_t npix = (size_t)w * h;
  if (any_negative(counts, npix)) return fail(c, GI_ERR_ARG, "accumulator state: negative sample count");
  DeviceScope dev(c->device);
  c->acc_valid = false;
  HIPCHK(c, c->res.acc.ensure(npix * 48));
  HIPCHK(c, c->res.acc_cnt.ensure(npix * 8));
  if (c->res.acc2.p) {  // as gi_accum_reset
    HIPCHK(c, c->res.acc2.ensure(npix * 48));
    HIPCHK(c, c->res.acc2_cnt.ensure(npix * 8));
  }
  HIPCHK(c, hipMemcpyAsync(c->res.acc.p, state, npix * 48, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->res.acc_cnt.p, counts, npix * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->acc_w = w;
  c->acc_h = h;
  c->acc_n = 0;
  c->acc_uniform = false;  // every pixel under its own count
  c->acc_valid = true;
  return GI_OK;
}

int gi_accum_merge(gi_ctx *c, int w, int h, const double *state, const int64_t *counts) {
  if (!c) return GI_ERR_ARG;
  if (int rc = check_accum(c)) return rc;
  if (w != c->acc_w || h != c->acc_h)
    return fail(c, GI_ERR_ARG, "accumulator state: not the accumulator's size");
  if (!state || !counts) return fail(c, GI_ERR_ARG, "null state buffers");
  const size_t npix = (size_t)w * h;
  if (any_negative(counts, npix)) return fail(c, GI_ERR_ARG, "accumulator state: negative sample count");
  DeviceScope dev(c->device);
  DBuf packed;
  HIPCHK(c, packed.ensure(npix * 56));
  HIPCHK(c, hipMemcpyAsync(packed.p, state, npix * 48, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(packed.as<uint8_t>() + npix * 48, counts, npix * 8, hipMemcpyHostToDevice,
                           c->stream));
  return fold_states(c, 1, packed.p, (int64_t)npix * 56, nullptr);
}

int gi_accum_export_packed(gi_ctx *c, void *packed, int64_t cap, int64_t *bytes) {
  if (!c) return GI_ERR_ARG;
  if (int rc = check_accum(c)) return rc;
  if (!packed && !bytes) return fail(c, GI_ERR_ARG, "null state buffers");
  const size_t npix = (size_t)c->acc_w * c->acc_h;
  if (bytes) *bytes = (int64_t)npix * 56;
  if (!packed) return GI_OK;
  if (cap < (int64_t)npix * 56) return fail(c, GI_ERR_ARG, "packed buffer smaller than the state");
  DeviceScope dev(c->device);
  HIPCHK(c, hipMemcpyAsync(packed, c->res.acc.p, npix * 48, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync((uint8_t *)packed + npix * 48, c->res.acc_cnt.p, npix * 8,
                           hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GI_OK;
}

int gi_accum_merge_packed(gi_ctx *c, int nstates, const void *packed, int64_t stride, double *kernel_ms) {
  if (!c) return GI_ERR_ARG;
  if (int rc = check_accum(c)) return rc;
  if (!packed || nstates < 1) return fail(c, GI_ERR_ARG, "accumulator merge: no states");
  if ((uintptr_t)packed % 8) return fail(c, GI_ERR_ARG, "accumulator merge: states not 8-byte aligned");
  if (stride < (int64_t)c->acc_w * c->acc_h * 56 || stride % 8)
    return fail(c, GI_ERR_ARG, "accumulator merge: stride below the state's size or not a multiple of 8");
  DeviceScope dev(c->device);
  return fold_states(c, nstates, packed, stride, kernel_ms);
}

int gi_accum_merge_from(gi_ctx *c, gi_ctx *src, double *kernel_ms) {
  if (!c || !src) return GI_ERR_ARG;
  if (c == src) return fail(c, GI_ERR_ARG, "accumulator merge: source is the destination");
  if (!src->peers.empty())
    return fail(c, GI_ERR_UNSUPPORTED, "the accumulator is for one-device contexts");
  if (int rc = check_accum(c)) return rc;
  if (!src->acc_valid) return fail(c, GI_ERR_STATE, "the source has no accumulator (gi_accum_reset)");
  if (src->acc_w != c->acc_w || src->acc_h != c->acc_h)
    return fail(c, GI_ERR_ARG, "accumulator state: not the accumulator's size");
  DeviceScope dev(c->device);
  const size_t npix = (size_t)c->acc_w * c->acc_h;
  DBuf packed;
  HIPCHK(c, packed.ensure(npix * 56));
  uint8_t *cnt = packed.as<uint8_t>() + npix * 48;
  // every accumulator call ends synchronised, so the source's planes are complete
  if (src->device == c->device) {
    HIPCHK(c, hipMemcpyAsync(packed.p, src->res.acc.p, npix * 48, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(cnt, src->res.acc_cnt.p, npix * 8, hipMemcpyDeviceToDevice, c->stream));
  } else {
    HIPCHK(c, hipMemcpyPeerAsync(packed.p, c->device, src->res.acc.p, src->device, npix * 48, c->stream));
    HIPCHK(c, hipMemcpyPeerAsync(cnt, c->device, src->res.acc_cnt.p, src->device, npix * 8, c->stream));
  }
  return fold_states(c, 1, packed.p, (int64_t)npix * 56, kernel_ms);
}

// ---- adaptive passes (gi.h "adaptive passes"; tile_error_kernel, tile_select_kernel) ----------
void gi_adaptive_params_default(gi_adaptive_params *p) {
  p->tile_px = 8;
  p->min_samples = 8;
  p->max_samples = 0;
  p->dilate = 1;
  p->threshold = 0.02;
}

static int check_adaptive(gi_ctx *c, const gi_adaptive_params *p) {
  if (!p) return fail(c, GI_ERR_ARG, "adaptive: null parameters");
  if (p->tile_px < 4 || p->tile_px > 64) return fail(c, GI_ERR_ARG, "adaptive: tile_px outside 4..64");
  if (p->min_samples < 0 || p->max_samples < 0)
    return fail(c, GI_ERR_ARG, "adaptive: negative min_samples or max_samples");
  if (p->dilate != 0 && p->dilate != 1) return fail(c, GI_ERR_ARG, "adaptive: dilate must be 0 or 1");
  if (!std::isfinite(p->threshold) || p->threshold < 0.0)
    return fail(c, GI_ERR_ARG, "adaptive: threshold must be finite and not negative");
  return GI_OK;
}

// pixels of the tile mask's active tiles inside the w x h frame
static int64_t mask_pixels(int w, int h, int tile, const uint8_t *mask, int64_t *tiles) {
  const int tx = (w + tile - 1) / tile, ty = (h + tile - 1) / tile;
  int64_t n = 0, nt = 0;
  for (int t = 0; t < tx * ty; t++) {
    if (!mask[t]) continue;
    const int x0 = (t % tx) * tile, y0 = (t / tx) * tile;
    n += (int64_t)(std::min(w, x0 + tile) - x0) * (std::min(h, y0 + tile) - y0);
    nt++;
  }
  if (tiles) *tiles = nt;
  return n;
}

// the selection into mask (host, one byte per tile); tile_error (host, optional)
static int accum_select(gi_ctx *c, const gi_adaptive_params *p, std::vector<uint8_t> &mask,
                        double *tile_error) {
  DeviceScope dev(c->device);
  const int T = p->tile_px;
  const int tx = (c->acc_w + T - 1) / T, ty = (c->acc_h + T - 1) / T;
  const size_t nt = (size_t)tx * ty;
  HIPCHK(c, c->s.tile_err.ensure(nt * 8));
  HIPCHK(c, c->s.tile_nmin.ensure(nt * 8));
  HIPCHK(c, c->s.tile_mask.ensure(nt));
  TileArgs a;
  memset(&a, 0, sizeof a);
  a.width = c->acc_w;
  a.height = c->acc_h;
  a.T = T;
  a.tiles_x = tx;
  a.tiles_y = ty;
  a.acc = c->res.acc.as<double>();
  a.counts = c->res.acc_cnt.as<int64_t>();
  a.tile_error = c->s.tile_err.as<double>();
  a.tile_nmin = c->s.tile_nmin.as<int64_t>();
  launch_tile_error(a, c->stream);
  HIPCHK(c, hipGetLastError());
  SelectArgs s;
  memset(&s, 0, sizeof s);
  s.tiles_x = tx;
  s.tiles_y = ty;
  s.dilate = p->dilate;
  s.min_samples = p->min_samples;
  s.max_samples = p->max_samples;
  s.threshold = p->threshold;
  s.tile_error = a.tile_error;
  s.tile_nmin = a.tile_nmin;
  s.mask = c->s.tile_mask.as<uint8_t>();
  launch_tile_select(s, c->stream);
  HIPCHK(c, hipGetLastError());
  mask.resize(nt);
  HIPCHK(c, hipMemcpyAsync(mask.data(), c->s.tile_mask.p, nt, hipMemcpyDeviceToHost, c->stream));
  if (tile_error)
    HIPCHK(c, hipMemcpyAsync(tile_error, c->s.tile_err.p, nt * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GI_OK;
}

int gi_accum_select(gi_ctx *c, const gi_adaptive_params *p, uint8_t *mask, double *tile_error,
                    int64_t *active_tiles, int64_t *active_pixels) {
  if (!c) return GI_ERR_ARG;
  int rc = check_accum(c);
  if (!rc) rc = check_adaptive(c, p);
  if (rc) return rc;
  std::vector<uint8_t> m;
  rc = accum_select(c, p, m, tile_error);
  if (rc) return rc;
  if (mask) memcpy(mask, m.data(), m.size());
  int64_t nt = 0;
  const int64_t np = mask_pixels(c->acc_w, c->acc_h, p->tile_px, m.data(), &nt);
  if (active_tiles) *active_tiles = nt;
  if (active_pixels) *active_pixels = np;
  return GI_OK;
}

// one camera pass over the mask's tiles: the list is built on the host like a tile shard's
// (shard_pixels: tiles in order, rows inside a tile), rendered, and folded into its pixels only
static int accum_add_tiles(gi_ctx *c, int aa, int tile, const uint8_t *mask, int64_t *active_pixels,
                           gi_render_stats *st) {
  if (aa < 0 || aa > 15) return fail(c, GI_ERR_ARG, "bad image size");
  const int w = c->acc_w, h = c->acc_h;
  const int tx = (w + tile - 1) / tile, ty = (h + tile - 1) / tile;
  std::vector<int32_t> pix;
  pix.reserve((size_t)mask_pixels(w, h, tile, mask, nullptr) * 2);
  for (int t = 0; t < tx * ty; t++) {
    if (!mask[t]) continue;
    const int x0 = (t % tx) * tile, y0 = (t / tx) * tile;
    for (int y = y0; y < std::min(h, y0 + tile); y++)
      for (int x = x0; x < std::min(w, x0 + tile); x++) {
        pix.push_back(x);
        pix.push_back(y);
      }
  }
  const int64_t n = (int64_t)pix.size() / 2;
  if (active_pixels) *active_pixels = n;
  if (n == 0) {  // nothing to render, nothing launched
    if (st) memset(st, 0, sizeof *st);
    return GI_OK;
  }
  // render_pixels sizes its batches by the largest queries per primary sample seen so far. That
  // rate was measured on whole frames and is low for a list made of the expensive tiles, so it is
  // measured again on this list (as after gi_set_camera) and the frames' rate put back afterwards.
  const double frame_rate = c->q_per_prim;
  c->q_per_prim = 0.0;
  int64_t S = 0;
  int rc = radiance_pass(c, aa, w, h, false, st, nullptr, &S, &pix);
  c->q_per_prim = frame_rate;
  if (rc) return rc;
  AccumArgs a;
  memset(&a, 0, sizeof a);
  a.npix = n;
  a.S = S;
  a.pass = c->s.rad_frame.as<double>();
  a.acc = c->res.acc.as<double>();
  a.counts = c->res.acc_cnt.as<int64_t>();
  a.pixels = c->s.pixels.as<int2>();  // the list as render_pixels uploaded it
  a.width = w;
  launch_accum_merge(a, c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n == (int64_t)w * h)
    c->acc_n += S;
  else
    c->acc_uniform = false;
  return GI_OK;
}

int gi_accum_add_tiles(gi_ctx *c, int aa, int tile_px, const uint8_t *mask, int64_t *active_pixels,
                       gi_render_stats *st) {
  if (!c) return GI_ERR_ARG;
  int rc = check_accum(c);
  if (rc) return rc;
  if (tile_px < 4 || tile_px > 64) return fail(c, GI_ERR_ARG, "adaptive: tile_px outside 4..64");
  if (!mask) return fail(c, GI_ERR_ARG, "adaptive: null tile mask");
  return accum_add_tiles(c, aa, tile_px, mask, active_pixels, st);
}

int gi_accum_add_adaptive(gi_ctx *c, int aa, const gi_adaptive_params *p, uint8_t *mask,
                          int64_t *active_pixels, gi_render_stats *st) {
  if (!c) return GI_ERR_ARG;
  int rc = check_accum(c);
  if (!rc) rc = check_adaptive(c, p);
  if (rc) return rc;
  if (aa < 0 || aa > 15) return fail(c, GI_ERR_ARG, "bad image size");
  std::vector<uint8_t> m;
  rc = accum_select(c, p, m, nullptr);
  if (rc) return rc;
  if (mask) memcpy(mask, m.data(), m.size());
  return accum_add_tiles(c, aa, p->tile_px, m.data(), active_pixels, st);
}

int gi_accum_get(gi_ctx *c, float *mean, float *variance, int64_t *nsamples, double *noise) {
  if (!c) return GI_ERR_ARG;
  int rc = check_accum(c);
  if (rc) return rc;
  DeviceScope dev(c->device);
  const size_t npix = (size_t)c->acc_w * c->acc_h;
  if (nsamples) {
    *nsamples = c->acc_n;
    if (!c->acc_uniform) {
      if ((rc = count_stats(c, nsamples, nullptr))) return rc;
    }
  }
  rc = radiance_resolve(c, c->res.acc.as<double>(), npix, 0, mean, variance, c->res.acc_cnt.as<int64_t>());
  if (rc || !noise) return rc;
  const size_t nb = (npix + NOISE_BLOCK - 1) / NOISE_BLOCK;
  HIPCHK(c, c->s.acc_part.ensure(nb * 8));
  NoiseArgs a;
  memset(&a, 0, sizeof a);
  a.npix = (int64_t)npix;
  a.counts = c->res.acc_cnt.as<int64_t>();
  a.acc = c->res.acc.as<double>();
  a.partial = c->s.acc_part.as<double>();
  launch_accum_noise(a, c->stream);
  HIPCHK(c, hipGetLastError());
  std::vector<double> part(nb);
  HIPCHK(c, hipMemcpyAsync(part.data(), c->s.acc_part.p, nb * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  double sum = 0.0;
  for (double v : part) sum += v;  // in block order: the result is reproducible bit for bit
  *noise = sum / (double)npix;
  return GI_OK;
}

// ---- reprojection across views (gi.h; accum_reproject_kernel) -------------------------------
void gi_reproject_params_default(gi_reproject_params *p) {
  if (!p) return;
  p->max_history = 32;
  p->depth_tol = 0.02;
  p->normal_min = 0.9;
  p->albedo_tol = 0.05;
}

static double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

int gi_accum_reproject(gi_ctx *c, const gi_view *prev_view, const gi_pixel_features *prev_feat,
                       const gi_pixel_features *cur_feat, const gi_reproject_params *pp,
                       gi_reproject_stats *stats, double *kernel_ms) {
  if (!c) return GI_ERR_ARG;
  int rc = check_accum(c);
  if (rc) return rc;
  if (!c->have_scene) return fail(c, GI_ERR_STATE, "no scene loaded (gi_read_scene)");
  if (!prev_view || !prev_feat || !cur_feat) return fail(c, GI_ERR_ARG, "reproject: null view or planes");
  gi_reproject_params P;
  gi_reproject_params_default(&P);
  if (pp) P = *pp;
  if (P.max_history < 2) return fail(c, GI_ERR_ARG, "reproject: max_history below 2");
  for (double t : {P.depth_tol, P.albedo_tol})
    if (!std::isfinite(t) || t < 0.0)
      return fail(c, GI_ERR_ARG, "reproject: tolerances must be finite and not negative");
  if (!(P.normal_min >= 0.0 && P.normal_min <= 1.0))
    return fail(c, GI_ERR_ARG, "reproject: normal_min outside [0, 1]");
  DeviceScope dev(c->device);
  const int w = c->acc_w, h = c->acc_h;
  const size_t npix = (size_t)w * h;
  const size_t nwaves = (size_t)reproject_waves(w, h);
  HIPCHK(c, c->res.acc2.ensure(npix * 48));
  HIPCHK(c, c->res.acc2_cnt.ensure(npix * 8));
  HIPCHK(c, c->s.acc_part.ensure(nwaves * 16));
  HIPCHK(c, upload(c->s.rp_prev, prev_feat, npix * sizeof(gi_pixel_features), c->stream));
  HIPCHK(c, upload(c->s.rp_cur, cur_feat, npix * sizeof(gi_pixel_features), c->stream));
  ReprojectArgs a;
  memset(&a, 0, sizeof a);
  a.W = w;
  a.H = h;
  a.max_history = P.max_history;
  a.depth_tol = P.depth_tol;
  a.nmin2 = P.normal_min * P.normal_min;
  a.atol2 = P.albedo_tol * P.albedo_tol;
  const DCamera cam = make_camera(c->scene, c->P);
  for (int i = 0; i < 3; i++) {
    a.eye1[i] = cam.eye[i];
    a.org1[i] = cam.far_org[i];
    a.right1[i] = cam.far_right[i];
    a.up1[i] = cam.far_up[i];
    a.eye0[i] = prev_view->eye[i];
    a.right0[i] = prev_view->far_right[i];
    a.up0[i] = prev_view->far_up[i];
    a.G[i] = prev_view->far_org[i] - prev_view->eye[i];
  }
  a.GG = dot3(a.G, a.G);
  a.RR = dot3(a.right0, a.right0);
  a.UU = dot3(a.up0, a.up0);
  a.acc = c->res.acc.as<double>();
  a.counts = c->res.acc_cnt.as<int64_t>();
  a.prev = c->s.rp_prev.as<float4>();
  a.cur = c->s.rp_cur.as<float4>();
  a.acc_out = c->res.acc2.as<double>();
  a.counts_out = c->res.acc2_cnt.as<int64_t>();
  a.partial = c->s.acc_part.as<int64_t>();
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (kernel_ms) {
    HIPCHK(c, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) {
      hipEventDestroy(e0);
      return fail(c, GI_ERR_HIP, "reproject: hipEventCreate failed");
    }
    (void)hipEventRecord(e0, c->stream);
  }
  launch_accum_reproject(a, c->stream);
  hipError_t le = hipGetLastError();
  if (kernel_ms) (void)hipEventRecord(e1, c->stream);
  std::vector<int64_t> part(nwaves * 2);
  if (le == hipSuccess)
    le = hipMemcpyAsync(part.data(), c->s.acc_part.p, nwaves * 16, hipMemcpyDeviceToHost, c->stream);
  if (le == hipSuccess) le = hipStreamSynchronize(c->stream);
  if (kernel_ms) {
    float ms = 0.f;
    if (le == hipSuccess) le = hipEventElapsedTime(&ms, e0, e1);
    *kernel_ms = ms;
    hipEventDestroy(e0);
    hipEventDestroy(e1);
  }
  HIPCHK(c, le);
  std::swap(c->res.acc, c->res.acc2);
  std::swap(c->res.acc_cnt, c->res.acc2_cnt);
  c->acc_uniform = false;  // every pixel under its own count from here on
  if (stats) {
    int64_t kept = 0, samples = 0;
    for (size_t v = 0; v < nwaves; v++) {
      kept += part[2 * v];
      samples += part[2 * v + 1];
    }
    stats->kept_pixels = kept;
    stats->reset_pixels = (int64_t)npix - kept;
    stats->kept_samples = samples;
  }
  return GI_OK;
}

// ---- variance-guided denoise (gi_denoise.hip vdenoise_*; no reference counterpart) --------
void gi_vdenoise_params_default(gi_vdenoise_params *p) {
  if (!p) return;
  p->levels = 5;
  p->normal_power_log2 = 5;
  p->sigma_lum = 4.0;
  p->sigma_depth = 0.05;
  p->sigma_albedo = 0.1;
  p->variance_floor = 1e-6;
}

// pp (null: defaults) checked into P
static int vdenoise_params(gi_ctx *c, const gi_vdenoise_params *pp, gi_vdenoise_params &P) {
  gi_vdenoise_params_default(&P);
  if (pp) P = *pp;
  if (P.levels < 1 || P.levels > 8) return fail(c, GI_ERR_ARG, "vdenoise: levels outside 1..8");
  if (P.normal_power_log2 < 0 || P.normal_power_log2 > 8)
    return fail(c, GI_ERR_ARG, "vdenoise: normal_power_log2 outside 0..8");
  for (double s : {P.sigma_lum, P.sigma_depth, P.sigma_albedo, P.variance_floor})
    if (!std::isfinite(s) || !(s > 0.0))
      return fail(c, GI_ERR_ARG, "vdenoise: sigmas and variance_floor must be finite and positive");
  return GI_OK;
}

// The levels over c->s.dn_img[0] (packed {r, g, b, v0}) and the planes uploaded from feat, then the
// outputs (either may be null) to the host.
static int vdenoise_levels(gi_ctx *c, int w, int h, const gi_pixel_features *feat,
                           const gi_vdenoise_params &P, float *out_mean, float *out_vlum,
                           double *kernel_ms) {
  const size_t npix = (size_t)w * h;
  HIPCHK(c, upload(c->s.dn_planes, feat, npix * sizeof(gi_pixel_features), c->stream));
  HIPCHK(c, c->s.dn_img[1].ensure(npix * sizeof(float4)));
  if (out_mean) HIPCHK(c, c->s.dn_rgbf.ensure(npix * 12));
  if (out_vlum) HIPCHK(c, c->s.vdn_vlum.ensure(npix * 4));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (kernel_ms) {
    HIPCHK(c, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) {
      hipEventDestroy(e0);
      return fail(c, GI_ERR_HIP, "vdenoise: hipEventCreate failed");
    }
    (void)hipEventRecord(e0, c->stream);
  }
  VDenoiseArgs a;
  memset(&a, 0, sizeof a);
  a.W = w;
  a.H = h;
  a.npow = P.normal_power_log2;
  a.sl2 = P.sigma_lum * P.sigma_lum;
  a.vfloor = P.variance_floor;
  a.sd2 = P.sigma_depth * P.sigma_depth;
  a.isa2 = 1.0 / (P.sigma_albedo * P.sigma_albedo);
  a.planes = c->s.dn_planes.as<float4>();
  int cur = 0;
  hipError_t le = hipSuccess;
  for (int l = 0; l < P.levels && le == hipSuccess; l++) {
    a.step = 1 << l;
    a.src = c->s.dn_img[cur].as<float4>();
    a.dst = c->s.dn_img[cur ^ 1].as<float4>();
    launch_vdenoise_level(a, c->stream);
    le = hipGetLastError();
    cur ^= 1;
  }
  if (kernel_ms) (void)hipEventRecord(e1, c->stream);
  if (le == hipSuccess) {
    launch_vdenoise_unpack(c->s.dn_img[cur].as<float4>(), (int64_t)npix,
                           out_mean ? c->s.dn_rgbf.as<float>() : nullptr,
                           out_vlum ? c->s.vdn_vlum.as<float>() : nullptr, c->stream);
    le = hipGetLastError();
  }
  if (le == hipSuccess && out_mean)
    le = hipMemcpyAsync(out_mean, c->s.dn_rgbf.p, npix * 12, hipMemcpyDeviceToHost, c->stream);
  if (le == hipSuccess && out_vlum)
    le = hipMemcpyAsync(out_vlum, c->s.vdn_vlum.p, npix * 4, hipMemcpyDeviceToHost, c->stream);
  if (le == hipSuccess) le = hipStreamSynchronize(c->stream);
  if (kernel_ms) {
    float ms = 0.f;
    if (le == hipSuccess) le = hipEventElapsedTime(&ms, e0, e1);
    *kernel_ms = ms;
    hipEventDestroy(e0);
    hipEventDestroy(e1);
  }
  HIPCHK(c, le);
  return GI_OK;
}

int gi_denoise_radiance(gi_ctx *c, int w, int h, const float *mean, const float *variance,
                        const gi_pixel_features *feat, const gi_vdenoise_params *pp, float *out_mean,
                        float *out_vlum, double *kernel_ms) {
  if (!c) return GI_ERR_ARG;
  if (!mean || !variance || !feat || (!out_mean && !out_vlum))
    return fail(c, GI_ERR_ARG, "null image buffer");
  if (w <= 0 || h <= 0 || (int64_t)w * h >= ((int64_t)1 << 31))
    return fail(c, GI_ERR_ARG, "bad image size");
  gi_vdenoise_params P;
  int rc = vdenoise_params(c, pp, P);
  if (rc) return rc;
  DeviceScope dev(c->device);
  const size_t npix = (size_t)w * h;
  HIPCHK(c, upload(c->s.dn_rgbf, mean, npix * 12, c->stream));
  HIPCHK(c, upload(c->s.vdn_var, variance, npix * 12, c->stream));
  HIPCHK(c, c->s.dn_img[0].ensure(npix * sizeof(float4)));
  launch_vdenoise_pack(c->s.dn_rgbf.as<float>(), c->s.vdn_var.as<float>(), (int64_t)npix,
                       c->s.dn_img[0].as<float4>(), c->stream);
  HIPCHK(c, hipGetLastError());
  return vdenoise_levels(c, w, h, feat, P, out_mean, out_vlum, kernel_ms);
}

int gi_accum_denoise(gi_ctx *c, const gi_pixel_features *feat, const gi_vdenoise_params *pp,
                     float *out_mean, float *out_vlum, double *kernel_ms) {
  if (!c) return GI_ERR_ARG;
  int rc = check_accum(c);
  if (rc) return rc;
  if (!feat || (!out_mean && !out_vlum)) return fail(c, GI_ERR_ARG, "null image buffer");
  gi_vdenoise_params P;
  rc = vdenoise_params(c, pp, P);
  if (rc) return rc;
  DeviceScope dev(c->device);
  int64_t least = c->acc_n;
  if (!c->acc_uniform && (rc = count_stats(c, &least, nullptr))) return rc;
  if (least < 2)
    return fail(c, GI_ERR_STATE, "vdenoise: every pixel of the accumulator needs at least 2 samples");
  const size_t npix = (size_t)c->acc_w * c->acc_h;
  HIPCHK(c, c->s.dn_img[0].ensure(npix * sizeof(float4)));
  launch_vdenoise_pack_accum(c->res.acc.as<double>(), c->res.acc_cnt.as<int64_t>(), (int64_t)npix,
                             c->s.dn_img[0].as<float4>(), c->stream);
  HIPCHK(c, hipGetLastError());
  return vdenoise_levels(c, c->acc_w, c->acc_h, feat, P, out_mean, out_vlum, kernel_ms);
}

void gi_progressive_params_default(gi_progressive_params *p) {
  if (!p) return;
  p->alpha = 0.7;
  p->global_radius = 0.0;
  p->caustic_radius = 0.0;
}

// Knaus & Zwicker's radius schedule, r_{j+1}^2 = r_j^2 (j + alpha) / (j + 1) with j counted from 1:
// host arithmetic, one IEEE operation per step (tests/progressive_ref.py restates it)
double gi_progressive_radius(double r0, double alpha, int64_t pass) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (!(r0 > 0.0) || !std::isfinite(r0) || !(alpha > 0.0 && alpha < 1.0) || pass < 0 ||
      pass >= ((int64_t)1 << 20))
    return nan;
  double r2 = r0 * r0;
  for (int64_t j = 1; j <= pass; j++) r2 = (r2 * ((double)j + alpha)) / ((double)j + 1.0);
  return std::sqrt(r2);
}

int gi_accum_add_progressive(gi_ctx *c, int aa, int64_t pass, const gi_progressive_params *pp,
                             gi_photon_stats *pstats, gi_render_stats *st) {
  if (!c) return GI_ERR_ARG;
  if (!c->peers.empty())
    return fail(c, GI_ERR_UNSUPPORTED, "progressive passes are for one-device contexts");
  if (!c->have_scene) return fail(c, GI_ERR_STATE, "no scene loaded (gi_read_scene)");
  int rc = check_accum(c);
  if (rc) return rc;
  gi_progressive_params D;
  gi_progressive_params_default(&D);
  if (pp) D = *pp;
  const gi_params P = c->P;
  if (P.irradiance_cache)
    return fail(c, GI_ERR_ARG, "progressive passes do not take the irradiance cache");
  if (aa < 0 || aa > 15) return fail(c, GI_ERR_ARG, "bad image size");
  if (pass < 0 || pass >= ((int64_t)1 << 20))
    return fail(c, GI_ERR_ARG, "progressive pass index must be in [0, 2^20)");
  if (!(D.alpha > 0.0 && D.alpha < 1.0))
    return fail(c, GI_ERR_ARG, "progressive alpha must be inside (0, 1)");
  const double r0g = D.global_radius == 0.0 ? P.global_estimate_dist : D.global_radius;
  const double r0c = D.caustic_radius == 0.0 ? P.caustic_estimate_dist : D.caustic_radius;
  const double rg = gi_progressive_radius(r0g, D.alpha, pass);
  const double rcst = gi_progressive_radius(r0c, D.alpha, pass);
  if (std::isnan(rg) || std::isnan(rcst))
    return fail(c, GI_ERR_ARG, "progressive radii must be finite and positive");
  gi_params Q = P;
  Q.seed = P.seed + (uint64_t)pass;
  Q.global_estimate_size = GI_ESTIMATE_ALL;
  Q.caustic_estimate_size = GI_ESTIMATE_ALL;
  Q.global_estimate_dist = rg;
  Q.caustic_estimate_dist = rcst;
  rc = gi_set_params(c, &Q);
  if (!rc) rc = gi_map_photons(c, pstats);
  if (!rc) rc = gi_accum_add_image(c, aa, st);
  // the context's own parameters come back whatever happened; the maps stay the pass's
  const int rc2 = gi_set_params(c, &P);
  return rc ? rc : rc2;
}

int gi_tonemap(gi_ctx *c, int w, int h, const float *radiance, double exposure, double white,
               float *out_rgbf, uint8_t *out_rgb8) {
  if (!c) return GI_ERR_ARG;
  if (!radiance || (!out_rgbf && !out_rgb8)) return fail(c, GI_ERR_ARG, "null image buffer");
  if (w <= 0 || h <= 0 || (int64_t)w * h >= ((int64_t)1 << 31))
    return fail(c, GI_ERR_ARG, "bad image size");
  if (!std::isfinite(exposure) || !(exposure > 0.0))
    return fail(c, GI_ERR_ARG, "tonemap: exposure must be finite and positive");
  if (!std::isfinite(white) || white < 0.0)
    return fail(c, GI_ERR_ARG, "tonemap: white must be finite and not negative");
  DeviceScope dev(c->device);
  const size_t nval = (size_t)w * h * 3;
  HIPCHK(c, upload(c->s.tm_in, radiance, nval * 4, c->stream));
  HIPCHK(c, c->s.tm_out.ensure(nval * 4));
  TonemapArgs a;
  memset(&a, 0, sizeof a);
  a.nval = (int64_t)nval;
  a.exposure = exposure;
  a.white = white;
  a.in = c->s.tm_in.as<float>();
  a.out = c->s.tm_out.as<float>();
  launch_tonemap(a, c->stream);
  HIPCHK(c, hipGetLastError());
  std::vector<float> stage;
  float *dst = out_rgbf;
  if (!dst) {
    stage.resize(nval);
    dst = stage.data();
  }
  HIPCHK(c, hipMemcpyAsync(dst, c->s.tm_out.p, nval * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (out_rgb8) return gi_quantize(w, h, dst, out_rgb8);
  return GI_OK;
}

}  // extern "C"
