// photonmap.cpp -- drop-in CLI: `photonmap src.scn out.png [-FLAGS]` on the MI355X path.
//
// Same control flow and reports as the reference main (photonmap.cpp:442-499):
// ParseArgs -> ReadScene -> MapPhotons (if indirect|caustic|photon_viz) -> RenderImage ->
// WriteImage, with the -v statistics of io_utils.cpp:240-246, photonmap.cpp:416-435 and
// render.cpp:224-255. Exit codes: 1 for a bad flag, -1 (255) for load/render/write failures.
//
// The extension flags. ParseCommandLine takes them out of argv before gi_parse_args, which keeps the
// reference's flag set, and refuses what is listed before a device is opened. "bad" is the exit code of
// a malformed flag: 1 with the reference's "Invalid program argument: FLAG" and no newline, -1 with a
// line of its own. R marks a radiance flag: with any of them the maps are built once, pass i is rendered
// under seed + i and folded into the context's accumulator (gi_accum_*), and the written image is
// gi_tonemap of the unclamped mean; one device only (refused with -gpus N or such a GI_DEVICES, exit -1).
//
//   flag, values                  bad  refused with              what it does
//   -camera EX EY EZ TX TY TZ      1                             renders from that camera (gi_set_camera; the numbers of the
//           UX UY UZ XFOV                                        .scn `camera` command) instead of the scene file's
//   -denoise L (1..8)              1   -vdenoise, -views         writes the frame filtered by L levels of the edge-avoiding
//                                                                a-trous pass (gi_camera_features + gi_denoise, defaults)
//   -passes N (1..4096)            1                         R   N passes; default 1, or 4096 under -noise
//   -noise T (>= 0)                1                         R   stops after a pass at noise <= T (from 2 samples per pixel on)
//   -exposure E (> 0)              1                         R   gi_tonemap's exposure, default 1
//   -white W (>= 0)                1                         R   gi_tonemap's white point, default 0: linear
//   -radiance FILE (.pfm, .hdr)    1                         R   FILE receives the unfiltered mean
//   -adaptive [TILE] (4..64)       1   -progressive, -layers     only with -noise T: whole-frame passes until every pixel has the
//                                                                default min_samples, then gi_accum_add_adaptive passes over TILE x
//                                                                TILE tiles (default 8) until none is above T or -passes is used up
//   -vdenoise L (1..8)             1   -denoise              R   the written image is gi_tonemap of the accumulator filtered by L
//                                                                levels of the variance-guided pass (gi_accum_denoise, defaults)
//   -views FILE                   -1   -denoise, -save_accum, R  one camera per line of FILE, ten numbers as in -camera (blank
//                                      -load_accum, -layers,     and # lines skipped); view k gets gi_set_camera and the pass
//                                      -progressive              loop; its image and -radiance file get .%04d of k before the extension
//   -history H (>= 2)             -1   (only with -views)        from the second view on the accumulator is carried into the new
//                                                                camera (gi_accum_reproject, max_history = H); with -adaptive the
//                                                                view goes straight to adaptive passes, which refine lost history
//   -save_accum FILE               1   -views, -layers       R   writes the accumulator's fp64 state as the pass loop leaves it
//                                                                (gi_accum_export; AccumFile below) and the passes behind it
//   -load_accum FILE               1   -views, -layers       R   starts from such a file (gi_accum_import): pass i runs under seed +
//                                                                passes_done + i and -passes N means N more, at least one, so a
//                                                                resumed run ends with the bits of the uninterrupted one. A file
//                                                                that is not a W x H accumulator's exits -1
//   -progressive A (0 < A < 1)     1   -adaptive, -views,    R   progressive photon mapping: no maps up front, pass i is
//                                      -cache, -layers           gi_accum_add_progressive with index passes_done + i. The file of
//                                                                -save_accum does not record A: a resumed run repeats the flag
//   -layers PREFIX                 1   -adaptive, -views,        the light-path layers (gi.h GI_LAYER_*) as float means in PREFIX
//                                      -progressive, -gpus N,    + _surface.pfm, _specular, _indirect, _global, _caustic: of one
//                                      -save_accum, -load_accum  more frame (gi_render_layers) or, with an R flag, of layered
//                                      (these exit 1)            passes over five scene-less contexts. With -vdenoise every layer
//                                                                but the specular one is filtered under its own variance and the
//                                                                image is gi_tonemap of their sum: what a mirror shows is not
//                                                                filtered by the planes of the mirror
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>
#include "../../include/gi.h"

// PrintProgress (io_utils.cpp:257-268) with the reference's bar width (photonmap.cpp:132);
// a bar is redrawn when its percentage changes (render.cpp:82-86, photontracer.cpp:168-173)
static const int PROGRESS_BAR_WIDTH = 50;
static void PrintProgress(double progress, int width) {
  printf("[");
  int pos = (int)(width * progress);
  for (int j = 0; j < width; j++) printf("%s", j < pos ? "=" : (j == pos ? ">" : " "));
  printf("] %d%%\r", (int)(progress * 100.0));
  fflush(stdout);
}
struct ProgressState {
  bool verbose;
  int last[3];
};
static void OnProgress(int stage, double progress, void *user) {
  ProgressState *s = (ProgressState *)user;
  if (stage > 0 && !s->verbose) return;  // photon-map bars only with -v (photonmap.cpp:193)
  const int v = (int)(progress * 100.0);
  if (stage == 0 && v >= 100) return;  // the final bar is printed after RenderImage returns
  if (v == s->last[stage]) return;
  s->last[stage] = v;
  PrintProgress(progress, PROGRESS_BAR_WIDTH);
}

// ---- the argument stage ----------------------------------------------------------------------
// prints the message on stderr and hands back the exit code: `return Fail(-1, ...)`
static int Fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  return code;
}
static int Invalid(const char *flag) { return Fail(1, "Invalid program argument: %s", flag); }
// the whole of text as an integer in lo..hi
static bool ParseInt(const char *text, long lo, long hi, long *v) {
  char *end = nullptr;
  *v = strtol(text, &end, 10);
  return end != text && !*end && *v >= lo && *v <= hi;
}
// the whole of text as strtod reads it (nan and inf too), and as a finite number
static bool ParseReal(const char *text, double *v) {
  char *end = nullptr;
  *v = strtod(text, &end);
  return end != text && !*end;
}
static bool ParseNumber(const char *text, double *v) { return ParseReal(text, v) && *v == *v && *v - *v == 0.0; }
// Takes every `flag ...` out of argv. check(n, tok) sees the n tokens after an occurrence and
// returns how many of them belong to the flag, or -1 to refuse (then false, argv as it is).
template <class Check>
static bool TakeFlag(int &argc, char **argv, const char *flag, Check check) {
  for (int a = 1; a < argc;) {
    if (strcmp(argv[a], flag)) { a++; continue; }
    const int take = 1 + check(argc - a - 1, argv + a + 1);
    if (take < 1) return false;
    for (int k = a + take; k < argc; k++) argv[k - take] = argv[k];
    argc -= take;
  }
  return true;
}
static gi_camera CameraFromNumbers(const double v[10]) {
  gi_camera cam;
  for (int i = 0; i < 3; i++) { cam.eye[i] = v[i]; cam.towards[i] = v[3 + i]; cam.up[i] = v[6 + i]; }
  cam.xfov = v[9];
  return cam;
}
// `-camera` and its ten numbers; every occurrence is checked, the last one wins
static bool TakeCamera(int &argc, char **argv, gi_camera &cam, bool &have) {
  return TakeFlag(argc, argv, "-camera", [&](int n, char **tok) {
    double v[10];
    for (int k = 0; k < 10; k++)
      if (k >= n || !ParseReal(tok[k], &v[k])) return -1;
    cam = CameraFromNumbers(v);
    have = true;
    return 10;
  });
}
// `-denoise L` / `-vdenoise L`, L in 1..8; every occurrence is checked, the last one wins
static bool TakeLevels(int &argc, char **argv, const char *flag, int &levels) {
  return TakeFlag(argc, argv, flag, [&](int n, char **tok) {
    long v;
    if (n < 1 || !ParseInt(tok[0], 1, 8, &v)) return -1;
    levels = (int)v;
    return 1;
  });
}
// `flag value`: *value = the last occurrence's text, the only one that its caller then checks
// (untouched when the flag is absent); false when the flag is last in argv
static bool TakeValue(int &argc, char **argv, const char *flag, const char **value) {
  return TakeFlag(argc, argv, flag, [&](int n, char **tok) {
    if (n < 1) return -1;
    *value = tok[0];
    return 1;
  });
}
// `flag X`, X a finite number that ok() accepts: *v = X and *given = true; false when malformed
static bool TakeNumber(int &argc, char **argv, const char *flag, bool (*ok)(double), double *v, bool *given) {
  const char *text = nullptr;
  if (!TakeValue(argc, argv, flag, &text) || (text && !(ParseNumber(text, v) && ok(*v)))) return false;
  if (text) *given = true;
  return true;
}
// `-adaptive [TILE]`: the token after it is TILE only when it is an integer (refused outside
// 4..64); every occurrence is checked and resets the tile to 8, the last one wins
static bool TakeAdaptive(int &argc, char **argv, int &tile) {
  return TakeFlag(argc, argv, "-adaptive", [&](int n, char **tok) {
    long v;
    tile = 8;
    if (n < 1 || !ParseInt(tok[0], LONG_MIN, LONG_MAX, &v)) return 0;
    if (v < 4 || v > 64) return -1;
    tile = (int)v;
    return 1;
  });
}

// The accumulator's file (gi.h "accumulator state", little-endian): a 32-byte header {"GIACC01\n",
// int32 width, int32 height, int64 passes_done, 8 zero bytes}, the state plane (W*H*6 doubles),
// the counts plane (W*H int64).
static const char ACCUM_MAGIC[9] = "GIACC01\n";
struct AccumFile {
  std::vector<double> state;
  std::vector<int64_t> counts;
  int64_t passes_done = 0;
};
// empty, or why the file is not the state of a w x h accumulator
static std::string ReadAccum(const char *path, int w, int h, AccumFile &a) {
  FILE *f = fopen(path, "rb");
  if (!f) return "cannot open it";
  unsigned char head[32];
  int32_t fw = 0, fh = 0;
  std::string why;
  if (fread(head, 1, 32, f) != 32) why = "shorter than its header";
  else if (memcmp(head, ACCUM_MAGIC, 8)) why = "not an accumulator file (bad magic)";
  else {
    memcpy(&fw, head + 8, 4);
    memcpy(&fh, head + 12, 4);
    memcpy(&a.passes_done, head + 16, 8);
    if (fw != w || fh != h)
      why = "it holds " + std::to_string(fw) + " x " + std::to_string(fh) + " pixels, -resolution is " +
            std::to_string(w) + " x " + std::to_string(h);
    else if (a.passes_done < 0) why = "negative pass count";
  }
  if (why.empty()) {
    const size_t npix = (size_t)w * h;
    a.state.resize(npix * 6);
    a.counts.resize(npix);
    if (fread(a.state.data(), 8, npix * 6, f) != npix * 6 || fread(a.counts.data(), 8, npix, f) != npix)
      why = "shorter than its " + std::to_string(32 + npix * 56) + " bytes";
    else if (fgetc(f) != EOF)
      why = "longer than its " + std::to_string(32 + npix * 56) + " bytes";
    else if (std::any_of(a.counts.begin(), a.counts.end(), [](int64_t n) { return n < 0; }))
      why = "negative sample count";
  }
  fclose(f);
  return why;
}
static bool WriteAccum(const char *path, int w, int h, const AccumFile &a) {
  FILE *f = fopen(path, "wb");
  if (!f) return false;
  unsigned char head[32];
  const int32_t fw = w, fh = h;
  memset(head, 0, sizeof head);
  memcpy(head, ACCUM_MAGIC, 8);
  memcpy(head + 8, &fw, 4);
  memcpy(head + 12, &fh, 4);
  memcpy(head + 16, &a.passes_done, 8);
  bool ok = fwrite(head, 1, 32, f) == 32 &&
            fwrite(a.state.data(), 8, a.state.size(), f) == a.state.size() &&
            fwrite(a.counts.data(), 8, a.counts.size(), f) == a.counts.size();
  return (fclose(f) == 0) && ok;
}

// -views FILE: one camera per line, ten numbers as in -camera; blank lines and lines starting with
// # are skipped. false with bad_line = 0 when the file cannot be opened, else on the first line
// that is not ten finite numbers.
static bool ReadViews(const char *path, std::vector<gi_camera> &views, int &bad_line) {
  FILE *f = fopen(path, "r");
  if (!f) return false;
  char line[4096];
  for (int ln = 1; fgets(line, sizeof line, f); ln++) {
    const char *q = line;
    while (*q == ' ' || *q == '\t' || *q == '\r' || *q == '\n') q++;
    if (!*q || *q == '#') continue;
    double v[10];
    int n = 0;
    bool ok = true;
    while (ok) {
      while (*q == ' ' || *q == '\t' || *q == '\r' || *q == '\n') q++;
      if (!*q) break;
      char *end = nullptr;
      const double x = strtod(q, &end);
      if (end == q || !(x - x == 0.0) || n == 10) ok = false;
      else v[n++] = x;
      q = end;
    }
    if (!ok || n != 10) {
      bad_line = ln;
      fclose(f);
      return false;
    }
    views.push_back(CameraFromNumbers(v));
  }
  fclose(f);
  return true;
}

// what the command line asks for: gi_parse_args' outputs and the extension flags
struct Options {
  gi_params P;
  const char *scene = nullptr, *out = nullptr;
  int w = 1024, h = 1024, aa = 2, real = 0;
  gi_device_set ds;
  bool have_cam = false;
  gi_camera cam;
  int denoise_levels = 0, vdenoise_levels = 0;  // 0: no such pass
  bool any = false;  // one of the radiance flags is given: the frame comes from the accumulator
  bool have_noise = false;
  int adaptive_tile = 0;  // 0: uniform passes
  int passes = 0;
  double noise = 0.0, exposure = 1.0, white = 0.0;
  const char *radiance_file = nullptr, *save_accum = nullptr, *load_accum = nullptr;
  bool progressive = false;  // -progressive A: fresh photon maps and a shrinking fixed radius per pass
  double alpha = 0.0;
  const char *layers_prefix = nullptr;
  std::vector<gi_camera> views;
  long history = 0;  // 0: every view starts from an empty accumulator
  AccumFile loaded;  // -load_accum; passes_done = 0 without
};

// -adaptive, -passes, -noise, -exposure, -white, -radiance, -save_accum, -load_accum, -progressive,
// tested in this order: null, or the flag that is malformed
static const char *TakeRadiance(int &argc, char **argv, Options &o) {
  const char *t = nullptr;
  long n = 0;
  if (!TakeAdaptive(argc, argv, o.adaptive_tile)) return "-adaptive";
  if (!TakeValue(argc, argv, "-passes", &t) || (t && !ParseInt(t, 1, 4096, &n))) return "-passes";
  if (t) o.any = true;
  o.passes = (int)n;
  if (!TakeNumber(argc, argv, "-noise", [](double v) { return v >= 0.0; }, &o.noise, &o.have_noise)) return "-noise";
  if (!TakeNumber(argc, argv, "-exposure", [](double v) { return v > 0.0; }, &o.exposure, &o.any)) return "-exposure";
  if (!TakeNumber(argc, argv, "-white", [](double v) { return v >= 0.0; }, &o.white, &o.any)) return "-white";
  if (!TakeValue(argc, argv, "-radiance", &o.radiance_file)) return "-radiance";
  if (o.radiance_file) {
    const char *ext = strrchr(o.radiance_file, '.');
    if (!ext || (strcmp(ext, ".pfm") && strcmp(ext, ".hdr"))) return "-radiance";
  }
  if (!TakeValue(argc, argv, "-save_accum", &o.save_accum)) return "-save_accum";
  if (!TakeValue(argc, argv, "-load_accum", &o.load_accum)) return "-load_accum";
  if (!TakeNumber(argc, argv, "-progressive", [](double v) { return v > 0.0 && v < 1.0; }, &o.alpha, &o.progressive))
    return "-progressive";
  if (o.progressive && o.adaptive_tile) return "-progressive (not with -adaptive)";
  if (o.adaptive_tile && !o.have_noise) return "-adaptive";
  if (o.have_noise || o.radiance_file || o.save_accum || o.load_accum || o.progressive) o.any = true;
  if (o.passes == 0) o.passes = o.have_noise ? 4096 : 1;
  return nullptr;
}
// -views FILE beside the flags it is refused with, then the file itself
static int TakeViews(const char *file, Options &o) {
  if (o.save_accum || o.load_accum)
    return Fail(-1, "Invalid program argument: -views (not with -save_accum or -load_accum)\n");
  if (o.progressive) return Fail(-1, "Invalid program argument: -progressive (not with -views)\n");
  if (o.denoise_levels) return Fail(-1, "Invalid program argument: -views (not with -denoise)\n");
  int bad_line = 0;
  if (!ReadViews(file, o.views, bad_line))
    return bad_line ? Fail(-1, "Unable to read views file %s: line %d is not ten numbers\n", file, bad_line)
                    : Fail(-1, "Unable to open views file %s\n", file);
  if (o.views.empty()) return Fail(-1, "Unable to read views file %s: no camera in it\n", file);
  o.any = true;
  return 0;
}
// devices: -gpus N takes devices 0..N-1 (the reference's -threads N re-cut as a device
// shard); GI_DEVICES="a,b,..." names them explicitly, GI_DEVICE the single device
static gi_device_set DeviceSet(int gpus) {
  gi_device_set ds;
  memset(&ds, 0, sizeof ds);
  ds.count = 1;
  if (const char *d = getenv("GI_DEVICE")) ds.devices[0] = atoi(d);
  if (gpus > 1) {
    ds.count = gpus < GI_MAX_DEVICES ? gpus : GI_MAX_DEVICES;
    for (int k = 0; k < ds.count; k++) ds.devices[k] = k;
  }
  if (const char *l = getenv("GI_DEVICES")) {
    ds.count = 0;
    for (const char *q = l; *q && ds.count < GI_MAX_DEVICES;) {
      ds.devices[ds.count++] = atoi(q);
      while (*q && *q != ',') q++;
      if (*q == ',') q++;
    }
    if (ds.count == 0) ds.count = 1;
  }
  return ds;
}
// Everything before a device is opened: prints why the command line is refused and returns the
// exit code, or 0. The order of the tests decides the message when two things are wrong; the
// numbered steps are pinned by tests/cli_cases.py.
static int ParseCommandLine(int argc, char **argv, Options &o) {
  // 1, 2: the flags whose malformed forms are the reference's line without a newline, exit 1
  if (!TakeCamera(argc, argv, o.cam, o.have_cam)) return Invalid("-camera");
  if (!TakeLevels(argc, argv, "-denoise", o.denoise_levels)) return Invalid("-denoise");
  if (!TakeLevels(argc, argv, "-vdenoise", o.vdenoise_levels) || (o.vdenoise_levels && o.denoise_levels))
    return Invalid("-vdenoise");
  if (const char *bad = TakeRadiance(argc, argv, o)) return Invalid(bad);
  if (o.vdenoise_levels) o.any = true;
  // 3: -layers, and -views / -history, whose malformed forms exit -1
  const char *views_file = nullptr, *history_text = nullptr;
  if (!TakeValue(argc, argv, "-layers", &o.layers_prefix)) return Invalid("-layers");
  if (!TakeValue(argc, argv, "-views", &views_file)) return Fail(-1, "Invalid program argument: -views\n");
  if (!TakeValue(argc, argv, "-history", &history_text)) return Fail(-1, "Invalid program argument: -history\n");
  // 4
  if (o.layers_prefix && (o.adaptive_tile || views_file || o.progressive || o.save_accum || o.load_accum))
    return Fail(1, "-layers takes whole-frame passes of one view: not with -adaptive, -views, -progressive, "
                   "-save_accum or -load_accum\n");
  // 5, 6
  if (history_text && (!ParseInt(history_text, 2, LONG_MAX, &o.history) || !views_file))
    return Fail(-1, "Invalid program argument: -history\n");
  if (views_file)
    if (int rc = TakeViews(views_file, o)) return rc;
  // 7: what is left is the reference's command line
  gi_params_default(&o.P);
  const char *err = nullptr;
  const int rc = gi_parse_args(argc, argv, &o.P, &o.scene, &o.out, &o.w, &o.h, &o.aa, &o.real, &err);
  if (rc == GI_ERR_ARG) return Fail(1, "%s", err);
  if (rc != GI_OK) return Fail(-1, "%s\n", err);
  // 8: what renders on one device
  o.ds = DeviceSet(o.P.gpus);
  if (o.layers_prefix && o.ds.count > 1) return Fail(1, "-layers renders on one device: not with -gpus %d\n", o.ds.count);
  if (o.progressive && o.P.irradiance_cache) return Fail(-1, "Invalid program argument: -progressive (not with -cache)\n");
  if (o.progressive && o.ds.count > 1)
    return Fail(-1, "-progressive renders on one device: not with -gpus %d\n", o.ds.count);
  if (o.any && o.ds.count > 1)
    return Fail(-1, "-passes, -noise, -exposure, -white, -radiance, -vdenoise and -views render on one device: "
                    "not with -gpus %d\n", o.ds.count);
  // 9
  if (o.load_accum) {
    const std::string why = ReadAccum(o.load_accum, o.w, o.h, o.loaded);
    if (!why.empty()) return Fail(-1, "Unable to read -load_accum file %s: %s\n", o.load_accum, why.c_str());
  }
  return 0;
}

// ---- contexts --------------------------------------------------------------------------------
struct DestroyContext { void operator()(gi_ctx *c) const { gi_destroy(c); } };
typedef std::unique_ptr<gi_ctx, DestroyContext> Context;  // the rendering context
// -layers with passes: one scene-less context per layer, destroyed with the object
struct LayerContexts {
  gi_ctx *c[GI_LAYER_COUNT] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  ~LayerContexts() { for (gi_ctx *x : c) if (x) gi_destroy(x); }
};
static int CreateContexts(const Options &o, Context &ctx, LayerContexts &lay) {
  gi_ctx *c = nullptr;
  if (gi_create_devices(&c, &o.ds) != GI_OK)
    return Fail(-1, "Unable to initialise %d HIP device(s) starting at %d\n", o.ds.count, o.ds.devices[0]);
  ctx.reset(c);
  for (int l = 0; o.layers_prefix && o.any && l < GI_LAYER_COUNT; l++)
    if (gi_create(&lay.c[l], o.ds.devices[0]) != GI_OK)
      return Fail(-1, "Unable to initialise HIP device %d\n", o.ds.devices[0]);
  return 0;
}

// ---- the stages ------------------------------------------------------------------------------
// What the stages share. ctx and layers are owned by main.
struct Run {
  const Options &o;
  gi_ctx *ctx;
  gi_ctx *const *layers;
  ProgressState prog;
  // -history: the planes of the last two views, and the previous view's pinhole frame
  std::vector<gi_pixel_features> prev_feat, cur_feat;
  gi_view prev_view;
};
// a library call's outcome; a failure's message is gi_last_error of the rendering context
static bool Ok(const Run &r, int rc) {
  if (rc != GI_OK) fprintf(stderr, "%s\n", gi_last_error(r.ctx));
  return rc == GI_OK;
}
static double SecondsSince(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
static bool ReadSceneAndReport(Run &r) {
  const Options &o = r.o;
  const auto t0 = std::chrono::steady_clock::now();
  if (!Ok(r, gi_read_scene(r.ctx, o.scene, o.real))) return false;
  if (o.have_cam && !Ok(r, gi_set_camera(r.ctx, &o.cam))) return false;
  if (o.P.verbose) {
    int nn = 0, nl = 0;
    gi_scene_info(r.ctx, &nn, &nl, nullptr, nullptr);
    printf("Read scene from %s ...\n", o.scene);
    printf("  Time = %.2f seconds\n", SecondsSince(t0));
    printf("  # Nodes = %d\n", nn);
    printf("  # Lights = %d\n", nl);
    fflush(stdout);
  }
  return true;
}
static bool MapPhotonsAndReport(Run &r) {
  const gi_params &P = r.o.P;
  // -progressive: every pass builds its own maps
  if (r.o.progressive || !(P.indirect_illum || P.caustic_illum || P.direct_photon_illum)) return true;
  gi_photon_stats ps;
  if (!Ok(r, gi_map_photons(r.ctx, &ps))) return false;
  if (r.prog.last[1] >= 0 || r.prog.last[2] >= 0) printf("\n");  // photonmap.cpp:196
  if (P.verbose) {
    printf("Built photon map ...\n");
    printf("  Total Time = %.2f seconds\n", ps.total_s);
    printf("  Photon Tracing = %.2f seconds\n", ps.trace_s);
    printf("  KdTree Construction = %.2f seconds\n", ps.kd_s);
    if (P.irradiance_cache) printf("  Irradiance Cache Computation = %.2f seconds\n", ps.irradiance_s);
    if (P.indirect_illum || P.direct_photon_illum)
      printf("  # Global Photons Stored = %lld\n", (long long)ps.global_stored);
    if (P.caustic_illum) printf("  # Caustic Photons Stored = %lld\n", (long long)ps.caustic_stored);
    printf("Total Photons Stored: %lld\n", (long long)(ps.global_stored + ps.caustic_stored));
    fflush(stdout);
  }
  return true;
}
// one view's outcome: what ReportView prints and WriteView writes
struct ViewResult {
  gi_render_stats rs = {};  // with passes: summed over them
  int passes_done = 0;
  long long primary_samples = 0;
  long long acc_n = 0, acc_total = 0, acc_max = 0;  // the smallest per-pixel count, their sum, the largest
  double acc_noise = 0.0, denoise_ms = 0.0, vdenoise_ms = 0.0;
  bool carried = false;  // -history: the view started from the previous view's accumulator
  gi_reproject_stats rps = {};
  std::vector<uint8_t> rgb;
  std::vector<float> rgbf, mean, layer_means;  // layer_means: GI_LAYER_COUNT + 1 planes
};
static void Add(gi_render_stats &rs, const gi_render_stats &ps) {
  rs.render_s += ps.render_s;
  rs.screen_rays += ps.screen_rays; rs.shadow_rays += ps.shadow_rays;
  rs.monte_carlo_rays += ps.monte_carlo_rays; rs.transmissive_samples += ps.transmissive_samples;
  rs.specular_samples += ps.specular_samples; rs.indirect_samples += ps.indirect_samples;
  rs.caustic_samples += ps.caustic_samples;
}
// The accumulator a view's passes start from: carried from the previous view (-history), the
// -load_accum file's, or empty. least = its smallest per-pixel count.
static bool StartAccumulator(Run &r, int k, ViewResult &v, int64_t &least) {
  const Options &o = r.o;
  if (o.history) {
    // the new view's planes; the previous view's planes and pinhole frame are kept from the step
    // before, and with them the accumulator is carried into this camera instead of emptied
    r.cur_feat.resize((size_t)o.w * o.h);
    if (!Ok(r, gi_camera_features(r.ctx, o.aa, o.w, o.h, r.cur_feat.data()))) return false;
    if (k >= 1) {
      gi_reproject_params rp;
      gi_reproject_params_default(&rp);
      rp.max_history = o.history;
      if (!Ok(r, gi_accum_reproject(r.ctx, &r.prev_view, r.prev_feat.data(), r.cur_feat.data(), &rp, &v.rps, nullptr)) ||
          !Ok(r, gi_accum_get(r.ctx, nullptr, nullptr, &least, nullptr)))
        return false;
      v.carried = true;
    }
  }
  // -load_accum: the run continues the file's: its state, its seeds, and its smallest count, so
  // that the adaptive branch decides as the uninterrupted run would
  if (o.load_accum) {
    if (!Ok(r, gi_accum_import(r.ctx, o.w, o.h, o.loaded.state.data(), o.loaded.counts.data())) ||
        !Ok(r, gi_accum_get(r.ctx, nullptr, nullptr, &least, nullptr)))
      return false;
  } else if (!v.carried && !Ok(r, gi_accum_reset(r.ctx, o.w, o.h))) {
    return false;
  }
  for (int l = 0; o.layers_prefix && l < GI_LAYER_COUNT; l++)
    if (!Ok(r, gi_accum_reset(r.layers[l], o.w, o.h))) return false;
  return true;
}
enum Step { FAILED, STOP, GO };
// Pass i of a view under seed + passes_done + i: progressive, adaptive (ap given), layered or
// plain. STOP: an adaptive pass found every tile at the threshold and rendered nothing.
static Step OnePass(Run &r, int i, const gi_adaptive_params *ap, ViewResult &v, gi_render_stats &ps) {
  const Options &o = r.o;
  const long long frame_samples = ((long long)o.w * o.h) << (2 * o.aa);
  r.prog.last[0] = -1;
  if (o.progressive) {
    // pass index = the seed offset; r_0 from -gd / -cd, photons per pass from -global / -caustic
    const int64_t idx = o.loaded.passes_done + (int64_t)i;
    gi_progressive_params pp;
    gi_progressive_params_default(&pp);
    pp.alpha = o.alpha;
    gi_photon_stats pst;
    if (!Ok(r, gi_set_params(r.ctx, &o.P)) || !Ok(r, gi_accum_add_progressive(r.ctx, o.aa, idx, &pp, &pst, &ps)))
      return FAILED;
    if (o.P.verbose) {
      printf("Progressive pass %lld: -gd %.17g -cd %.17g, %lld global and %lld caustic photons stored\n",
             (long long)idx, gi_progressive_radius(o.P.global_estimate_dist, o.alpha, idx),
             gi_progressive_radius(o.P.caustic_estimate_dist, o.alpha, idx),
             (long long)pst.global_stored, (long long)pst.caustic_stored);
      fflush(stdout);
    }
    v.primary_samples += frame_samples;
    return GO;
  }
  gi_params Pi = o.P;
  Pi.seed = o.P.seed + (uint64_t)o.loaded.passes_done + (uint64_t)i;
  if (!Ok(r, gi_set_params(r.ctx, &Pi))) return FAILED;
  if (ap) {
    int64_t active = 0;
    if (!Ok(r, gi_accum_add_adaptive(r.ctx, o.aa, ap, nullptr, &active, &ps))) return FAILED;
    if (active == 0) return STOP;
    v.primary_samples += (long long)active << (2 * o.aa);
    return GO;
  }
  if (!Ok(r, o.layers_prefix ? gi_accum_add_image_layers(r.ctx, o.aa, r.layers, &ps)
                             : gi_accum_add_image(r.ctx, o.aa, &ps)))
    return FAILED;
  v.primary_samples += frame_samples;
  return GO;
}
// After a pass: -adaptive takes the new smallest count, -noise T stops at noise <= T
static Step AfterPass(Run &r, ViewResult &v, int64_t &least) {
  const Options &o = r.o;
  if (o.adaptive_tile) return Ok(r, gi_accum_get(r.ctx, nullptr, nullptr, &least, nullptr)) ? GO : FAILED;
  if (!o.have_noise) return GO;
  int64_t n = 0;  // the noise is defined from two samples per pixel on
  if (!Ok(r, gi_accum_get(r.ctx, nullptr, nullptr, &n, &v.acc_noise))) return FAILED;
  return n >= 2 && v.acc_noise <= o.noise ? STOP : GO;
}
// -save_accum: the accumulator as the pass loop leaves it
static bool SaveAccumulator(Run &r, const ViewResult &v) {
  const Options &o = r.o;
  AccumFile a;
  a.state.resize((size_t)o.w * o.h * 6);
  a.counts.resize((size_t)o.w * o.h);
  a.passes_done = o.loaded.passes_done + v.passes_done;
  if (!Ok(r, gi_accum_export(r.ctx, a.state.data(), a.counts.data()))) return false;
  if (WriteAccum(o.save_accum, o.w, o.h, a)) return true;
  fprintf(stderr, "Unable to write -save_accum file %s\n", o.save_accum);
  return false;
}
// -vdenoise: filtered = the accumulator's mean filtered under its variance; with -layers every
// layer but the specular one filtered under its own, and their sum
static bool FilterAccumulator(Run &r, ViewResult &v, std::vector<float> &filtered) {
  const Options &o = r.o;
  std::vector<gi_pixel_features> feat;  // -history has this view's planes already
  if (!o.history) {
    feat.resize((size_t)o.w * o.h);
    if (!Ok(r, gi_camera_features(r.ctx, o.aa, o.w, o.h, feat.data()))) return false;
  }
  gi_vdenoise_params vp;
  gi_vdenoise_params_default(&vp);
  vp.levels = o.vdenoise_levels;
  filtered.resize((size_t)o.w * o.h * 3);
  if (!o.layers_prefix)
    return Ok(r, gi_accum_denoise(r.ctx, o.history ? r.cur_feat.data() : feat.data(), &vp, filtered.data(), nullptr,
                                  &v.vdenoise_ms));
  // per channel the five floats widened to double, added in layer order, rounded once
  std::vector<double> sum(filtered.size(), 0.0);
  std::vector<float> part(filtered.size());
  for (int l = 0; l < GI_LAYER_COUNT; l++) {
    double ms = 0.0;
    const int rc = l == GI_LAYER_SPECULAR ? gi_accum_get(r.layers[l], part.data(), nullptr, nullptr, nullptr)
                                          : gi_accum_denoise(r.layers[l], feat.data(), &vp, part.data(), nullptr, &ms);
    if (rc != GI_OK) fprintf(stderr, "%s\n", gi_last_error(r.layers[l]));  // the layer context's, then ctx's
    if (!Ok(r, rc)) return false;
    v.vdenoise_ms += ms;
    for (size_t i = 0; i < sum.size(); i++) sum[i] += (double)part[i];
  }
  for (size_t i = 0; i < sum.size(); i++) filtered[i] = (float)sum[i];
  return true;
}
// A view with a radiance flag: passes folded into the accumulator, then its tone-mapped mean.
// The passes leave their own seed in the context's parameters; RenderView restores them.
static bool RenderPasses(Run &r, int k, ViewResult &v) {
  const Options &o = r.o;
  int64_t least = 0;  // the smallest per-pixel count so far
  if (!StartAccumulator(r, k, v, least)) return false;
  gi_adaptive_params ap;
  gi_adaptive_params_default(&ap);
  ap.tile_px = o.adaptive_tile ? o.adaptive_tile : ap.tile_px;
  ap.threshold = o.noise;
  for (int i = 0; i < o.passes; i++) {
    // a carried accumulator goes straight to adaptive passes: the selection's n_min < min_samples
    // rule makes the tiles whose history was lost core
    const bool adaptive = o.adaptive_tile && (v.carried || least >= ap.min_samples);
    gi_render_stats ps;
    Step s = OnePass(r, i, adaptive ? &ap : nullptr, v, ps);
    if (s == GO) {
      v.passes_done++;
      Add(v.rs, ps);
      s = AfterPass(r, v, least);
    }
    if (s == FAILED) return false;
    if (s == STOP) break;
  }
  if (o.adaptive_tile) {
    std::vector<int64_t> counts((size_t)o.w * o.h);
    int64_t total = 0;
    if (!Ok(r, gi_accum_get_counts(r.ctx, counts.data(), &total))) return false;
    v.acc_total = total;
    for (int64_t n : counts) v.acc_max = n > v.acc_max ? n : v.acc_max;
  }
  if (o.save_accum && !SaveAccumulator(r, v)) return false;
  int64_t n = 0;
  if (!Ok(r, gi_accum_get(r.ctx, v.mean.data(), nullptr, &n, &v.acc_noise))) return false;
  v.acc_n = n;
  std::vector<float> filtered;  // -vdenoise: the written image is the tone-mapped filtered mean
  if (o.vdenoise_levels && !FilterAccumulator(r, v, filtered)) return false;
  for (int l = 0; o.layers_prefix && l < GI_LAYER_COUNT; l++)
    if (!Ok(r, gi_accum_get(r.layers[l], v.layer_means.data() + (size_t)l * o.w * o.h * 3, nullptr, nullptr, nullptr)))
      return false;
  return Ok(r, gi_tonemap(r.ctx, o.w, o.h, o.vdenoise_levels ? filtered.data() : v.mean.data(), o.exposure, o.white,
                          v.rgbf.data(), v.rgb.data()));
}
// A view without one: the reference's RenderImage
static bool RenderFrame(Run &r, ViewResult &v) {
  const Options &o = r.o;
  if (!Ok(r, gi_render_image(r.ctx, o.aa, o.w, o.h, v.rgb.data(), o.denoise_levels ? v.rgbf.data() : nullptr, &v.rs)))
    return false;
  // -layers: the frame once more, split (the image is gi_render_image's own)
  return !o.layers_prefix ||
         Ok(r, gi_render_layers(r.ctx, o.aa, o.w, o.h, v.layer_means.data(), nullptr, nullptr, nullptr));
}
// -denoise: the written image is the filtered frame
static bool DenoiseFrame(Run &r, ViewResult &v) {
  const Options &o = r.o;
  std::vector<gi_pixel_features> feat((size_t)o.w * o.h);
  gi_denoise_params dp;
  gi_denoise_params_default(&dp);
  dp.levels = o.denoise_levels;
  return Ok(r, gi_camera_features(r.ctx, o.aa, o.w, o.h, feat.data())) &&
         Ok(r, gi_denoise(r.ctx, o.w, o.h, v.rgbf.data(), feat.data(), &dp, nullptr, v.rgb.data(), &v.denoise_ms));
}
static bool RenderView(Run &r, int k, ViewResult &v) {
  const Options &o = r.o;
  const size_t n3 = (size_t)o.w * o.h * 3;
  if (!o.views.empty() && !Ok(r, gi_set_camera(r.ctx, &o.views[k]))) return false;
  if (o.P.verbose) printf("Rendering image ...\n");
  v.rgb.resize(n3);
  v.rgbf.resize(o.denoise_levels || o.any ? n3 : 0);
  v.mean.resize(o.any ? n3 : 0);
  v.layer_means.resize(o.layers_prefix ? (GI_LAYER_COUNT + 1) * n3 : 0);
  if (o.any) {
    const bool ok = RenderPasses(r, k, v);
    gi_set_params(r.ctx, &o.P);
    if (!ok) return false;
    if (o.history) {  // this view is the next one's previous view
      if (!Ok(r, gi_get_view(r.ctx, &r.prev_view))) return false;
      r.prev_feat.swap(r.cur_feat);
    }
  } else if (!RenderFrame(r, v)) {
    return false;
  }
  if (o.denoise_levels && !DenoiseFrame(r, v)) return false;
  PrintProgress(1.0, PROGRESS_BAR_WIDTH);  // render.cpp:201-202
  printf("\n");
  fflush(stdout);
  return true;
}
static void ReportView(const Options &o, int k, const ViewResult &v) {
  const gi_params &P = o.P;
  const gi_render_stats &rs = v.rs;
  unsigned long long total = rs.screen_rays;
  printf("Rendered image ...\n");
  printf("  Time = %.2f seconds\n", rs.render_s);
  printf("  # Screen Rays = %llu\n", (unsigned long long)rs.screen_rays);
  if (P.shadows) { printf("  # Shadow Rays = %llu\n", (unsigned long long)rs.shadow_rays); total += rs.shadow_rays; }
  if (P.monte_carlo) { printf("  # Monte Carlo Rays = %llu\n", (unsigned long long)rs.monte_carlo_rays); total += rs.monte_carlo_rays; }
  if (P.transmissive_illum) { printf("  # Transmissive Samples = %llu\n", (unsigned long long)rs.transmissive_samples); total += rs.transmissive_samples; }
  if (P.specular_illum) { printf("  # Specular Samples = %llu\n", (unsigned long long)rs.specular_samples); total += rs.specular_samples; }
  if (P.indirect_illum) { printf("  # Indirect Samples = %llu\n", (unsigned long long)rs.indirect_samples); total += rs.indirect_samples; }
  if (P.caustic_illum) { printf("  # Caustic Samples = %llu\n", (unsigned long long)rs.caustic_samples); total += rs.caustic_samples; }
  printf("Total Rays: %llu\n", total);
  if (!o.views.empty())
    printf("View %d of %d: %lld primary samples rendered\n", k, (int)o.views.size(), v.primary_samples);
  if (v.carried)
    printf("Reprojected history: %lld pixels kept, %lld pixels reset, %lld samples kept\n",
           (long long)v.rps.kept_pixels, (long long)v.rps.reset_pixels, (long long)v.rps.kept_samples);
  if (o.adaptive_tile)
    printf("Accumulated image: %d passes, %lld samples, %lld to %lld per pixel, noise = %.6g\n",
           v.passes_done, v.acc_total, v.acc_n, v.acc_max, v.acc_noise);
  else if (o.any)
    printf("Accumulated image: %d passes, N = %lld samples per pixel, noise = %.6g\n", v.passes_done,
           v.acc_n, v.acc_noise);
  if (o.denoise_levels) printf("Denoised image: %d levels, %.3f ms\n", o.denoise_levels, v.denoise_ms);
  if (o.vdenoise_levels)
    printf("Variance-guided denoise: %d levels, %.3f ms\n", o.vdenoise_levels, v.vdenoise_ms);
  fflush(stdout);
}
static const char *const LAYER_SUFFIX[GI_LAYER_COUNT] = {"_surface.pfm", "_specular.pfm", "_indirect.pfm",
                                                        "_global.pfm", "_caustic.pfm"};
// path with ".%04d" of k before its extension (appended when it has none)
static std::string NumberedPath(const char *path, int k) {
  std::string p(path);
  char num[16];
  snprintf(num, sizeof num, ".%04d", k);
  const size_t slash = p.find_last_of('/');
  const size_t dot = p.find_last_of('.');
  if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return p + num;
  return p.substr(0, dot) + num + p.substr(dot);
}
// The image, the -radiance file and the -layers files of view k. Uses no context.
static bool WriteView(const Options &o, int k, const ViewResult &v) {
  const bool numbered = !o.views.empty();
  const std::string out_k = numbered ? NumberedPath(o.out, k) : std::string(o.out);
  const auto tw = std::chrono::steady_clock::now();
  if (gi_write_image(out_k.c_str(), o.w, o.h, v.rgb.data()) != GI_OK) {
    const char *ext = strrchr(o.out, '.');
    if (ext && !strncmp(ext, ".tif", 4)) fprintf(stderr, "TIFF not supported\n");  // R2Image.cpp:1300
    else fprintf(stderr, "Unable to write image %s\n", out_k.c_str());
    return false;
  }
  std::vector<std::pair<std::string, const float *>> floats;  // the float frames, in the order written
  if (o.radiance_file)
    floats.push_back({numbered ? NumberedPath(o.radiance_file, k) : std::string(o.radiance_file), v.mean.data()});
  for (int l = 0; o.layers_prefix && l < GI_LAYER_COUNT; l++)
    floats.push_back({std::string(o.layers_prefix) + LAYER_SUFFIX[l], v.layer_means.data() + (size_t)l * o.w * o.h * 3});
  for (const auto &f : floats)
    if (gi_write_image_float(f.first.c_str(), o.w, o.h, f.second) != GI_OK) {
      fprintf(stderr, "Unable to write image %s\n", f.first.c_str());
      return false;
    }
  if (o.P.verbose) {
    printf("Wrote image to %s ...\n", out_k.c_str());
    printf("  Time = %.2f seconds\n", SecondsSince(tw));
    printf("  Width = %d\n", o.w);
    printf("  Height = %d\n", o.h);
    fflush(stdout);
  }
  return true;
}

int main(int argc, char **argv) {
  Options o;
  if (int rc = ParseCommandLine(argc, argv, o)) return rc;
  // destroyed in reverse order: the rendering context first, then the layer contexts
  LayerContexts lay;
  Context ctx;
  if (int rc = CreateContexts(o, ctx, lay)) return rc;
  Run r = {o, ctx.get(), lay.c, {o.P.verbose != 0, {-1, -1, -1}}, {}, {}, {}};
  gi_set_params(r.ctx, &o.P);
  gi_set_progress(r.ctx, OnProgress, &r.prog);
  if (!ReadSceneAndReport(r) || !MapPhotonsAndReport(r)) return -1;
  const int nviews = o.views.empty() ? 1 : (int)o.views.size();
  for (int k = 0; k < nviews; k++) {
    ViewResult v;
    if (!RenderView(r, k, v)) return -1;
    if (o.P.verbose) ReportView(o, k, v);
    // the last view's files are written with the device released (the reference's renderer is
    // gone when WriteImage runs); nothing below uses r.ctx
    if (k == nviews - 1) ctx.reset();
    if (!WriteView(o, k, v)) return -1;
  }
  return 0;
}
