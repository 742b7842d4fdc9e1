// photonmap.cpp -- drop-in CLI: `photonmap src.scn out.png [-FLAGS]` on the MI355X path.
//
// Same control flow and reports as the reference main (photonmap.cpp:442-499):
// ParseArgs -> ReadScene -> MapPhotons (if indirect|caustic|photon_viz) -> RenderImage ->
// WriteImage, with the -v statistics of io_utils.cpp:240-246, photonmap.cpp:416-435 and
// render.cpp:224-255. Exit codes: 1 for a bad flag, -1 (255) for load/render/write failures.
// Extension: -camera ex ey ez tx ty tz ux uy uz xfov renders from that camera instead of the
// scene file's (gi_set_camera; the numbers of the .scn `camera` command).
// Extension: -denoise L writes the frame filtered by L (1..8) levels of the edge-avoiding
// a-trous pass over its feature planes (gi_camera_features + gi_denoise, default parameters).
// Extension: -passes N (1..4096), -noise T, -exposure E, -white W, -radiance FILE. With any of
// them the maps are built once, pass i is rendered under seed + i and folded into the context's
// accumulator (gi_accum_*), after each pass -noise stops at noise <= T (default passes: 1, or
// 4096 under -noise), the written image is gi_tonemap of the unclamped mean (E default 1, W
// default 0: linear) and FILE (.pfm / .hdr) receives that mean. One device only.
// Extension: -adaptive [TILE] (TILE 4..64, default 8), only together with -noise T: whole-frame
// passes until every pixel has the default min_samples, then gi_accum_add_adaptive passes with
// threshold T over TILE x TILE tiles, until no tile is active or -passes is used up.
// Extension: -vdenoise L (1..8, not with -denoise): counts as one of the radiance flags; after the
// passes the accumulator is filtered by L levels of the variance-guided pass over its feature
// planes (gi_camera_features + gi_accum_denoise, other parameters default) and the written image
// is gi_tonemap of the filtered mean. -radiance FILE still receives the unfiltered mean.
// Extension: -views FILE (one of the radiance flags; not with -denoise): FILE holds one camera per
// line, ten numbers as in -camera (blank lines and # lines skipped). The maps are built once; view
// k gets gi_set_camera and the pass loop above, and its image (and -radiance file) is written with
// .%04d of k before the extension. -history H (H >= 2, only with -views): from the second view on
// the accumulator is not emptied but carried into the new camera (gi_camera_features +
// gi_accum_reproject with max_history = H); with -adaptive the view then goes straight to adaptive
// passes, which refine the tiles whose history was lost.
// Extension: -save_accum FILE, -load_accum FILE (radiance flags; not with -views): -save_accum
// writes the accumulator's fp64 state as the pass loop leaves it (gi_accum_export; the file:
// AccumFile below) with the number of pass-loop iterations behind it. -load_accum starts from
// such a file instead of an empty accumulator (gi_accum_import): pass i runs under seed +
// passes_done + i, -passes N means N more passes, and a saved file counts the loaded passes too,
// so an interrupted run that is resumed ends with the bits of the uninterrupted one. A file that is
// missing, short or long, of another magic or size than -resolution, or holds a negative count exits
// -1. -noise T is tested after a pass, as without a file: a resumed run renders at least one pass,
// also when the loaded state is already at T (the uninterrupted run would have stopped there, and
// its file would not have been resumed).
// Extension: -progressive A (A in (0, 1); a radiance flag, with -passes / -noise): progressive
// photon mapping. No maps are built up front; pass i is gi_accum_add_progressive with the index
// passes_done + i: fresh maps of -global / -caustic photons under seed + index, fixed-radius
// estimates whose radii shrink from -gd / -cd by the schedule of gi_progressive_radius. Refused
// before a device is opened with -adaptive, -views, -cache or -gpus N. The accumulator file does
// not record the flag: a resumed run must be given the same -progressive A.
// Extension: -layers PREFIX: the frame's light-path layers (gi.h GI_LAYER_*) as float means in
// PREFIX_surface.pfm, _specular, _indirect, _global and _caustic. Without a radiance flag the
// frame is rendered once more by gi_render_layers for them; with one, every pass is a layered one
// (gi_accum_add_image_layers) over five scene-less contexts. The usual image and -radiance come
// from the total and do not change. With -vdenoise L the surface, indirect, global and caustic
// layers are each filtered under their own variance (gi_accum_denoise of the layer's context, the
// frame's planes), the specular layer is left as it is, and the written image is gi_tonemap of
// their sum (per channel the five floats widened to double, added in layer order, rounded once):
// what a mirror or glass shows is not filtered by the planes of the surface that shows it.
// Refused (exit 1) with -adaptive, -views, -progressive, -save_accum, -load_accum or -gpus N.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

// Takes `-camera` and its ten numbers out of argv (gi_parse_args keeps the reference's flag
// set); false on fewer than ten numbers or a non-number. The last -camera wins.
static bool TakeCamera(int &argc, char **argv, gi_camera &cam, bool &have) {
  for (int a = 1; a < argc;) {
    if (strcmp(argv[a], "-camera")) { a++; continue; }
    double v[10];
    for (int k = 0; k < 10; k++) {
      if (a + 1 + k >= argc) return false;
      char *end = nullptr;
      v[k] = strtod(argv[a + 1 + k], &end);
      if (end == argv[a + 1 + k] || *end) return false;
    }
    for (int i = 0; i < 3; i++) { cam.eye[i] = v[i]; cam.towards[i] = v[3 + i]; cam.up[i] = v[6 + i]; }
    cam.xfov = v[9];
    have = true;
    for (int k = a + 11; k < argc; k++) argv[k - 11] = argv[k];
    argc -= 11;
  }
  return true;
}

// Takes `-denoise L` (or `-vdenoise L`: flag) out of argv in the same way; false on a missing,
// non-integer or out-of-range (1..8) L. The last one wins.
static bool TakeDenoise(int &argc, char **argv, int &levels, const char *flag = "-denoise") {
  for (int a = 1; a < argc;) {
    if (strcmp(argv[a], flag)) { a++; continue; }
    if (a + 1 >= argc) return false;
    char *end = nullptr;
    const long v = strtol(argv[a + 1], &end, 10);
    if (end == argv[a + 1] || *end || v < 1 || v > 8) return false;
    levels = (int)v;
    for (int k = a + 2; k < argc; k++) argv[k - 2] = argv[k];
    argc -= 2;
  }
  return true;
}

// Takes `flag value` out of argv in the same way: *value = the last one's text (null when the
// flag is absent); false when the flag is last in argv.
static bool TakeValue(int &argc, char **argv, const char *flag, const char **value) {
  for (int a = 1; a < argc;) {
    if (strcmp(argv[a], flag)) { a++; continue; }
    if (a + 1 >= argc) return false;
    *value = argv[a + 1];
    for (int k = a + 2; k < argc; k++) argv[k - 2] = argv[k];
    argc -= 2;
  }
  return true;
}
static bool ParseNumber(const char *text, double *v) {
  char *end = nullptr;
  *v = strtod(text, &end);
  return end != text && !*end && *v == *v && *v - *v == 0.0;  // a finite number, nothing after it
}

// Takes `-adaptive [TILE]` out of argv: the token after it is TILE when it is an integer (false
// when that is outside 4..64). The last -adaptive wins.
static bool TakeAdaptive(int &argc, char **argv, int &tile) {
  for (int a = 1; a < argc;) {
    if (strcmp(argv[a], "-adaptive")) { a++; continue; }
    int take = 1;
    tile = 8;
    if (a + 1 < argc) {
      char *end = nullptr;
      const long v = strtol(argv[a + 1], &end, 10);
      if (end != argv[a + 1] && !*end) {
        if (v < 4 || v > 64) return false;
        tile = (int)v;
        take = 2;
      }
    }
    for (int k = a + take; k < argc; k++) argv[k - take] = argv[k];
    argc -= take;
  }
  return true;
}

// -passes / -noise / -exposure / -white / -radiance / -adaptive
struct RadianceFlags {
  bool any = false, have_noise = false;
  int adaptive_tile = 0;  // 0: uniform passes
  int passes = 0;  // 0: not given
  double noise = 0.0, exposure = 1.0, white = 0.0;
  const char *file = nullptr;
  const char *save_accum = nullptr, *load_accum = nullptr;
  bool progressive = false;  // -progressive A: fresh photon maps and a shrinking fixed radius per pass
  double alpha = 0.0;
};
// null, or the flag that is malformed
static const char *TakeRadiance(int &argc, char **argv, RadianceFlags &r) {
  const char *t = nullptr;
  double v = 0.0;
  if (!TakeAdaptive(argc, argv, r.adaptive_tile)) return "-adaptive";
  if (!TakeValue(argc, argv, "-passes", &t)) return "-passes";
  if (t) {
    char *end = nullptr;
    const long n = strtol(t, &end, 10);
    if (end == t || *end || n < 1 || n > 4096) return "-passes";
    r.passes = (int)n;
    r.any = true;
  }
  t = nullptr;
  if (!TakeValue(argc, argv, "-noise", &t)) return "-noise";
  if (t) {
    if (!ParseNumber(t, &v) || v < 0.0) return "-noise";
    r.noise = v;
    r.have_noise = r.any = true;
  }
  t = nullptr;
  if (!TakeValue(argc, argv, "-exposure", &t)) return "-exposure";
  if (t) {
    if (!ParseNumber(t, &v) || !(v > 0.0)) return "-exposure";
    r.exposure = v;
    r.any = true;
  }
  t = nullptr;
  if (!TakeValue(argc, argv, "-white", &t)) return "-white";
  if (t) {
    if (!ParseNumber(t, &v) || v < 0.0) return "-white";
    r.white = v;
    r.any = true;
  }
  t = nullptr;
  if (!TakeValue(argc, argv, "-radiance", &t)) return "-radiance";
  if (t) {
    const char *ext = strrchr(t, '.');
    if (!ext || (strcmp(ext, ".pfm") && strcmp(ext, ".hdr"))) return "-radiance";
    r.file = t;
    r.any = true;
  }
  if (!TakeValue(argc, argv, "-save_accum", &r.save_accum)) return "-save_accum";
  if (!TakeValue(argc, argv, "-load_accum", &r.load_accum)) return "-load_accum";
  if (r.save_accum || r.load_accum) r.any = true;
  t = nullptr;
  if (!TakeValue(argc, argv, "-progressive", &t)) return "-progressive";
  if (t) {
    if (!ParseNumber(t, &v) || !(v > 0.0 && v < 1.0)) return "-progressive";
    if (r.adaptive_tile) return "-progressive (not with -adaptive)";
    r.alpha = v;
    r.progressive = r.any = true;
  }
  if (r.adaptive_tile && !r.have_noise) return "-adaptive";
  if (r.passes == 0) r.passes = r.have_noise ? 4096 : 1;
  return nullptr;
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
    else
      for (int64_t n : a.counts)
        if (n < 0) {
          why = "negative sample count";
          break;
        }
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
    gi_camera cam;
    for (int i = 0; i < 3; i++) { cam.eye[i] = v[i]; cam.towards[i] = v[3 + i]; cam.up[i] = v[6 + i]; }
    cam.xfov = v[9];
    views.push_back(cam);
  }
  fclose(f);
  return true;
}

static const char *const LAYER_SUFFIX[GI_LAYER_COUNT] = {"_surface.pfm", "_specular.pfm", "_indirect.pfm",
                                                        "_global.pfm", "_caustic.pfm"};
// -layers with passes: one scene-less context per layer, destroyed with the object
struct LayerContexts {
  gi_ctx *c[GI_LAYER_COUNT] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  ~LayerContexts() {
    for (gi_ctx *x : c)
      if (x) gi_destroy(x);
  }
};
// plane l of means (GI_LAYER_COUNT planes of w * h * 3 floats) to PREFIX + its suffix
static bool WriteLayers(const char *prefix, int w, int h, const std::vector<float> &means) {
  for (int l = 0; l < GI_LAYER_COUNT; l++) {
    const std::string path = std::string(prefix) + LAYER_SUFFIX[l];
    if (gi_write_image_float(path.c_str(), w, h, means.data() + (size_t)l * w * h * 3) != GI_OK) {
      fprintf(stderr, "Unable to write image %s\n", path.c_str());
      return false;
    }
  }
  return true;
}

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

int main(int argc, char **argv) {
  gi_camera cam;
  bool have_cam = false;
  if (!TakeCamera(argc, argv, cam, have_cam)) {
    fprintf(stderr, "Invalid program argument: -camera");
    return 1;
  }
  int denoise_levels = 0;  // 0: no denoise pass
  if (!TakeDenoise(argc, argv, denoise_levels)) {
    fprintf(stderr, "Invalid program argument: -denoise");
    return 1;
  }
  int vdenoise_levels = 0;  // 0: no variance-guided denoise pass
  if (!TakeDenoise(argc, argv, vdenoise_levels, "-vdenoise") || (vdenoise_levels && denoise_levels)) {
    fprintf(stderr, "Invalid program argument: -vdenoise");
    return 1;
  }
  RadianceFlags rad;
  if (const char *bad = TakeRadiance(argc, argv, rad)) {
    fprintf(stderr, "Invalid program argument: %s", bad);
    return 1;
  }
  if (vdenoise_levels) rad.any = true;
  const char *layers_prefix = nullptr;
  if (!TakeValue(argc, argv, "-layers", &layers_prefix)) {
    fprintf(stderr, "Invalid program argument: -layers");
    return 1;
  }
  // -views FILE / -history H: one of the radiance flags; malformed ones exit -1
  const char *views_file = nullptr, *history_text = nullptr;
  std::vector<gi_camera> views;
  long history = 0;  // 0: every view starts from an empty accumulator
  if (!TakeValue(argc, argv, "-views", &views_file)) {
    fprintf(stderr, "Invalid program argument: -views\n");
    return -1;
  }
  if (!TakeValue(argc, argv, "-history", &history_text)) {
    fprintf(stderr, "Invalid program argument: -history\n");
    return -1;
  }
  if (layers_prefix && (rad.adaptive_tile || views_file || rad.progressive || rad.save_accum || rad.load_accum)) {
    fprintf(stderr, "-layers takes whole-frame passes of one view: not with -adaptive, -views, -progressive, "
                    "-save_accum or -load_accum\n");
    return 1;
  }
  if (history_text) {
    char *end = nullptr;
    history = strtol(history_text, &end, 10);
    if (end == history_text || *end || history < 2 || !views_file) {
      fprintf(stderr, "Invalid program argument: -history\n");
      return -1;
    }
  }
  if (views_file && (rad.save_accum || rad.load_accum)) {
    fprintf(stderr, "Invalid program argument: -views (not with -save_accum or -load_accum)\n");
    return -1;
  }
  if (views_file && rad.progressive) {
    fprintf(stderr, "Invalid program argument: -progressive (not with -views)\n");
    return -1;
  }
  if (views_file) {
    if (denoise_levels) {
      fprintf(stderr, "Invalid program argument: -views (not with -denoise)\n");
      return -1;
    }
    int bad_line = 0;
    if (!ReadViews(views_file, views, bad_line)) {
      if (bad_line) fprintf(stderr, "Unable to read views file %s: line %d is not ten numbers\n", views_file, bad_line);
      else fprintf(stderr, "Unable to open views file %s\n", views_file);
      return -1;
    }
    if (views.empty()) {
      fprintf(stderr, "Unable to read views file %s: no camera in it\n", views_file);
      return -1;
    }
    rad.any = true;
  }
  gi_params P;
  gi_params_default(&P);
  const char *scene = nullptr, *out = nullptr, *err = nullptr;
  int w = 1024, h = 1024, aa = 2, real = 0;
  int rc = gi_parse_args(argc, argv, &P, &scene, &out, &w, &h, &aa, &real, &err);
  if (rc == GI_ERR_ARG) {
    fprintf(stderr, "%s", err);
    return 1;
  }
  if (rc != GI_OK) {
    fprintf(stderr, "%s\n", err);
    return -1;
  }
  // devices: -gpus N takes devices 0..N-1 (the reference's -threads N re-cut as a device
  // shard); GI_DEVICES="a,b,..." names them explicitly, GI_DEVICE the single device
  gi_device_set ds;
  memset(&ds, 0, sizeof ds);
  ds.count = 1;
  if (const char *d = getenv("GI_DEVICE")) ds.devices[0] = atoi(d);
  if (P.gpus > 1) {
    ds.count = P.gpus < GI_MAX_DEVICES ? P.gpus : GI_MAX_DEVICES;
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
  if (layers_prefix && ds.count > 1) {
    fprintf(stderr, "-layers renders on one device: not with -gpus %d\n", ds.count);
    return 1;
  }
  if (rad.progressive && P.irradiance_cache) {
    fprintf(stderr, "Invalid program argument: -progressive (not with -cache)\n");
    return -1;
  }
  if (rad.progressive && ds.count > 1) {
    fprintf(stderr, "-progressive renders on one device: not with -gpus %d\n", ds.count);
    return -1;
  }
  if (rad.any && ds.count > 1) {
    fprintf(stderr, "-passes, -noise, -exposure, -white, -radiance, -vdenoise and -views render on one device: not with -gpus %d\n",
            ds.count);
    return -1;
  }
  AccumFile loaded;  // -load_accum: checked before a device is opened
  if (rad.load_accum) {
    const std::string why = ReadAccum(rad.load_accum, w, h, loaded);
    if (!why.empty()) {
      fprintf(stderr, "Unable to read -load_accum file %s: %s\n", rad.load_accum, why.c_str());
      return -1;
    }
  }
  gi_ctx *ctx = nullptr;
  if (gi_create_devices(&ctx, &ds) != GI_OK) {
    fprintf(stderr, "Unable to initialise %d HIP device(s) starting at %d\n", ds.count, ds.devices[0]);
    return -1;
  }
  LayerContexts lay;
  std::vector<float> layer_means(layers_prefix ? (size_t)(GI_LAYER_COUNT + 1) * w * h * 3 : 0);
  if (layers_prefix && rad.any)
    for (int l = 0; l < GI_LAYER_COUNT; l++)
      if (gi_create(&lay.c[l], ds.devices[0]) != GI_OK) {
        fprintf(stderr, "Unable to initialise HIP device %d\n", ds.devices[0]);
        gi_destroy(ctx);
        return -1;
      }
  gi_set_params(ctx, &P);
  ProgressState prog = {P.verbose != 0, {-1, -1, -1}};
  gi_set_progress(ctx, OnProgress, &prog);
  auto t0 = std::chrono::steady_clock::now();
  if (gi_read_scene(ctx, scene, real) != GI_OK) {
    fprintf(stderr, "%s\n", gi_last_error(ctx));
    gi_destroy(ctx);
    return -1;
  }
  if (have_cam && gi_set_camera(ctx, &cam) != GI_OK) {
    fprintf(stderr, "%s\n", gi_last_error(ctx));
    gi_destroy(ctx);
    return -1;
  }
  if (P.verbose) {
    int nn = 0, nl = 0;
    gi_scene_info(ctx, &nn, &nl, nullptr, nullptr);
    printf("Read scene from %s ...\n", scene);
    printf("  Time = %.2f seconds\n",
           std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    printf("  # Nodes = %d\n", nn);
    printf("  # Lights = %d\n", nl);
    fflush(stdout);
  }
  // -progressive: every pass builds its own maps
  if (!rad.progressive && (P.indirect_illum || P.caustic_illum || P.direct_photon_illum)) {
    gi_photon_stats ps;
    if (gi_map_photons(ctx, &ps) != GI_OK) {
      fprintf(stderr, "%s\n", gi_last_error(ctx));
      gi_destroy(ctx);
      return -1;
    }
    if (prog.last[1] >= 0 || prog.last[2] >= 0) printf("\n");  // photonmap.cpp:196
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
  }
  const int nviews = views.empty() ? 1 : (int)views.size();
  std::vector<gi_pixel_features> prev_feat, cur_feat;  // -history: the planes of the last two views
  gi_view prev_view;
  memset(&prev_view, 0, sizeof prev_view);
  for (int k = 0; k < nviews; k++) {
    const std::string out_k = views.empty() ? std::string(out) : NumberedPath(out, k);
    const std::string rad_k = !rad.file ? std::string() : (views.empty() ? std::string(rad.file) : NumberedPath(rad.file, k));
    if (!views.empty() && gi_set_camera(ctx, &views[k]) != GI_OK) {
      fprintf(stderr, "%s\n", gi_last_error(ctx));
      gi_destroy(ctx);
      return -1;
    }
    std::vector<uint8_t> rgb((size_t)w * h * 3);
    gi_render_stats rs;
    if (P.verbose) printf("Rendering image ...\n");
    std::vector<float> rgbf(denoise_levels || rad.any ? (size_t)w * h * 3 : 0);
    std::vector<float> mean(rad.any ? (size_t)w * h * 3 : 0);
    int passes_done = 0;
    long long acc_n = 0, acc_total = 0, acc_max = 0, primary_samples = 0;
    double acc_noise = 0.0, vdenoise_ms = 0.0;
    bool carried = false;  // -history: this view starts from the previous view's accumulator
    gi_reproject_stats rps;
    memset(&rps, 0, sizeof rps);
    if (rad.any) {
      // passes under seed, seed + 1, ... from the same maps, folded into the accumulator; the
      // written image is the tone-mapped unclamped mean
      memset(&rs, 0, sizeof rs);
      bool ok = true;
      int64_t least = 0;  // the smallest per-pixel count so far
      if (history) {
        // the new view's planes; the previous view's planes and pinhole frame are kept from the step
        // before, and with them the accumulator is carried into this camera instead of emptied
        cur_feat.resize((size_t)w * h);
        ok = gi_camera_features(ctx, aa, w, h, cur_feat.data()) == GI_OK;
        if (ok && k >= 1) {
          gi_reproject_params rp;
          gi_reproject_params_default(&rp);
          rp.max_history = history;
          ok = gi_accum_reproject(ctx, &prev_view, prev_feat.data(), cur_feat.data(), &rp, &rps, nullptr) == GI_OK &&
               gi_accum_get(ctx, nullptr, nullptr, &least, nullptr) == GI_OK;
          carried = ok;
        }
      }
      // -load_accum: the run continues the file's: its state, its seeds, and its smallest count, so
      // that the adaptive branch decides as the uninterrupted run would
      if (ok && rad.load_accum)
        ok = gi_accum_import(ctx, w, h, loaded.state.data(), loaded.counts.data()) == GI_OK &&
             gi_accum_get(ctx, nullptr, nullptr, &least, nullptr) == GI_OK;
      else if (ok && !carried) ok = gi_accum_reset(ctx, w, h) == GI_OK;
      for (int l = 0; ok && layers_prefix && l < GI_LAYER_COUNT; l++) ok = gi_accum_reset(lay.c[l], w, h) == GI_OK;
      gi_adaptive_params ap;
      gi_adaptive_params_default(&ap);
      ap.tile_px = rad.adaptive_tile ? rad.adaptive_tile : ap.tile_px;
      ap.threshold = rad.noise;
      for (int i = 0; ok && i < rad.passes; i++) {
        gi_params Pi = P;
        Pi.seed = P.seed + (uint64_t)loaded.passes_done + (uint64_t)i;
        gi_render_stats ps;
        prog.last[0] = -1;
        if (rad.progressive) {
          // pass index = the seed offset; r_0 from -gd / -cd, photons per pass from -global / -caustic
          const int64_t idx = loaded.passes_done + (int64_t)i;
          gi_progressive_params pp;
          gi_progressive_params_default(&pp);
          pp.alpha = rad.alpha;
          gi_photon_stats pst;
          ok = gi_set_params(ctx, &P) == GI_OK &&
               gi_accum_add_progressive(ctx, aa, idx, &pp, &pst, &ps) == GI_OK;
          if (!ok) break;
          if (P.verbose) {
            printf("Progressive pass %lld: -gd %.17g -cd %.17g, %lld global and %lld caustic photons stored\n",
                   (long long)idx, gi_progressive_radius(P.global_estimate_dist, rad.alpha, idx),
                   gi_progressive_radius(P.caustic_estimate_dist, rad.alpha, idx),
                   (long long)pst.global_stored, (long long)pst.caustic_stored);
            fflush(stdout);
          }
          primary_samples += ((long long)w * h) << (2 * aa);
        } else {
        ok = gi_set_params(ctx, &Pi) == GI_OK;
        // a carried accumulator goes straight to adaptive passes: the selection's n_min < min_samples
        // rule makes the tiles whose history was lost core
        if (ok && rad.adaptive_tile && (carried || least >= ap.min_samples)) {
          int64_t active = 0;
          ok = gi_accum_add_adaptive(ctx, aa, &ap, nullptr, &active, &ps) == GI_OK;
          if (ok && active == 0) break;  // every tile is at the threshold: nothing was rendered
          primary_samples += (long long)active << (2 * aa);
        } else if (ok) {
          ok = (layers_prefix ? gi_accum_add_image_layers(ctx, aa, lay.c, &ps) : gi_accum_add_image(ctx, aa, &ps)) == GI_OK;
          primary_samples += ((long long)w * h) << (2 * aa);
        }
        }
        if (!ok) break;
        passes_done++;
        rs.render_s += ps.render_s;
        rs.screen_rays += ps.screen_rays; rs.shadow_rays += ps.shadow_rays;
        rs.monte_carlo_rays += ps.monte_carlo_rays; rs.transmissive_samples += ps.transmissive_samples;
        rs.specular_samples += ps.specular_samples; rs.indirect_samples += ps.indirect_samples;
        rs.caustic_samples += ps.caustic_samples;
        if (rad.adaptive_tile) {
          ok = gi_accum_get(ctx, nullptr, nullptr, &least, nullptr) == GI_OK;
        } else if (rad.have_noise) {  // defined from two samples per pixel on
          int64_t n = 0;
          ok = gi_accum_get(ctx, nullptr, nullptr, &n, &acc_noise) == GI_OK;
          if (ok && n >= 2 && acc_noise <= rad.noise) break;
        }
      }
      if (ok && rad.adaptive_tile) {
        std::vector<int64_t> counts((size_t)w * h);
        int64_t total = 0;
        ok = gi_accum_get_counts(ctx, counts.data(), &total) == GI_OK;
        acc_total = total;
        for (int64_t v : counts) acc_max = v > acc_max ? v : acc_max;
      }
      if (ok && rad.save_accum) {  // the accumulator as the pass loop leaves it
        AccumFile out_acc;
        out_acc.state.resize((size_t)w * h * 6);
        out_acc.counts.resize((size_t)w * h);
        out_acc.passes_done = loaded.passes_done + passes_done;
        ok = gi_accum_export(ctx, out_acc.state.data(), out_acc.counts.data()) == GI_OK;
        if (ok && !WriteAccum(rad.save_accum, w, h, out_acc)) {
          fprintf(stderr, "Unable to write -save_accum file %s\n", rad.save_accum);
          gi_destroy(ctx);
          return -1;
        }
      }
      int64_t n = 0;
      ok = ok && gi_accum_get(ctx, mean.data(), nullptr, &n, &acc_noise) == GI_OK;
      std::vector<float> filtered;  // -vdenoise: the written image is the tone-mapped filtered mean
      if (ok && vdenoise_levels) {
        std::vector<gi_pixel_features> feat;
        if (!history) {
          feat.resize((size_t)w * h);
          ok = gi_camera_features(ctx, aa, w, h, feat.data()) == GI_OK;
        }
        gi_vdenoise_params vp;
        gi_vdenoise_params_default(&vp);
        vp.levels = vdenoise_levels;
        filtered.resize((size_t)w * h * 3);
        if (!layers_prefix)
          ok = ok && gi_accum_denoise(ctx, history ? cur_feat.data() : feat.data(), &vp, filtered.data(), nullptr,
                                      &vdenoise_ms) == GI_OK;
        // -layers: every layer but the specular one filtered under its own variance, then their sum
        std::vector<double> sum(layers_prefix ? filtered.size() : 0, 0.0);
        std::vector<float> part(sum.size());
        for (int l = 0; ok && layers_prefix && l < GI_LAYER_COUNT; l++) {
          double ms = 0.0;
          // (a failure's message is the layer context's)
          if (l == GI_LAYER_SPECULAR) ok = gi_accum_get(lay.c[l], part.data(), nullptr, nullptr, nullptr) == GI_OK;
          else ok = gi_accum_denoise(lay.c[l], feat.data(), &vp, part.data(), nullptr, &ms) == GI_OK;
          if (!ok) fprintf(stderr, "%s\n", gi_last_error(lay.c[l]));
          vdenoise_ms += ms;
          for (size_t i = 0; i < sum.size(); i++) sum[i] += (double)part[i];
        }
        for (size_t i = 0; i < sum.size(); i++) filtered[i] = (float)sum[i];
      }
      for (int l = 0; ok && layers_prefix && l < GI_LAYER_COUNT; l++)
        ok = gi_accum_get(lay.c[l], layer_means.data() + (size_t)l * w * h * 3, nullptr, nullptr, nullptr) == GI_OK;
      ok = ok && gi_tonemap(ctx, w, h, vdenoise_levels ? filtered.data() : mean.data(), rad.exposure,
                            rad.white, rgbf.data(), rgb.data()) == GI_OK;
      acc_n = n;
      gi_set_params(ctx, &P);
      if (ok && history) {
        ok = gi_get_view(ctx, &prev_view) == GI_OK;
        prev_feat.swap(cur_feat);
      }
      if (!ok) {
        fprintf(stderr, "%s\n", gi_last_error(ctx));
        gi_destroy(ctx);
        return -1;
      }
    } else if (gi_render_image(ctx, aa, w, h, rgb.data(), denoise_levels ? rgbf.data() : nullptr, &rs) != GI_OK) {
      fprintf(stderr, "%s\n", gi_last_error(ctx));
      gi_destroy(ctx);
      return -1;
    }
    // -layers without passes: the frame once more, split (the image above is gi_render_image's own)
    if (layers_prefix && !rad.any &&
        gi_render_layers(ctx, aa, w, h, layer_means.data(), nullptr, nullptr, nullptr) != GI_OK) {
      fprintf(stderr, "%s\n", gi_last_error(ctx));
      gi_destroy(ctx);
      return -1;
    }
    double denoise_ms = 0.0;
    if (denoise_levels) {  // the written image is the filtered frame
      std::vector<gi_pixel_features> feat((size_t)w * h);
      gi_denoise_params dp;
      gi_denoise_params_default(&dp);
      dp.levels = denoise_levels;
      if (gi_camera_features(ctx, aa, w, h, feat.data()) != GI_OK ||
          gi_denoise(ctx, w, h, rgbf.data(), feat.data(), &dp, nullptr, rgb.data(), &denoise_ms) != GI_OK) {
        fprintf(stderr, "%s\n", gi_last_error(ctx));
        gi_destroy(ctx);
        return -1;
      }
    }
    PrintProgress(1.0, PROGRESS_BAR_WIDTH);  // render.cpp:201-202
    printf("\n");
    fflush(stdout);
    if (P.verbose) {
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
      if (!views.empty())
        printf("View %d of %d: %lld primary samples rendered\n", k, nviews, primary_samples);
      if (carried)
        printf("Reprojected history: %lld pixels kept, %lld pixels reset, %lld samples kept\n",
               (long long)rps.kept_pixels, (long long)rps.reset_pixels, (long long)rps.kept_samples);
      if (rad.adaptive_tile)
        printf("Accumulated image: %d passes, %lld samples, %lld to %lld per pixel, noise = %.6g\n",
               passes_done, acc_total, acc_n, acc_max, acc_noise);
      else if (rad.any)
        printf("Accumulated image: %d passes, N = %lld samples per pixel, noise = %.6g\n", passes_done,
               acc_n, acc_noise);
      if (denoise_levels) printf("Denoised image: %d levels, %.3f ms\n", denoise_levels, denoise_ms);
      if (vdenoise_levels)
        printf("Variance-guided denoise: %d levels, %.3f ms\n", vdenoise_levels, vdenoise_ms);
      fflush(stdout);
    }
    if (k == nviews - 1) gi_destroy(ctx);
    auto tw = std::chrono::steady_clock::now();
    if (gi_write_image(out_k.c_str(), w, h, rgb.data()) != GI_OK) {
      const char *ext = strrchr(out, '.');
      if (ext && !strncmp(ext, ".tif", 4)) fprintf(stderr, "TIFF not supported\n");  // R2Image.cpp:1300
      else fprintf(stderr, "Unable to write image %s\n", out_k.c_str());
      if (k < nviews - 1) gi_destroy(ctx);
      return -1;
    }
    if (rad.file && gi_write_image_float(rad_k.c_str(), w, h, mean.data()) != GI_OK) {
      fprintf(stderr, "Unable to write image %s\n", rad_k.c_str());
      if (k < nviews - 1) gi_destroy(ctx);
      return -1;
    }
    if (layers_prefix && !WriteLayers(layers_prefix, w, h, layer_means)) return -1;
    if (P.verbose) {
      printf("Wrote image to %s ...\n", out_k.c_str());
      printf("  Time = %.2f seconds\n",
             std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count());
      printf("  Width = %d\n", w);
      printf("  Height = %d\n", h);
      fflush(stdout);
    }
  }  // views
  return 0;
}
