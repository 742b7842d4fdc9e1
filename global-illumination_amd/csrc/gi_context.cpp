// gi_context.cpp -- contexts of the MI355X renderer: the RCCL loader, creation and destruction,
// parameters, the scene upload, the camera, and the helpers every host unit shares (gi_ctx.h).
#include <dlfcn.h>
#include <cmath>
#include "gi_ctx.h"

namespace gi_internal __attribute__((visibility("hidden"))) {

bool Rccl::load() {
  static std::mutex mu;
  std::lock_guard<std::mutex> g(mu);
  if (tried) return ok;
  tried = true;
  void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
  if (!h) return false;
  commInitAll = (decltype(commInitAll))dlsym(h, "ncclCommInitAll");
  commDestroy = (decltype(commDestroy))dlsym(h, "ncclCommDestroy");
  groupStart = (decltype(groupStart))dlsym(h, "ncclGroupStart");
  groupEnd = (decltype(groupEnd))dlsym(h, "ncclGroupEnd");
  send = (decltype(send))dlsym(h, "ncclSend");
  recv = (decltype(recv))dlsym(h, "ncclRecv");
  errString = (decltype(errString))dlsym(h, "ncclGetErrorString");
  commCount = (decltype(commCount))dlsym(h, "ncclCommCount");
  commUserRank = (decltype(commUserRank))dlsym(h, "ncclCommUserRank");
  ok = commInitAll && commDestroy && groupStart && groupEnd && send && recv && errString;
  return ok;
}
Rccl g_rccl;

Flags make_flags(const gi_params &P) {
  Flags F;
  memset(&F, 0, sizeof F);
  F.ambient = P.ambient; F.direct = P.direct_illum; F.transmissive = P.transmissive_illum;
  F.specular = P.specular_illum; F.indirect = P.indirect_illum; F.caustic = P.caustic_illum;
  F.photon_viz = P.direct_photon_illum; F.fast_global = P.fast_global;
  F.cache = P.irradiance_cache; F.shadows = P.shadows; F.soft_shadows = P.soft_shadows;
  F.light_test = P.light_test; F.shadow_test = P.shadow_test; F.monte_carlo = P.monte_carlo;
  F.max_monte_depth = P.max_monte_depth; F.recursive_shadows = P.recursive_shadows;
  F.distrib_trans = P.distrib_transmissive; F.trans_test = P.transmissive_test;
  F.distrib_spec = P.distrib_specular; F.spec_test = P.specular_test; F.fresnel = P.fresnel;
  F.indirect_test = P.indirect_test; F.dof = P.depth_of_field; F.dof_test = P.dof_test;
  F.max_photon_depth = P.max_photon_depth;
  F.ir_air = P.ir_air;
  F.prob_absorb = P.prob_absorb;
  F.seed = P.seed;
  return F;
}

// render.cpp:67-77: the camera block of the render kernels (and what gi_get_view returns)
DCamera make_camera(const HostScene &H, const gi_params &P) {
  DCamera cam;
  memset(&cam, 0, sizeof cam);
  double tx = tan(H.xfov), ty = tan(H.yfov);
  double ul = sqrt(H.up[0] * H.up[0] + H.up[1] * H.up[1] + H.up[2] * H.up[2]);
  double rl = sqrt(H.right[0] * H.right[0] + H.right[1] * H.right[1] + H.right[2] * H.right[2]);
  for (int i = 0; i < 3; i++) {
    cam.eye[i] = H.eye[i];
    cam.far_org[i] = H.eye[i] + H.towards[i] * P.focus_depth;
    cam.far_right[i] = H.right[i] * tx * P.focus_depth;
    cam.far_up[i] = H.up[i] * ty * P.focus_depth;
    cam.dof_u[i] = (ul == 0.0 ? H.up[i] : H.up[i] / ul) * P.aperture_radius;
    cam.dof_v[i] = (rl == 0.0 ? H.right[i] : H.right[i] / rl) * P.aperture_radius;
  }
  return cam;
}

SceneView make_view(gi_ctx *c) {
  SceneView S;
  memset(&S, 0, sizeof S);
  const HostScene &H = c->scene;
  S.nodes = c->res.d_nodes.as<DNode>();
  S.elems = c->res.d_elems.as<DElement>();
  S.shapes = c->res.d_shapes.as<DShape>();
  S.tris = c->res.d_tris.as<DTri>();
  S.bvh = c->res.d_bvh.as<DBvhNode>();
  S.mats = c->res.d_mats.as<DMaterial>();
  S.lights = c->res.d_lights.as<DLight>();
  S.nnodes = (int)H.nodes.size();
  S.nelems = (int)H.elems.size();
  S.nlights = (int)H.lights.size();
  S.kinds = 0;
  for (const DShape &sh : H.shapes) S.kinds |= 1u << sh.kind;
  S.hard_lights = 1;
  for (const DLight &L : H.lights)
    if (L.kind == LK_AREA || L.kind == LK_RECT) S.hard_lights = 0;
  // the division-free element pre-test pays where soft lights cast many shadow rays (C3 jensen
  // +3 %) and costs where every light is hard (C2 cornell -2 %, r02 A/B); GI_ELEM_PRETEST=0/1
  S.elem_pretest = c->elem_pretest >= 0 ? c->elem_pretest : (S.hard_lights ? 0 : 1);
  // rigid scene graph: every node's 3x3 part orthonormal (then R3SceneNode's t rescale stays 1
  // and a hit's t is its world distance, which the bounded shadow walk relies on)
  S.rigid = 1;
  for (const DNode &nd : H.nodes) {
    if (nd.identity) continue;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        double g = nd.T[4 * 0 + i] * nd.T[4 * 0 + j] + nd.T[4 * 1 + i] * nd.T[4 * 1 + j] +
                   nd.T[4 * 2 + i] * nd.T[4 * 2 + j];
        if (std::fabs(g - (i == j ? 1.0 : 0.0)) > 1e-12) S.rigid = 0;
      }
  }
  S.radius = H.radius;
  for (int i = 0; i < 3; i++) {
    S.centroid[i] = H.centroid[i];
    S.ambient[i] = H.ambient[i];
    S.background[i] = H.background[i];
  }
  S.cam = make_camera(H, c->P);
  return S;
}

hipError_t upload(DBuf &b, const void *src, size_t bytes, hipStream_t st) {
  hipError_t e = b.ensure(bytes);
  if (e != hipSuccess) return e;
  if (bytes) return hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st);
  return hipSuccess;
}

ScanTemp scan_temp(gi_ctx *c, int64_t n) {
  ScanTemp t;
  memset(&t, 0, sizeof t);
  int64_t m = n;
  for (int l = 0; l < 8; l++) {
    m = (m + 1023) / 1024;
    c->s.scan_lvl[l].ensure((size_t)(m + 2) * 4);
    c->s.scan_out[l].ensure((size_t)(m + 2) * 4);
    t.level[l] = c->s.scan_lvl[l].as<uint32_t>();
    t.level_out[l] = c->s.scan_out[l].as<uint32_t>();
  }
  t.depth = 0;
  return t;
}

int check_ready(gi_ctx *c) {
  if (!c->have_scene) return fail(c, GI_ERR_STATE, "no scene loaded (gi_read_scene)");
  if (c->scene.unsupported_depth)
    return fail(c, GI_ERR_UNSUPPORTED, "scene graph deeper than 16 levels");
  if (c->scene.unsupported_shapes)
    return fail(c, GI_ERR_UNSUPPORTED,
                "scene contains cone shapes: not yet on the device path");
  return GI_OK;
}

}  // namespace gi_internal

namespace {

// BuildDirectionLookupTable, photon_utils.cpp:253-272
void build_lut(std::vector<double> &lut) {
  lut.assign(65536 * 3, 0.0);
  const double PI = 3.14159265358979323846;
  for (int phi = 0; phi < 256; phi++)
    for (int th = 0; th < 256; th++) {
      double tp = (phi * (2.0 * PI) / 255.0) - PI;
      double tt = (th * PI / 255.0);
      double x = sin(tt) * cos(tp), y = sin(tt) * sin(tp), z = cos(tt);
      double l = sqrt((x * x) + (y * y) + (z * z));
      if (l != 0.0) { x /= l; y /= l; z /= l; }
      int i = 256 * phi + th;
      lut[3 * i] = x; lut[3 * i + 1] = y; lut[3 * i + 2] = z;
    }
}

int upload_scene(gi_ctx *c) {
  HostScene &H = c->scene;
  if (H.mats.size() >= (size_t)QMETA_MAX_MATS) return fail(c, GI_ERR_UNSUPPORTED, "more than 2^26 materials");
  HIPCHK(c, upload(c->res.d_nodes, H.nodes.data(), H.nodes.size() * sizeof(DNode), c->stream));
  HIPCHK(c, upload(c->res.d_elems, H.elems.data(), H.elems.size() * sizeof(DElement), c->stream));
  HIPCHK(c, upload(c->res.d_shapes, H.shapes.data(), H.shapes.size() * sizeof(DShape), c->stream));
  HIPCHK(c, upload(c->res.d_tris, H.tris.data(), H.tris.size() * sizeof(DTri), c->stream));
  HIPCHK(c, upload(c->res.d_bvh, H.bvh.data(), H.bvh.size() * sizeof(DBvhNode), c->stream));
  HIPCHK(c, upload(c->res.d_mats, H.mats.data(), H.mats.size() * sizeof(DMaterial), c->stream));
  HIPCHK(c, upload(c->res.d_lights, H.lights.data(), H.lights.size() * sizeof(DLight), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->have_scene = true;
  c->map_valid[0] = c->map_valid[1] = false;
  c->q_per_prim = 0.0;  // the batch size is re-measured on the new scene
  c->mc_app_rate[0] = c->mc_app_rate[1] = 0.0;
  for (int i = 0; i < 3; i++) {
    c->sbmin[i] = (float)H.bmin[i];
    c->sbmax[i] = (float)H.bmax[i];
  }
  return GI_OK;
}

}  // namespace

// =======================================================================================
// C-ABI
// =======================================================================================
extern "C" {

int gi_create(gi_ctx **out, int dev) {
  *out = nullptr;
  gi_ctx *c = new gi_ctx();
  c->device = dev;
  gi_params_default(&c->P);
  if (hipSetDevice(dev) != hipSuccess) { delete c; return GI_ERR_HIP; }
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return GI_ERR_HIP; }
  // (stream priorities for either stream measured no different: r06)
  if (hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess) c->stream2 = nullptr;
  hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
  hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming);
  for (int m = 0; m < 2; m++) {
    c->mx[m].st = c->stream;
    hipEventCreate(&c->mx[m].ev0);
    hipEventCreate(&c->mx[m].ev1);
    hipEventCreate(&c->mx[m].ev2);
    hipEventCreate(&c->mx[m].ev3);
  }
  std::vector<double> lut;
  build_lut(lut);
  if (upload(c->res.d_lut, lut.data(), lut.size() * 8, c->stream) != hipSuccess ||
      c->res.d_stats.ensure(ST_BYTES) != hipSuccess) {
    delete c;
    return GI_ERR_HIP;
  }
  hipStreamSynchronize(c->stream);
  // diagnostics and the exactness-tested alternatives (tests/test_gpu_*.py select them)
  c->batch_log = (log_bits() & 2) != 0;
  c->knn_log = (log_bits() & 4) != 0;
  c->knn_dbg = (int)env_num("GI_KNN_DBG", 0);
  c->render_dbg = (int)env_num("GI_DBG", 0);
  c->slot_limit = (int64_t)env_num("GI_SLOT_LIMIT", 0);
  if (const int ls = (int)env_num("GI_LEAF_SIZE", 0); ls > 0) c->leaf_size[0] = c->leaf_size[1] = ls;
  c->gpu_kd = env_num("GI_HOST_KD", 0) == 0;                      // 1: the host kd build
  c->photon_2pass = env_num("GI_PHOTON_2PASS", c->photon_2pass) != 0;
  c->prate[0] = c->prate[1] = std::max(0.0, env_num("GI_PHOTON_RATE0", c->prate[0]));
  c->chunk_minsub_big = std::min(64, std::max(1, (int)env_num("GI_CHUNK_MINSUB_BIG", c->chunk_minsub_big)));
  c->chunk_dk_exact = env_num("GI_CHUNK_DK_EXACT", c->chunk_dk_exact) != 0;
  c->chunk_cap_big3 = (int)env_num("GI_CHUNK_CAP_BIG3", c->chunk_cap_big3);
  c->chunk_minsub = std::min(64, std::max(1, (int)env_num("GI_CHUNK_MINSUB", c->chunk_minsub)));
  c->split_ind = env_num("GI_SPLIT_IND", c->split_ind) != 0;
  c->knn_general_mode = std::max(-1, std::min(1, (int)env_num("GI_KNN_GENERAL", c->knn_general_mode)));
  c->use_dk = env_num("GI_KNN_DK", c->use_dk) != 0;
  c->chunk_dk = env_num("GI_CHUNK_DK", c->chunk_dk) != 0;
  c->mc_sub = env_num("GI_MC_SUB", c->mc_sub) != 0;
  c->mc_persist = std::max(-1, (int)env_num("GI_MC_PERSIST", c->mc_persist));
  c->mc_wave = std::min(MC_WAVE_MAX_ROUNDS, std::max(-1, (int)env_num("GI_MC_WAVE", c->mc_wave)));
  c->elem_pretest = env_num("GI_ELEM_PRETEST", c->elem_pretest) != 0;
  c->chunk_fb_all = env_num("GI_CHUNK_FB_ALL", c->chunk_fb_all) != 0;
  c->ind_frac = std::min(1.0, std::max(1e-6, env_num("GI_IND_FRAC", c->ind_frac)));
  c->knn_kernel_kind = (int)env_num("GI_KNN_KERNEL", c->knn_kernel_kind);
  c->row_order = env_num("GI_ROW_ORDER", c->row_order) != 0;
  c->surf_key = env_num("GI_SURF_KEY", c->surf_key) != 0;
  c->surf_key_c = env_num("GI_SURF_KEY_C", c->surf_key_c) != 0;
  c->fb_wave = env_num("GI_FB_WAVE", c->fb_wave) != 0;
  *out = c;
  return GI_OK;
}

int gi_create_devices(gi_ctx **out, const gi_device_set *set) {
  if (!out || !set || set->count < 1 || set->count > GI_MAX_DEVICES) return GI_ERR_ARG;
  *out = nullptr;
  gi_ctx *c = nullptr;
  int rc = gi_create(&c, set->devices[0]);
  if (rc) return rc;
  bool distinct = true;
  for (int k = 1; k < set->count; k++) {
    gi_ctx *d = nullptr;
    rc = gi_create(&d, set->devices[k]);
    if (rc) {
      gi_destroy(c);
      return rc;
    }
    c->peers.push_back(d);
    for (int j = 0; j < k; j++) distinct = distinct && set->devices[j] != set->devices[k];
  }
  if (set->count > 1 && distinct) {
    if (!g_rccl.load()) {
      gi_destroy(c);
      return GI_ERR_UNSUPPORTED;
    }
    c->comms.assign(set->count, nullptr);
    ncclResult_t r = g_rccl.commInitAll(c->comms.data(), set->count, set->devices);
    if (r != ncclSuccess) {
      c->comms.clear();
      gi_destroy(c);
      return GI_ERR_HIP;
    }
  }
  hipSetDevice(c->device);
  *out = c;
  return GI_OK;
}

int gi_device_info(const gi_ctx *c, int max, int *ndev, int *devices, int *pci_bus,
                   int *comm_rank, int *comm_count) {
  if (!c || !ndev || max < 0) return GI_ERR_ARG;
  const int nd = 1 + (int)c->peers.size();
  *ndev = nd;
  for (int k = 0; k < nd && k < max; k++) {
    const gi_ctx *d = k ? c->peers[k - 1] : c;
    if (devices) devices[k] = d->device;
    if (pci_bus) {
      int bus = -1;
      if (hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, d->device) != hipSuccess) bus = -1;
      pci_bus[k] = bus;
    }
    if (comm_rank) {
      int r = -1;
      if (k < (int)c->comms.size() && c->comms[k] && g_rccl.commUserRank &&
          g_rccl.commUserRank(c->comms[k], &r) != ncclSuccess)
        r = -1;
      comm_rank[k] = r;
    }
  }
  if (comm_count) {
    int n = 0;
    if (!c->comms.empty() && c->comms[0] && g_rccl.commCount &&
        g_rccl.commCount(c->comms[0], &n) != ncclSuccess)
      n = 0;
    *comm_count = n;
  }
  return GI_OK;
}

// Frees the device scratch (gi_ctx.h Scratch: everything but the scene, the maps, the counters, the
// accumulator and the streams), device by device; the next call re-allocates what it needs.
int gi_release_scratch(gi_ctx *c) {
  if (!c) return GI_ERR_ARG;
  DeviceScope scope(c->device);  // the caller's current device is restored on return
  for (gi_ctx *d : c->peers) {
    hipSetDevice(d->device);
    hipDeviceSynchronize();
    d->s = Scratch();
  }
  hipSetDevice(c->device);
  hipDeviceSynchronize();
  c->s = Scratch();
  return GI_OK;
}

void gi_destroy(gi_ctx *c) {
  if (!c) return;
  for (ncclComm_t m : c->comms)
    if (m) g_rccl.commDestroy(m);
  c->comms.clear();
  for (gi_ctx *d : c->peers) gi_destroy(d);
  c->peers.clear();
  hipSetDevice(c->device);
  // the buffers are freed here, explicitly, before the streams they were used on are destroyed
  // (the destructor then finds them empty)
  c->s = Scratch();
  c->res = Resident();
  for (int m = 0; m < 2; m++) {
    MapExec &X = c->mx[m];
    if (X.ev0) hipEventDestroy(X.ev0);
    if (X.ev1) hipEventDestroy(X.ev1);
    if (X.ev2) hipEventDestroy(X.ev2);
    if (X.ev3) hipEventDestroy(X.ev3);
  }
  if (c->ev_fork) hipEventDestroy(c->ev_fork);
  if (c->ev_join) hipEventDestroy(c->ev_join);
  if (c->stream2) hipStreamDestroy(c->stream2);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
}

const char *gi_last_error(const gi_ctx *c) { return c ? c->err.c_str() : "null context"; }

int gi_set_progress(gi_ctx *c, gi_progress_fn fn, void *user) {
  if (!c) return GI_ERR_ARG;
  c->progress = fn;  // device 0 reports for a device set (its share of the pixels)
  c->progress_user = user;
  return GI_OK;
}

int gi_set_params(gi_ctx *c, const gi_params *p) {
  if (!c || !p) return GI_ERR_ARG;
  c->P = *p;
  c->have_params = true;
  for (gi_ctx *d : c->peers) {
    d->P = *p;
    d->have_params = true;
  }
  return GI_OK;
}

int gi_read_scene(gi_ctx *c, const char *path, int real) {
  if (!c || !path) return GI_ERR_ARG;
  hipSetDevice(c->device);
  std::string err;
  HostScene S;
  if (!load_scene(path, real != 0, S, err)) return fail(c, GI_ERR_IO, err);
  c->scene = std::move(S);
  // the device set shares the host scene; every device gets its own copy of the arrays
  return on_devices(c, [&](int k, gi_ctx *d) -> int {
    if (k) d->scene = c->scene;
    return upload_scene(d);
  });
}

int gi_get_camera(const gi_ctx *c, gi_camera *out) {
  if (!c || !out) return GI_ERR_ARG;
  if (!c->have_scene) return GI_ERR_STATE;
  const double *r = c->scene.cam_raw;
  for (int i = 0; i < 3; i++) {
    out->eye[i] = r[i];
    out->towards[i] = r[3 + i];
    out->up[i] = r[6 + i];
  }
  out->xfov = r[9];
  return GI_OK;
}

int gi_get_view(const gi_ctx *c, gi_view *out) {
  if (!c || !out) return GI_ERR_ARG;
  if (!c->have_scene) return GI_ERR_STATE;
  const DCamera cam = make_camera(c->scene, c->P);
  for (int i = 0; i < 3; i++) {
    out->eye[i] = cam.eye[i];
    out->far_org[i] = cam.far_org[i];
    out->far_right[i] = cam.far_right[i];
    out->far_up[i] = cam.far_up[i];
  }
  return GI_OK;
}

int gi_set_camera(gi_ctx *c, const gi_camera *cam) {
  if (!c || !cam) return GI_ERR_ARG;
  if (!c->have_scene) return fail(c, GI_ERR_STATE, "no scene loaded (gi_read_scene)");
  double r[10];
  for (int i = 0; i < 3; i++) {
    r[i] = cam->eye[i];
    r[3 + i] = cam->towards[i];
    r[6 + i] = cam->up[i];
  }
  r[9] = cam->xfov;
  for (double v : r)
    if (!std::isfinite(v)) return fail(c, GI_ERR_ARG, "camera: non-finite value");
  const double *t = r + 3, *u = r + 6;
  const double x[3] = {u[1] * t[2] - u[2] * t[1], u[2] * t[0] - u[0] * t[2], u[0] * t[1] - u[1] * t[0]};
  const double tl = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
  const double ul = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  const double xl = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  if (!(tl > 0.0) || !std::isfinite(tl)) return fail(c, GI_ERR_ARG, "camera: zero towards vector");
  // parallel within rounding: the sine of the angle between them is below 1e-12
  if (!(xl > 1e-12 * tl * ul) || !std::isfinite(xl))
    return fail(c, GI_ERR_ARG, "camera: up vector parallel to towards");
  if (!(r[9] > 0.0 && r[9] < 1.5707963267948966))
    return fail(c, GI_ERR_ARG, "camera: xfov outside (0, pi/2)");
  // the view enters only the primary rays (make_view): the scene upload, the photon maps, their
  // kd trees and dk bounds and the -cache irradiance stay; the batch size is measured again
  set_camera(c->scene, r);
  c->q_per_prim = 0.0;
  for (gi_ctx *d : c->peers) {
    set_camera(d->scene, r);
    d->q_per_prim = 0.0;
  }
  return GI_OK;
}

int gi_scene_info(gi_ctx *c, int *nnodes, int *nlights, int *nprims, double *radius) {
  if (!c || !c->have_scene) return GI_ERR_STATE;
  if (nnodes) *nnodes = (int)c->scene.nodes.size();
  if (nlights) *nlights = (int)c->scene.lights.size();
  if (nprims) *nprims = (int)c->scene.shapes.size();
  if (radius) *radius = c->scene.radius;
  return GI_OK;
}

int gi_get_materials(gi_ctx *c, gi_material *out, int32_t cap, int32_t *n) {
  if (!c || !n) return GI_ERR_ARG;
  if (!c->have_scene) return fail(c, GI_ERR_STATE, "no scene loaded (gi_read_scene)");
  const std::vector<DMaterial> &mats = c->scene.mats;
  *n = (int32_t)mats.size();
  if (!out) return GI_OK;
  if (cap < *n) return fail(c, GI_ERR_ARG, "material buffer holds fewer materials than the scene");
  for (size_t i = 0; i < mats.size(); i++) {
    const DMaterial &m = mats[i];
    gi_material &o = out[i];
    for (int k = 0; k < 3; k++) {
      o.ka[k] = m.ka[k]; o.kd[k] = m.kd[k]; o.ks[k] = m.ks[k]; o.kt[k] = m.kt[k]; o.e[k] = m.e[k];
    }
    o.n = m.n;
    o.ir = m.ir;
  }
  return GI_OK;
}

}  // extern "C"
