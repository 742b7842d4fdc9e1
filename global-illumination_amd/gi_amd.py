"""Python mirror of the reference's renderer interface over the C-ABI of include/gi.h.

Names follow the reference (ReillyBova/Global-Illumination, src/):
  ParseArgs        utils/io_utils.cpp:16-212
  ReadScene        utils/io_utils.cpp:219-250
  MapPhotons       photonmap.cpp:260-436
  RenderImage      render.cpp:155-259
  get_camera / set_camera / camera_rays / render_rays: further views from the resident photon
                   maps (no reference counterpart; gi.h "views from resident photon maps")
  materials / camera_features / ray_features / denoise: per-pixel feature planes and the
                   edge-avoiding denoise pass (no reference counterpart; gi.h "feature planes
                   and denoise pass")
  accum_select / accum_add_tiles / accum_add_adaptive / accum_get_counts: adaptive passes over
                   the noisy tiles of the accumulator (gi.h "adaptive passes")
  denoise_radiance / accum_denoise: the variance-guided denoise of a radiance frame and of
                   the accumulator (gi.h "variance-guided denoise")
  get_view / accum_reproject: the accumulator carried into a new camera (gi.h "reprojection
                   across views")
  accum_export / accum_import / accum_merge / accum_export_packed / accum_merge_packed /
  accum_merge_from: the accumulator's fp64 state out of its context, back in, and folded into
                   another accumulator (gi.h "accumulator state")
  render_radiance / render_rays_radiance / accum_* / tonemap / write_image_float: unclamped
                   radiance frames with their variance, accumulation over passes and the tone
                   map (no reference counterpart; gi.h "radiance frames, accumulation over
                   passes, tone map")
  render_layers / render_rays_layers / accum_add_*_layers: the same frames and passes split
                   into light-path layers (gi.h "light-path layers")
  EstimateRadiance utils/photon_utils.cpp:72-162      (batched test seam)
  FindClosestQuick R3Shapes/R3Kdtree.cpp:688-848      (batched test seam)
  Intersects       R3Graphics/R3Scene.cpp:471-479     (batched test seam)

The shared library libgi_amd.so (HIP, gfx950) is loaded from this directory; there is no CPU
fallback: if the library or a GPU is missing every entry point raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GI_AMD_LIB") or os.path.join(_HERE, "libgi_amd.so")  # GI_AMD_LIB: experiment builds

GI_OK, GI_ERR_ARG, GI_ERR_IO, GI_ERR_HIP, GI_ERR_STATE, GI_ERR_UNSUPPORTED, GI_ERR_ALLOC = range(7)
DISK, CONE, GAUSS = 0, 1, 2
GLOBAL, CAUSTIC = 0, 1
# light-path layers (gi.h GI_LAYER_*): plane l of render_layers' outputs, entry l of a layered
# pass's context list; plane LAYER_TOTAL is the undivided frame
LAYER_NAMES = ("surface", "specular", "indirect", "global", "caustic")
LAYER_SURFACE, LAYER_SPECULAR, LAYER_INDIRECT, LAYER_GLOBAL, LAYER_CAUSTIC = range(5)
LAYER_COUNT = LAYER_TOTAL = 5

EXPORTED = [
    "gi_params_default", "gi_parse_args", "gi_create", "gi_create_devices", "gi_device_info",
    "gi_destroy", "gi_last_error",
    "gi_set_params", "gi_read_scene", "gi_scene_info", "gi_map_photons", "gi_set_photon_map",
    "gi_get_photon_map", "gi_get_kd_tree", "gi_set_progress", "gi_render_image", "gi_render_tiles",
    "gi_get_camera", "gi_set_camera", "gi_camera_rays", "gi_render_rays",
    "gi_render_tiles_packed", "gi_compose_tiles", "gi_quantize",
    "gi_get_materials", "gi_camera_features", "gi_ray_features", "gi_denoise_params_default",
    "gi_denoise",
    "gi_render_radiance", "gi_render_rays_radiance", "gi_accum_reset", "gi_accum_add_image",
    "gi_accum_add_rays", "gi_accum_get", "gi_tonemap", "gi_radiance_bench",
    "gi_render_layers", "gi_render_rays_layers", "gi_accum_add_image_layers",
    "gi_accum_add_rays_layers", "gi_layers_timing",
    "gi_accum_get_counts", "gi_adaptive_params_default", "gi_accum_select", "gi_accum_add_tiles",
    "gi_accum_add_adaptive", "gi_adaptive_bench",
    "gi_vdenoise_params_default", "gi_denoise_radiance", "gi_accum_denoise",
    "gi_get_view", "gi_reproject_params_default", "gi_accum_reproject",
    "gi_accum_export", "gi_accum_import", "gi_accum_merge", "gi_accum_export_packed",
    "gi_accum_merge_packed", "gi_accum_merge_from",
    "gi_progressive_params_default", "gi_progressive_radius", "gi_accum_add_progressive",
    "gi_estimate_radiance_batch", "gi_knn_batch", "gi_knn_bench", "gi_intersect_batch",
    "gi_intersect_probe", "gi_illum_probe", "gi_scene_triangle_planes",
    "gi_scene_slab_boxes",
    "gi_math_probe", "gi_release_scratch",
    "gi_write_image", "gi_write_image_float",
]


class GiParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "verbose", "threads", "fresnel", "ambient", "direct_illum", "transmissive_illum",
        "specular_illum", "indirect_illum", "caustic_illum", "direct_photon_illum", "fast_global",
        "irradiance_cache", "shadows", "soft_shadows", "light_test", "shadow_test", "monte_carlo",
        "max_monte_depth", "recursive_shadows", "distrib_transmissive", "transmissive_test",
        "distrib_specular", "specular_test", "depth_of_field", "dof_test", "global_photon_count",
        "caustic_photon_count", "max_photon_depth", "indirect_test", "global_estimate_size",
        "global_filter", "caustic_estimate_size", "caustic_filter", "gpus")] + [
        (n, C.c_double) for n in (
            "ir_air", "prob_absorb", "focus_depth", "aperture_radius", "global_estimate_dist",
            "caustic_estimate_dist", "filter_const_a", "filter_const_b", "filter_const_k")] + [
        ("seed", C.c_uint64)]


PHOTON_DTYPE = np.dtype([("pos", "<f4", 3), ("rgbe", "u1", 4), ("dir", "<u2"), ("flags", "<u2")])
assert PHOTON_DTYPE.itemsize == 20

QUERY_DTYPE = np.dtype([
    ("point", "<f8", 3), ("normal", "<f8", 3), ("exact_bounce", "<f8", 3), ("cos_theta", "<f8"),
    ("kd", "<f8", 3), ("ks", "<f8", 3), ("shininess", "<f8"), ("max_dist", "<f8"),
    ("k", "<i4"), ("filter", "<i4")])


class Camera(C.Structure):
    """gi_camera: the .scn `camera` command's first ten numbers, as given."""
    _fields_ = [("eye", C.c_double * 3), ("towards", C.c_double * 3), ("up", C.c_double * 3),
                ("xfov", C.c_double)]


RAY_DTYPE = np.dtype([("org", "<f8", 3), ("dir", "<f8", 3)])  # gi_ray
assert RAY_DTYPE.itemsize == 48

# gi_material / gi_pixel_features
MATERIAL_DTYPE = np.dtype([("ka", "<f8", 3), ("kd", "<f8", 3), ("ks", "<f8", 3), ("kt", "<f8", 3),
                           ("e", "<f8", 3), ("n", "<f8"), ("ir", "<f8")])
assert MATERIAL_DTYPE.itemsize == 136
FEATURE_DTYPE = np.dtype([("normal", "<f4", 3), ("depth", "<f4"), ("albedo", "<f4", 3),
                          ("coverage", "<f4")])
assert FEATURE_DTYPE.itemsize == 32


class DenoiseParams(C.Structure):
    _fields_ = [("levels", C.c_int32), ("normal_power_log2", C.c_int32),
                ("sigma_color", C.c_double), ("sigma_depth", C.c_double),
                ("sigma_albedo", C.c_double)]


class VDenoiseParams(C.Structure):
    """gi_vdenoise_params"""
    _fields_ = [("levels", C.c_int32), ("normal_power_log2", C.c_int32),
                ("sigma_lum", C.c_double), ("sigma_depth", C.c_double),
                ("sigma_albedo", C.c_double), ("variance_floor", C.c_double)]


class View(C.Structure):
    """gi_view: the pinhole frame the device renders from."""
    _fields_ = [("eye", C.c_double * 3), ("far_org", C.c_double * 3),
                ("far_right", C.c_double * 3), ("far_up", C.c_double * 3)]


class ReprojectParams(C.Structure):
    """gi_reproject_params"""
    _fields_ = [("max_history", C.c_int64), ("depth_tol", C.c_double),
                ("normal_min", C.c_double), ("albedo_tol", C.c_double)]


class ReprojectStats(C.Structure):
    """gi_reproject_stats"""
    _fields_ = [("kept_pixels", C.c_int64), ("reset_pixels", C.c_int64),
                ("kept_samples", C.c_int64)]


class ProgressiveParams(C.Structure):
    """gi_progressive_params"""
    _fields_ = [("alpha", C.c_double), ("global_radius", C.c_double),
                ("caustic_radius", C.c_double)]


GI_ESTIMATE_ALL = 1 << 30


class AdaptiveParams(C.Structure):
    """gi_adaptive_params"""
    _fields_ = [("tile_px", C.c_int32), ("min_samples", C.c_int32), ("max_samples", C.c_int32),
                ("dilate", C.c_int32), ("threshold", C.c_double)]


GI_MAX_DEVICES = 64


class DeviceSet(C.Structure):
    _fields_ = [("count", C.c_int32), ("devices", C.c_int32 * GI_MAX_DEVICES)]


class PhotonStats(C.Structure):
    _fields_ = [("global_stored", C.c_int64), ("caustic_stored", C.c_int64),
                ("global_emitted", C.c_int64), ("caustic_emitted", C.c_int64),
                ("total_s", C.c_double), ("trace_s", C.c_double), ("kd_s", C.c_double),
                ("irradiance_s", C.c_double)]


class RenderStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "screen_rays", "shadow_rays", "monte_carlo_rays", "transmissive_samples",
        "specular_samples", "indirect_samples", "caustic_samples", "knn_queries",
        "knn_photons", "knn_visited")] + [("render_s", C.c_double), ("knn_kernel_ms", C.c_double),
                           ("knn_kernel_launches", C.c_double)] + [
        ("knn_map_queries", C.c_uint64 * 2), ("knn_map_photons", C.c_uint64 * 2),
        ("knn_map_visited", C.c_uint64 * 2), ("knn_map_kernel_ms", C.c_double * 2),
        ("knn_map_launches", C.c_double * 2), ("knn_map_fallback_ms", C.c_double * 2),
        ("knn_map_fallback_queries", C.c_uint64 * 2), ("knn_map_kind", C.c_int32 * 2),
        ("knn_map_pass2_ms", C.c_double * 2), ("knn_map_pass2_queries", C.c_uint64 * 2),
        ("device_render_s_max", C.c_double), ("device_render_s_min", C.c_double),
        ("gather_s", C.c_double)]


def _stats_dict(st):
    out = {}
    for f, _ in type(st)._fields_:
        v = getattr(st, f)
        out[f] = list(v) if isinstance(v, C.Array) else v
    return out


_lib = None


def lib():
    """Load libgi_amd.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: run `make -C global-illumination_amd`")
        # One HIP runtime per process: torch ships its own libamdhip64 (soname libamdhip64.so.7,
        # but its libraries NEED it under the unversioned name), so a process that loads this
        # library first and torch later ends up with two runtimes, and torch then sees no GPU.
        # When torch is importable it is loaded first and the library binds to its runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        P = C.POINTER
        L.gi_params_default.argtypes = [P(GiParams)]
        L.gi_parse_args.argtypes = [C.c_int, P(C.c_char_p), P(GiParams), P(C.c_char_p),
                                    P(C.c_char_p), P(C.c_int), P(C.c_int), P(C.c_int),
                                    P(C.c_int), P(C.c_char_p)]
        L.gi_create.argtypes = [P(C.c_void_p), C.c_int]
        L.gi_create_devices.argtypes = [P(C.c_void_p), P(DeviceSet)]
        L.gi_device_info.argtypes = [C.c_void_p, C.c_int, P(C.c_int), C.c_void_p, C.c_void_p,
                                     C.c_void_p, P(C.c_int)]
        L.gi_destroy.argtypes = [C.c_void_p]
        L.gi_destroy.restype = None
        L.gi_last_error.argtypes = [C.c_void_p]
        L.gi_last_error.restype = C.c_char_p
        L.gi_set_params.argtypes = [C.c_void_p, P(GiParams)]
        L.gi_read_scene.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.gi_scene_info.argtypes = [C.c_void_p, P(C.c_int), P(C.c_int), P(C.c_int),
                                    P(C.c_double)]
        L.gi_map_photons.argtypes = [C.c_void_p, P(PhotonStats)]
        L.gi_set_photon_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
        L.gi_get_photon_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                        P(C.c_int64)]
        L.gi_get_kd_tree.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_int64, P(C.c_int32), P(C.c_int64)]
        L.gi_render_image.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p, P(RenderStats)]
        L.gi_get_camera.argtypes = [C.c_void_p, P(Camera)]
        L.gi_set_camera.argtypes = [C.c_void_p, P(Camera)]
        L.gi_camera_rays.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_int64, P(C.c_int64)]
        L.gi_render_rays.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, P(RenderStats)]
        L.gi_render_tiles.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_void_p, P(RenderStats)]
        L.gi_render_tiles_packed.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                             P(C.c_int64), P(RenderStats)]
        L.gi_compose_tiles.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.gi_quantize.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.gi_get_materials.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, P(C.c_int32)]
        L.gi_camera_features.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.gi_ray_features.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p]
        L.gi_denoise_params_default.argtypes = [P(DenoiseParams)]
        L.gi_denoise_params_default.restype = None
        L.gi_denoise.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                 P(DenoiseParams), C.c_void_p, C.c_void_p, P(C.c_double)]
        L.gi_render_radiance.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, P(RenderStats)]
        L.gi_render_rays_radiance.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              P(RenderStats)]
        L.gi_render_layers.argtypes = L.gi_render_radiance.argtypes
        L.gi_render_rays_layers.argtypes = L.gi_render_rays_radiance.argtypes
        L.gi_accum_add_image_layers.argtypes = [C.c_void_p, C.c_int, P(C.c_void_p), P(RenderStats)]
        L.gi_accum_add_rays_layers.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                               P(C.c_void_p), P(RenderStats)]
        L.gi_layers_timing.argtypes = [C.c_void_p, C.c_int, P(C.c_double)]
        L.gi_accum_reset.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.gi_accum_add_image.argtypes = [C.c_void_p, C.c_int, P(RenderStats)]
        L.gi_accum_add_rays.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        P(RenderStats)]
        L.gi_accum_get.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_int64),
                                   P(C.c_double)]
        L.gi_accum_get_counts.argtypes = [C.c_void_p, C.c_void_p, P(C.c_int64)]
        L.gi_adaptive_params_default.argtypes = [P(AdaptiveParams)]
        L.gi_adaptive_params_default.restype = None
        L.gi_accum_select.argtypes = [C.c_void_p, P(AdaptiveParams), C.c_void_p, C.c_void_p,
                                      P(C.c_int64), P(C.c_int64)]
        L.gi_accum_add_tiles.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, P(C.c_int64),
                                         P(RenderStats)]
        L.gi_accum_add_adaptive.argtypes = [C.c_void_p, C.c_int, P(AdaptiveParams), C.c_void_p,
                                            P(C.c_int64), P(RenderStats)]
        L.gi_adaptive_bench.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        P(C.c_double), P(C.c_double), P(C.c_double)]
        L.gi_vdenoise_params_default.argtypes = [P(VDenoiseParams)]
        L.gi_vdenoise_params_default.restype = None
        L.gi_denoise_radiance.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, P(VDenoiseParams), C.c_void_p, C.c_void_p,
                                          P(C.c_double)]
        L.gi_accum_denoise.argtypes = [C.c_void_p, C.c_void_p, P(VDenoiseParams), C.c_void_p,
                                       C.c_void_p, P(C.c_double)]
        L.gi_get_view.argtypes = [C.c_void_p, P(View)]
        L.gi_reproject_params_default.argtypes = [P(ReprojectParams)]
        L.gi_reproject_params_default.restype = None
        L.gi_accum_reproject.argtypes = [C.c_void_p, P(View), C.c_void_p, C.c_void_p,
                                         P(ReprojectParams), P(ReprojectStats), P(C.c_double)]
        L.gi_accum_export.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.gi_accum_import.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.gi_accum_merge.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.gi_accum_export_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, P(C.c_int64)]
        L.gi_accum_merge_packed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                            P(C.c_double)]
        L.gi_accum_merge_from.argtypes = [C.c_void_p, C.c_void_p, P(C.c_double)]
        L.gi_progressive_params_default.argtypes = [P(ProgressiveParams)]
        L.gi_progressive_params_default.restype = None
        L.gi_progressive_radius.argtypes = [C.c_double, C.c_double, C.c_int64]
        L.gi_progressive_radius.restype = C.c_double
        L.gi_accum_add_progressive.argtypes = [C.c_void_p, C.c_int, C.c_int64,
                                               P(ProgressiveParams), P(PhotonStats),
                                               P(RenderStats)]
        L.gi_tonemap.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                 C.c_double, C.c_void_p, C.c_void_p]
        L.gi_radiance_bench.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        P(C.c_double), P(C.c_double), P(C.c_double)]
        L.gi_write_image_float.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p]
        L.gi_estimate_radiance_batch.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
        L.gi_knn_batch.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int,
                                   C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gi_knn_bench.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_int, C.c_int, C.c_int, P(C.c_double),
                                   P(C.c_double), P(C.c_double)]
        L.gi_release_scratch.argtypes = [C.c_void_p]
        L.gi_math_probe.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_void_p]
        L.gi_intersect_batch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
        L.gi_intersect_probe.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int] + [C.c_void_p] * 6
        L.gi_illum_probe.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.gi_scene_triangle_planes.argtypes = [C.c_void_p, C.c_int64, C.c_void_p,
                                               P(C.c_int64)]
        L.gi_scene_slab_boxes.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, P(C.c_int64)]
        L.gi_write_image.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p]
        _lib = L
    return _lib


def default_params():
    p = GiParams()
    lib().gi_params_default(C.byref(p))
    return p


def default_denoise_params():
    p = DenoiseParams()
    lib().gi_denoise_params_default(C.byref(p))
    return p


def default_vdenoise_params(**kw):
    """gi_vdenoise_params: the defaults (gi_vdenoise_params_default) with the given fields set."""
    p = VDenoiseParams()
    lib().gi_vdenoise_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(VDenoiseParams._fields_):
            raise TypeError(f"unknown vdenoise parameter {k}")
        setattr(p, k, v)
    return p


def reproject_params(**kw):
    """gi_reproject_params: the defaults (gi_reproject_params_default) with the given fields set."""
    p = ReprojectParams()
    lib().gi_reproject_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(ReprojectParams._fields_):
            raise TypeError(f"unknown reproject parameter {k}")
        setattr(p, k, v)
    return p


def adaptive_params(**kw):
    """gi_adaptive_params: the defaults (gi_adaptive_params_default) with the given fields set."""
    p = AdaptiveParams()
    lib().gi_adaptive_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(AdaptiveParams._fields_):
            raise TypeError(f"unknown adaptive parameter {k}")
        setattr(p, k, v)
    return p


def progressive_params(**kw):
    """gi_progressive_params: the defaults (gi_progressive_params_default) with the given fields
    set."""
    p = ProgressiveParams()
    lib().gi_progressive_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(ProgressiveParams._fields_):
            raise TypeError(f"unknown progressive parameter {k}")
        setattr(p, k, v)
    return p


def progressive_radius(r0, alpha, npass):
    """The radius of progressive pass `npass` (0-based) from r0 (gi_progressive_radius); NaN for
    a bad argument."""
    return lib().gi_progressive_radius(float(r0), float(alpha), int(npass))


def ParseArgs(argv):
    """Return (params, scene, output, width, height, aa, real_material); raises ValueError with
    the reference's message on a bad flag (io_utils.cpp:186-188)."""
    p = default_params()
    args = ["photonmap"] + list(argv)
    arr = (C.c_char_p * len(args))(*[a.encode() for a in args])
    scene, out, err = C.c_char_p(), C.c_char_p(), C.c_char_p()
    w, h, aa, real = C.c_int(1024), C.c_int(1024), C.c_int(2), C.c_int(0)
    rc = lib().gi_parse_args(len(args), arr, C.byref(p), C.byref(scene), C.byref(out),
                             C.byref(w), C.byref(h), C.byref(aa), C.byref(real), C.byref(err))
    if rc != GI_OK:
        raise ValueError(err.value.decode() if err.value else f"gi_parse_args rc={rc}")
    return p, scene.value.decode(), out.value.decode(), w.value, h.value, aa.value, real.value


class GiError(RuntimeError):
    pass


class Renderer:
    """One context: scene, photon maps and render scratch on one HIP device, or on a device
    set (`devices=[...]`, gi_create_devices: tiles dealt across the devices, gathered onto the
    first)."""

    def __init__(self, device=0, params=None, devices=None):
        self._ctx = C.c_void_p()
        if devices is not None:
            ds = DeviceSet()
            ds.count = len(devices)
            for i, d in enumerate(devices):
                ds.devices[i] = d
            rc = lib().gi_create_devices(C.byref(self._ctx), C.byref(ds))
            if rc != GI_OK:
                raise GiError(f"gi_create_devices failed (rc={rc}) for devices {list(devices)}")
        else:
            rc = lib().gi_create(C.byref(self._ctx), device)
            if rc != GI_OK:
                raise GiError(f"gi_create failed (rc={rc}): no usable HIP device {device}")
        self.params = params if params is not None else default_params()
        self._check(lib().gi_set_params(self._ctx, C.byref(self.params)))

    def device_info(self):
        """What the context drives (gi_device_info): HIP ordinals, PCI bus ids, RCCL user rank
        per device, and the RCCL communicator's rank count (0 without RCCL)."""
        n = C.c_int(0)
        self._check(lib().gi_device_info(self._ctx, 0, C.byref(n), None, None, None, None))
        k = n.value
        dev, bus, rk = (C.c_int * k)(), (C.c_int * k)(), (C.c_int * k)()
        cc = C.c_int(0)
        self._check(lib().gi_device_info(self._ctx, k, C.byref(n), dev, bus, rk, C.byref(cc)))
        return {"devices": list(dev), "pci_bus": list(bus), "comm_rank": list(rk),
                "comm_count": cc.value}

    def release_scratch(self):
        """Free the device scratch of renders and map builds; scene and maps stay resident."""
        self._check(lib().gi_release_scratch(self._ctx))

    def close(self):
        if self._ctx:
            lib().gi_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != GI_OK:
            msg = lib().gi_last_error(self._ctx)
            raise GiError(f"rc={rc}: {msg.decode() if msg else ''}")

    def set_params(self, params):
        self.params = params
        self._check(lib().gi_set_params(self._ctx, C.byref(params)))

    def ReadScene(self, path, real_material=False):
        self._check(lib().gi_read_scene(self._ctx, path.encode(), int(real_material)))
        nn, nl, npr, r = C.c_int(), C.c_int(), C.c_int(), C.c_double()
        self._check(lib().gi_scene_info(self._ctx, C.byref(nn), C.byref(nl), C.byref(npr),
                                        C.byref(r)))
        return {"nodes": nn.value, "lights": nl.value, "shapes": npr.value, "radius": r.value}

    def MapPhotons(self):
        st = PhotonStats()
        self._check(lib().gi_map_photons(self._ctx, C.byref(st)))
        return {f: getattr(st, f) for f, _ in PhotonStats._fields_}

    def photon_map(self, which):
        n = C.c_int64()
        self._check(lib().gi_get_photon_map(self._ctx, which, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=PHOTON_DTYPE)
        self._check(lib().gi_get_photon_map(self._ctx, which, out.ctypes.data, n.value,
                                            C.byref(n)))
        return out

    def kd_tree(self, which):
        """(nodes [2L, 8] float32, perm [n] int32 kd position -> emission index, nleaves)"""
        nl, n = C.c_int32(), C.c_int64()
        self._check(lib().gi_get_kd_tree(self._ctx, which, None, 0, None, 0, C.byref(nl), C.byref(n)))
        nodes = np.zeros((2 * nl.value, 8), dtype=np.float32)
        perm = np.zeros(n.value, dtype=np.int32)
        self._check(lib().gi_get_kd_tree(self._ctx, which, nodes.ctypes.data, nodes.size,
                                         perm.ctypes.data, n.value, C.byref(nl), C.byref(n)))
        return nodes, perm, nl.value

    def set_photon_map(self, which, photons):
        photons = np.ascontiguousarray(photons, dtype=PHOTON_DTYPE)
        self._check(lib().gi_set_photon_map(self._ctx, which, photons.ctypes.data, len(photons)))

    def RenderImage(self, aa, width, height, want_float=False):
        rgb = np.zeros((height, width, 3), dtype=np.uint8)
        rgbf = np.zeros((height, width, 3), dtype=np.float32) if want_float else None
        st = RenderStats()
        self._check(lib().gi_render_image(self._ctx, aa, width, height, rgb.ctypes.data,
                                          rgbf.ctypes.data if want_float else None,
                                          C.byref(st)))
        stats = _stats_dict(st)
        return (rgb, rgbf, stats) if want_float else (rgb, stats)

    def get_camera(self):
        """(eye, towards, up, xfov) the context renders from, as given by the scene file or the
        last set_camera (tuples of floats; gi_get_camera)."""
        cam = Camera()
        self._check(lib().gi_get_camera(self._ctx, C.byref(cam)))
        return tuple(cam.eye), tuple(cam.towards), tuple(cam.up), cam.xfov

    def set_camera(self, eye, towards, up, xfov):
        """Render from another camera; scene, photon maps and kd trees stay (gi_set_camera)."""
        cam = Camera()
        for i in range(3):
            cam.eye[i], cam.towards[i], cam.up[i] = float(eye[i]), float(towards[i]), float(up[i])
        cam.xfov = float(xfov)
        self._check(lib().gi_set_camera(self._ctx, C.byref(cam)))

    def camera_rays(self, aa, width, height):
        """The primary rays RenderImage(aa, width, height) traces and their RNG stream ids
        (gi_camera_rays): (rays [n] RAY_DTYPE, ids [n] uint64), pixels row-major from the bottom
        row, a pixel's 4^aa * dof_test samples together."""
        n = C.c_int64(0)
        self._check(lib().gi_camera_rays(self._ctx, aa, width, height, None, None, 0, C.byref(n)))
        rays = np.zeros(n.value, dtype=RAY_DTYPE)
        ids = np.zeros(n.value, dtype=np.uint64)
        self._check(lib().gi_camera_rays(self._ctx, aa, width, height, rays.ctypes.data,
                                         ids.ctypes.data, n.value, C.byref(n)))
        return rays, ids

    def _ray_batch(self, width, height, spp, rays, ids):
        """Contiguous rays and ids of a width x height x spp batch, lengths checked."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE).ravel()
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.uint64).ravel()
        need = width * height * spp
        if spp >= 1 and (len(rays) != need or (ids is not None and len(ids) != need)):
            raise ValueError(f"{need} rays expected (width * height * spp), got {len(rays)}")
        return rays, ids

    def render_rays(self, width, height, spp, rays, ids=None, want_float=False):
        """Render caller-made primary rays, spp per output pixel (gi_render_rays); returns like
        RenderImage. ids: RNG stream id per ray (default: the ray's index)."""
        rays, ids = self._ray_batch(width, height, spp, rays, ids)
        rgb = np.zeros((height, width, 3), dtype=np.uint8)
        rgbf = np.zeros((height, width, 3), dtype=np.float32) if want_float else None
        st = RenderStats()
        self._check(lib().gi_render_rays(self._ctx, width, height, spp, rays.ctypes.data,
                                         None if ids is None else ids.ctypes.data,
                                         rgb.ctypes.data,
                                         rgbf.ctypes.data if want_float else None, C.byref(st)))
        stats = _stats_dict(st)
        return (rgb, rgbf, stats) if want_float else (rgb, stats)

    def materials(self):
        """The scene's materials as the device holds them, indexed by Intersects' material
        value (gi_get_materials): [n] MATERIAL_DTYPE."""
        n = C.c_int32(0)
        self._check(lib().gi_get_materials(self._ctx, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=MATERIAL_DTYPE)
        self._check(lib().gi_get_materials(self._ctx, out.ctypes.data, n.value, C.byref(n)))
        return out

    def camera_features(self, aa, width, height):
        """Feature planes of the frame RenderImage(aa, width, height) renders
        (gi_camera_features): [height, width] FEATURE_DTYPE, row 0 = bottom."""
        out = np.zeros((height, width), dtype=FEATURE_DTYPE)
        self._check(lib().gi_camera_features(self._ctx, aa, width, height, out.ctypes.data))
        return out

    def ray_features(self, width, height, spp, rays):
        """Feature planes of a caller-made ray batch, spp rays per pixel as in render_rays
        (gi_ray_features): [height, width] FEATURE_DTYPE."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE).ravel()
        need = width * height * spp
        if spp >= 1 and len(rays) != need:
            raise ValueError(f"{need} rays expected (width * height * spp), got {len(rays)}")
        out = np.zeros((height, width), dtype=FEATURE_DTYPE)
        self._check(lib().gi_ray_features(self._ctx, width, height, spp, rays.ctypes.data,
                                          out.ctypes.data))
        return out

    def denoise(self, rgbf, feat, want_float=False, **params):
        """Edge-avoiding a-trous filter of a float frame [H, W, 3] by its planes [H, W]
        (gi_denoise); params: fields of gi_denoise_params that differ from the defaults.
        Returns (rgb8, kernel_ms), or (rgb8, rgbf, kernel_ms) with want_float."""
        rgbf = np.ascontiguousarray(rgbf, dtype=np.float32)
        feat = np.ascontiguousarray(feat, dtype=FEATURE_DTYPE)
        h, w = feat.shape
        if rgbf.shape != (h, w, 3):
            raise ValueError(f"image {rgbf.shape} does not match planes {feat.shape}")
        p = default_denoise_params()
        for k, v in params.items():
            if k not in dict(DenoiseParams._fields_):
                raise TypeError(f"unknown denoise parameter {k}")
            setattr(p, k, v)
        rgb = np.zeros((h, w, 3), dtype=np.uint8)
        out = np.zeros((h, w, 3), dtype=np.float32)
        ms = C.c_double(0.0)
        self._check(lib().gi_denoise(self._ctx, w, h, rgbf.ctypes.data, feat.ctypes.data,
                                     C.byref(p), out.ctypes.data, rgb.ctypes.data, C.byref(ms)))
        return (rgb, out, ms.value) if want_float else (rgb, ms.value)

    def render_radiance(self, aa, width, height, want_samples=False):
        """Unclamped frame of RenderImage(aa, width, height) (gi_render_radiance): (mean
        [H, W, 3] float32, variance of the mean [H, W, 3] float32, stats), or with want_samples
        (mean, variance, samples [H, W, 4^aa, 3] float64, stats)."""
        S = 4 ** aa if 0 <= aa <= 15 else 1
        mean = np.zeros((height, width, 3), dtype=np.float32)
        var = np.zeros((height, width, 3), dtype=np.float32)
        smp = np.zeros((height, width, S, 3), dtype=np.float64) if want_samples else None
        st = RenderStats()
        self._check(lib().gi_render_radiance(self._ctx, aa, width, height, mean.ctypes.data,
                                             var.ctypes.data,
                                             smp.ctypes.data if want_samples else None,
                                             C.byref(st)))
        stats = _stats_dict(st)
        return (mean, var, smp, stats) if want_samples else (mean, var, stats)

    def render_rays_radiance(self, width, height, spp, rays, ids=None, want_samples=False):
        """Unclamped frame of a caller-made ray batch, spp rays per pixel as in render_rays
        (gi_render_rays_radiance); returns like render_radiance, samples [H, W, spp, 3]."""
        rays, ids = self._ray_batch(width, height, spp, rays, ids)
        mean = np.zeros((height, width, 3), dtype=np.float32)
        var = np.zeros((height, width, 3), dtype=np.float32)
        smp = (np.zeros((height, width, max(spp, 1), 3), dtype=np.float64) if want_samples
               else None)
        st = RenderStats()
        self._check(lib().gi_render_rays_radiance(
            self._ctx, width, height, spp, rays.ctypes.data,
            None if ids is None else ids.ctypes.data, mean.ctypes.data, var.ctypes.data,
            smp.ctypes.data if want_samples else None, C.byref(st)))
        stats = _stats_dict(st)
        return (mean, var, smp, stats) if want_samples else (mean, var, stats)

    def render_layers(self, aa, width, height, want_samples=False):
        """render_radiance with LAYER_COUNT + 1 planes per output (gi_render_layers): mean and
        variance [6, H, W, 3] float32, samples [6, H, W, 4^aa, 3] float64; plane l < LAYER_COUNT
        is light-path layer l (LAYER_NAMES), plane LAYER_TOTAL what render_radiance returns."""
        S = 4 ** aa if 0 <= aa <= 15 else 1
        n = LAYER_COUNT + 1
        mean = np.zeros((n, height, width, 3), dtype=np.float32)
        var = np.zeros((n, height, width, 3), dtype=np.float32)
        smp = np.zeros((n, height, width, S, 3), dtype=np.float64) if want_samples else None
        st = RenderStats()
        self._check(lib().gi_render_layers(self._ctx, aa, width, height, mean.ctypes.data,
                                           var.ctypes.data,
                                           smp.ctypes.data if want_samples else None, C.byref(st)))
        stats = _stats_dict(st)
        return (mean, var, smp, stats) if want_samples else (mean, var, stats)

    def render_rays_layers(self, width, height, spp, rays, ids=None, want_samples=False):
        """render_rays_radiance with LAYER_COUNT + 1 planes per output (gi_render_rays_layers);
        returns like render_layers, samples [6, H, W, spp, 3]."""
        rays, ids = self._ray_batch(width, height, spp, rays, ids)
        n = LAYER_COUNT + 1
        mean = np.zeros((n, height, width, 3), dtype=np.float32)
        var = np.zeros((n, height, width, 3), dtype=np.float32)
        smp = (np.zeros((n, height, width, max(spp, 1), 3), dtype=np.float64) if want_samples
               else None)
        st = RenderStats()
        self._check(lib().gi_render_rays_layers(
            self._ctx, width, height, spp, rays.ctypes.data,
            None if ids is None else ids.ctypes.data, mean.ctypes.data, var.ctypes.data,
            smp.ctypes.data if want_samples else None, C.byref(st)))
        stats = _stats_dict(st)
        return (mean, var, smp, stats) if want_samples else (mean, var, stats)

    @staticmethod
    def _layer_list(layers):
        """The C array of a layered pass: LAYER_COUNT Renderers (on this device, accumulators of
        this one's size), None dropping a layer."""
        layers = list(layers)
        if len(layers) != LAYER_COUNT:
            raise ValueError(f"{LAYER_COUNT} layer contexts (or None) expected, got {len(layers)}")
        return (C.c_void_p * LAYER_COUNT)(*[None if r is None else r._ctx for r in layers])

    def accum_add_image_layers(self, aa, layers):
        """accum_add_image that also folds light-path layer l of the pass into the accumulator of
        layers[l] (gi_accum_add_image_layers). Returns the pass's stats."""
        st = RenderStats()
        self._check(lib().gi_accum_add_image_layers(self._ctx, aa, self._layer_list(layers),
                                                    C.byref(st)))
        return _stats_dict(st)

    def accum_add_rays_layers(self, spp, rays, layers, ids=None):
        """accum_add_rays with the layers folded as in accum_add_image_layers
        (gi_accum_add_rays_layers)."""
        w, h = getattr(self, "_accum_size", (0, 0))
        if w:
            rays, ids = self._ray_batch(w, h, spp, rays, ids)
        else:  # no reset yet: the library reports it
            rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE).ravel()
            ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint64).ravel()
        st = RenderStats()
        self._check(lib().gi_accum_add_rays_layers(self._ctx, spp, rays.ctypes.data,
                                                   None if ids is None else ids.ctypes.data,
                                                   self._layer_list(layers), C.byref(st)))
        return _stats_dict(st)

    def layers_timing(self, on):
        """Switch the HIP-event timing of the layer reduction's kernel on or off
        (gi_layers_timing); returns the ms summed since it was last switched on."""
        ms = C.c_double(0.0)
        self._check(lib().gi_layers_timing(self._ctx, int(bool(on)), C.byref(ms)))
        return ms.value

    def accum_reset(self, width, height):
        """Size and empty the context's accumulator over passes (gi_accum_reset)."""
        self._check(lib().gi_accum_reset(self._ctx, width, height))
        self._accum_size = (width, height)

    def accum_add_image(self, aa):
        """Render one camera pass under the current parameters and fold it into the accumulator
        (gi_accum_add_image); change params.seed with set_params between passes: the photon maps
        stay. Returns the pass's stats."""
        st = RenderStats()
        self._check(lib().gi_accum_add_image(self._ctx, aa, C.byref(st)))
        return _stats_dict(st)

    def accum_add_progressive(self, aa, npass, params=None, **kw):
        """Progressive photon-map pass `npass` (0-based) into the accumulator
        (gi_accum_add_progressive): fresh maps under seed + npass, fixed-radius estimates at the
        pass's radii. Returns (photon stats, render stats)."""
        p = params if params is not None else progressive_params(**kw)
        pst, st = PhotonStats(), RenderStats()
        self._check(lib().gi_accum_add_progressive(self._ctx, aa, npass, C.byref(p),
                                                   C.byref(pst), C.byref(st)))
        return {f: getattr(pst, f) for f, _ in PhotonStats._fields_}, _stats_dict(st)

    def accum_add_rays(self, spp, rays, ids=None):
        """Render one ray pass of the accumulator's size and fold it in (gi_accum_add_rays); give
        other ids for every pass."""
        w, h = getattr(self, "_accum_size", (0, 0))
        if w:
            rays, ids = self._ray_batch(w, h, spp, rays, ids)
        else:  # no reset yet: the library reports it
            rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE).ravel()
            ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint64).ravel()
        st = RenderStats()
        self._check(lib().gi_accum_add_rays(self._ctx, spp, rays.ctypes.data,
                                            None if ids is None else ids.ctypes.data,
                                            C.byref(st)))
        return _stats_dict(st)

    def accum_get(self):
        """(mean [H, W, 3] float32, variance of the mean [H, W, 3] float32, samples per pixel N,
        noise: the frame's mean relative standard error of luminance) of the accumulator
        (gi_accum_get)."""
        w, h = getattr(self, "_accum_size", (0, 0))
        mean = np.zeros((h, w, 3), dtype=np.float32)
        var = np.zeros((h, w, 3), dtype=np.float32)
        n, noise = C.c_int64(0), C.c_double(0.0)
        self._check(lib().gi_accum_get(self._ctx, mean.ctypes.data if w else None,
                                       var.ctypes.data if w else None, C.byref(n),
                                       C.byref(noise)))
        return mean, var, n.value, noise.value

    def accum_get_counts(self):
        """(per-pixel sample counts [H, W] int64, their sum) of the accumulator
        (gi_accum_get_counts)."""
        w, h = getattr(self, "_accum_size", (0, 0))
        counts = np.zeros((h, w), dtype=np.int64)
        total = C.c_int64(0)
        self._check(lib().gi_accum_get_counts(self._ctx, counts.ctypes.data if w else None,
                                              C.byref(total)))
        return counts, total.value

    def accum_export(self):
        """(state [H, W, 6] float64: {mu.rgb, A.rgb}, counts [H, W] int64) of the accumulator, the
        device's own bits (gi_accum_export)."""
        w, h = getattr(self, "_accum_size", (0, 0))
        state = np.zeros((h, w, 6), dtype=np.float64)
        counts = np.zeros((h, w), dtype=np.int64)
        self._check(lib().gi_accum_export(self._ctx, state.ctypes.data if w else None,
                                          counts.ctypes.data if w else None))
        return state, counts

    @staticmethod
    def _host_state(state, counts):
        state = np.ascontiguousarray(state, dtype=np.float64)
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        if state.ndim != 3 or state.shape[2] != 6 or counts.shape != state.shape[:2]:
            raise ValueError(f"state {state.shape} / counts {counts.shape} are not [H, W, 6] / [H, W]")
        return state, counts

    def accum_import(self, state, counts):
        """Replace the accumulator by a state as accum_export returns it (gi_accum_import);
        needs no scene and no reset."""
        state, counts = self._host_state(state, counts)
        h, w = counts.shape
        self._check(lib().gi_accum_import(self._ctx, w, h, state.ctypes.data, counts.ctypes.data))
        self._accum_size = (w, h)

    def accum_merge(self, state, counts):
        """Fold a state of the accumulator's size into it (gi_accum_merge)."""
        state, counts = self._host_state(state, counts)
        h, w = counts.shape
        self._check(lib().gi_accum_merge(self._ctx, w, h, state.ctypes.data, counts.ctypes.data))

    def accum_state_bytes(self):
        """Bytes of the packed state (gi_accum_export_packed with a null buffer)."""
        n = C.c_int64(0)
        self._check(lib().gi_accum_export_packed(self._ctx, None, 0, C.byref(n)))
        return n.value

    def accum_export_packed(self, dev_ptr, capacity_bytes):
        """The packed state into device memory at dev_ptr (on this renderer's device); returns its
        bytes (gi_accum_export_packed)."""
        n = C.c_int64(0)
        self._check(lib().gi_accum_export_packed(self._ctx, dev_ptr, capacity_bytes, C.byref(n)))
        return n.value

    def accum_merge_packed(self, nstates, dev_ptr, stride_bytes):
        """Fold nstates packed states at dev_ptr (device memory, stride_bytes apart) into the
        accumulator in order, in one launch (gi_accum_merge_packed); returns its HIP-event ms."""
        ms = C.c_double(0.0)
        self._check(lib().gi_accum_merge_packed(self._ctx, nstates, dev_ptr, stride_bytes,
                                                C.byref(ms)))
        return ms.value

    def accum_merge_from(self, other):
        """Fold another renderer's accumulator (same size, on any device) into this one; the
        other is left unchanged (gi_accum_merge_from). Returns the fold's HIP-event ms."""
        ms = C.c_double(0.0)
        self._check(lib().gi_accum_merge_from(self._ctx, other._ctx, C.byref(ms)))
        return ms.value

    def _tiles(self, tile_px):
        w, h = getattr(self, "_accum_size", (0, 0))
        t = max(1, int(tile_px))
        return ((w + t - 1) // t) * ((h + t - 1) // t)

    def accum_select(self, params=None, **kw):
        """The tiles an adaptive pass would refine (gi_accum_select): (mask [tiles] uint8,
        tile_error [tiles] float64, active tiles, active pixels). params: AdaptiveParams, or the
        defaults with the keyword fields set."""
        p = params if params is not None else adaptive_params(**kw)
        nt = self._tiles(p.tile_px)
        mask = np.zeros(nt, dtype=np.uint8)
        err = np.zeros(nt, dtype=np.float64)
        at, ap = C.c_int64(0), C.c_int64(0)
        self._check(lib().gi_accum_select(self._ctx, C.byref(p), mask.ctypes.data,
                                          err.ctypes.data, C.byref(at), C.byref(ap)))
        return mask, err, at.value, ap.value

    def accum_add_tiles(self, aa, tile_px, mask):
        """One camera pass over the tiles with mask != 0, folded into their pixels only
        (gi_accum_add_tiles). Returns (active pixels, stats)."""
        mask = np.ascontiguousarray(mask, dtype=np.uint8).ravel()
        if 4 <= tile_px <= 64 and getattr(self, "_accum_size", None) \
                and mask.size != self._tiles(tile_px):
            raise ValueError(f"{self._tiles(tile_px)} tiles expected, got {mask.size}")
        st = RenderStats()
        ap = C.c_int64(0)
        self._check(lib().gi_accum_add_tiles(self._ctx, aa, tile_px, mask.ctypes.data,
                                             C.byref(ap), C.byref(st)))
        return ap.value, _stats_dict(st)

    def accum_add_adaptive(self, aa, params=None, **kw):
        """Select and refine in one call (gi_accum_add_adaptive). Returns (mask [tiles] uint8,
        active pixels, stats)."""
        p = params if params is not None else adaptive_params(**kw)
        mask = np.zeros(self._tiles(p.tile_px), dtype=np.uint8)
        st = RenderStats()
        ap = C.c_int64(0)
        self._check(lib().gi_accum_add_adaptive(self._ctx, aa, C.byref(p), mask.ctypes.data,
                                                C.byref(ap), C.byref(st)))
        return mask, ap.value, _stats_dict(st)

    def adaptive_bench(self, width, height, tile_px=8, warmup=5, reps=50):
        """Median HIP-event ms of the tile selection, the masked fold at half the tiles and the
        whole-frame fold on a synthetic frame (diagnostics; gi_adaptive_bench)."""
        t = [C.c_double(0.0) for _ in range(3)]
        self._check(lib().gi_adaptive_bench(self._ctx, width, height, tile_px, warmup, reps,
                                            C.byref(t[0]), C.byref(t[1]), C.byref(t[2])))
        return {"select_ms": t[0].value, "masked_merge_ms": t[1].value,
                "accum_merge_ms": t[2].value}

    def denoise_radiance(self, mean, variance, feat, **params):
        """Variance-guided a-trous filter of a radiance frame (gi_denoise_radiance): mean and
        variance of the mean [H, W, 3] as render_radiance / accum_get return them, feat [H, W];
        params: fields of gi_vdenoise_params that differ from the defaults. Returns (filtered
        mean [H, W, 3] float32, filtered luminance variance [H, W] float32, kernel_ms)."""
        mean = np.ascontiguousarray(mean, dtype=np.float32)
        variance = np.ascontiguousarray(variance, dtype=np.float32)
        feat = np.ascontiguousarray(feat, dtype=FEATURE_DTYPE)
        h, w = feat.shape
        if mean.shape != (h, w, 3) or variance.shape != (h, w, 3):
            raise ValueError(f"frames {mean.shape}, {variance.shape} do not match planes "
                             f"{feat.shape}")
        p = default_vdenoise_params(**params)
        out = np.zeros((h, w, 3), dtype=np.float32)
        vlum = np.zeros((h, w), dtype=np.float32)
        ms = C.c_double(0.0)
        self._check(lib().gi_denoise_radiance(self._ctx, w, h, mean.ctypes.data,
                                              variance.ctypes.data, feat.ctypes.data, C.byref(p),
                                              out.ctypes.data, vlum.ctypes.data, C.byref(ms)))
        return out, vlum, ms.value

    def accum_denoise(self, feat, **params):
        """The same filter of the accumulator as it stands, read on the device and left
        unchanged (gi_accum_denoise); feat: the planes of the accumulator's frame. Returns like
        denoise_radiance."""
        feat = np.ascontiguousarray(feat, dtype=FEATURE_DTYPE)
        w, h = getattr(self, "_accum_size", (0, 0))
        if w and feat.shape != (h, w):
            raise ValueError(f"planes {feat.shape} do not match the accumulator's {(h, w)}")
        p = default_vdenoise_params(**params)
        out = np.zeros(feat.shape + (3,), dtype=np.float32)
        vlum = np.zeros(feat.shape, dtype=np.float32)
        ms = C.c_double(0.0)
        self._check(lib().gi_accum_denoise(self._ctx, feat.ctypes.data, C.byref(p),
                                           out.ctypes.data, vlum.ctypes.data, C.byref(ms)))
        return out, vlum, ms.value

    def get_view(self):
        """The pinhole frame the device renders from under the current camera and focus_depth
        (gi_get_view): a View; save it before set_camera to name the previous camera later."""
        v = View()
        self._check(lib().gi_get_view(self._ctx, C.byref(v)))
        return v

    def accum_reproject(self, prev_view, prev_feat, cur_feat, params=None, **kw):
        """Carry the accumulator from prev_view (a View; prev_feat its frame's planes) into the
        current camera (cur_feat: the planes of the same frame now) (gi_accum_reproject). params:
        ReprojectParams, or the defaults with the keyword fields set. Returns (stats dict:
        kept_pixels, reset_pixels, kept_samples; kernel_ms)."""
        prev_feat = np.ascontiguousarray(prev_feat, dtype=FEATURE_DTYPE)
        cur_feat = np.ascontiguousarray(cur_feat, dtype=FEATURE_DTYPE)
        w, h = getattr(self, "_accum_size", (0, 0))
        if w and (prev_feat.shape != (h, w) or cur_feat.shape != (h, w)):
            raise ValueError(f"planes {prev_feat.shape}, {cur_feat.shape} do not match the "
                             f"accumulator's {(h, w)}")
        p = params if params is not None else reproject_params(**kw)
        st = ReprojectStats()
        ms = C.c_double(0.0)
        self._check(lib().gi_accum_reproject(self._ctx, C.byref(prev_view),
                                             prev_feat.ctypes.data, cur_feat.ctypes.data,
                                             C.byref(p), C.byref(st), C.byref(ms)))
        return {f: getattr(st, f) for f, _ in ReprojectStats._fields_}, ms.value

    def tonemap(self, radiance, exposure=1.0, white=0.0, want_float=False):
        """Exposure, extended Reinhard curve (white > 0; 0: linear) and clamp of a radiance frame
        [H, W, 3] (gi_tonemap). Returns rgb8, or (rgb8, rgbf) with want_float."""
        radiance = np.ascontiguousarray(radiance, dtype=np.float32)
        if radiance.ndim != 3 or radiance.shape[2] != 3:
            raise ValueError(f"[H, W, 3] frame expected, got {radiance.shape}")
        h, w, _ = radiance.shape
        rgb = np.zeros((h, w, 3), dtype=np.uint8)
        out = np.zeros((h, w, 3), dtype=np.float32)
        self._check(lib().gi_tonemap(self._ctx, w, h, radiance.ctypes.data, exposure, white,
                                     out.ctypes.data, rgb.ctypes.data))
        return (rgb, out) if want_float else rgb

    def radiance_bench(self, aa, width, height, warmup=5, reps=50):
        """Median HIP-event ms of the radiance reduction, the accumulator merge and the noise
        reduction on a synthetic frame (diagnostics; gi_radiance_bench)."""
        t = [C.c_double(0.0) for _ in range(3)]
        self._check(lib().gi_radiance_bench(self._ctx, aa, width, height, warmup, reps,
                                            C.byref(t[0]), C.byref(t[1]), C.byref(t[2])))
        return {"reduce_radiance_ms": t[0].value, "accum_merge_ms": t[1].value,
                "accum_noise_ms": t[2].value}

    def render_tiles(self, aa, width, height, tile, shard, nshards, rgbf=None):
        if rgbf is None:
            rgbf = np.zeros((height, width, 3), dtype=np.float32)
        st = RenderStats()
        self._check(lib().gi_render_tiles(self._ctx, aa, width, height, tile, shard, nshards,
                                          rgbf.ctypes.data, C.byref(st)))
        return rgbf, _stats_dict(st)

    def shard_pixels(self, width, height, tile, shard, nshards):
        """Pixels of one tile shard (gi_render_tiles_packed with a null buffer)."""
        n = C.c_int64(0)
        self._check(lib().gi_render_tiles_packed(self._ctx, 0, width, height, tile, shard,
                                                 nshards, None, 0, C.byref(n), None))
        return n.value

    def render_tiles_packed(self, aa, width, height, tile, shard, nshards, dev_ptr, capacity):
        """Render a tile shard into a device buffer (`dev_ptr`, 16 B per pixel, e.g. the
        data_ptr() of a CUDA tensor on this context's device). Returns (pixels, stats)."""
        n = C.c_int64(0)
        st = RenderStats()
        self._check(lib().gi_render_tiles_packed(self._ctx, aa, width, height, tile, shard,
                                                 nshards, C.c_void_p(dev_ptr), capacity,
                                                 C.byref(n), C.byref(st)))
        return n.value, _stats_dict(st)

    def compose_tiles(self, width, height, tile, nshards, dev_ptr, stride, want_float=False):
        """Full frame from nshards packed shard buffers at dev_ptr (device, stride pixels
        apart). Returns rgb8 [, rgbf]."""
        rgb = np.zeros((height, width, 3), dtype=np.uint8)
        rgbf = np.zeros((height, width, 3), dtype=np.float32) if want_float else None
        self._check(lib().gi_compose_tiles(self._ctx, width, height, tile, nshards,
                                           C.c_void_p(dev_ptr), stride, rgb.ctypes.data,
                                           rgbf.ctypes.data if want_float else None))
        return (rgb, rgbf) if want_float else rgb

    def EstimateRadiance(self, which, queries):
        q = np.ascontiguousarray(queries, dtype=QUERY_DTYPE)
        n = len(q)
        out = np.zeros((n, 3), dtype=np.float64)
        nf = np.zeros(n, dtype=np.int32)
        md = np.zeros(n, dtype=np.float32)
        self._check(lib().gi_estimate_radiance_batch(self._ctx, which, n, q.ctypes.data,
                                                     out.ctypes.data, nf.ctypes.data,
                                                     md.ctypes.data))
        return out, nf, md

    def FindClosestQuick(self, which, points, k, max_dist):
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = len(pts)
        idx = np.zeros((n, k), dtype=np.int32)
        d2 = np.zeros((n, k), dtype=np.float32)
        nf = np.zeros(n, dtype=np.int32)
        self._check(lib().gi_knn_batch(self._ctx, which, n, pts.ctypes.data, k, max_dist,
                                       idx.ctypes.data, d2.ctypes.data, nf.ctypes.data))
        return idx, d2, nf

    def knn_bench(self, which, points, normals=None, materials=None, mode=0, kernel=-1,
                  iters=3):
        """Time the k-NN estimate kernel on resident queries (diagnostics; gi_knn_bench)."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float64)
        mat = None if materials is None else np.ascontiguousarray(materials, dtype=np.int32)
        ms, fq, vq = C.c_double(), C.c_double(), C.c_double()
        self._check(lib().gi_knn_bench(
            self._ctx, which, len(pts), pts.ctypes.data,
            None if nrm is None else nrm.ctypes.data, None if mat is None else mat.ctypes.data,
            mode, kernel, iters, C.byref(ms), C.byref(fq), C.byref(vq)))
        return ms.value, fq.value, vq.value

    def Intersects(self, org, dirs):
        org = np.ascontiguousarray(org, dtype=np.float64).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        n = len(org)
        hit = np.zeros(n, dtype=np.int32)
        t = np.zeros(n, dtype=np.float64)
        p = np.zeros((n, 3), dtype=np.float64)
        nr = np.zeros((n, 3), dtype=np.float64)
        m = np.zeros(n, dtype=np.int32)
        self._check(lib().gi_intersect_batch(self._ctx, n, org.ctypes.data, dirs.ctypes.data,
                                             hit.ctypes.data, t.ctypes.data, p.ctypes.data,
                                             nr.ctypes.data, m.ctypes.data))
        return hit, t, p, nr, m

    def IntersectProbe(self, org, dirs, hint=None, instance=0):
        """Intersects through a chosen instance of the scene walk (gi_intersect_probe): 0 the
        render's for the loaded scene, 1 every shape kind, 2 triangles and spheres, 3 those plus
        meshes and boxes. hint: per ray, the triangle it leaves from (-1 none). Returns (hit, t,
        point, normal, material, tri)."""
        org = np.ascontiguousarray(org, dtype=np.float64).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        n = len(org)
        assert len(dirs) == n
        if hint is not None:
            hint = np.ascontiguousarray(hint, dtype=np.int32).ravel()
            assert len(hint) == n
        hit = np.zeros(n, dtype=np.int32)
        t = np.zeros(n, dtype=np.float64)
        p = np.zeros((n, 3), dtype=np.float64)
        nr = np.zeros((n, 3), dtype=np.float64)
        m = np.zeros(n, dtype=np.int32)
        tri = np.zeros(n, dtype=np.int32)
        self._check(lib().gi_intersect_probe(
            self._ctx, n, org.ctypes.data, dirs.ctypes.data,
            None if hint is None else hint.ctypes.data, instance, hit.ctypes.data, t.ctypes.data,
            p.ctypes.data, nr.ctypes.data, m.ctypes.data, tri.ctypes.data))
        return hit, t, p, nr, m, tri

    def IllumProbe(self, p_scene, light, r12=None, p_light=None, mask=False, instance=0):
        """RayIlluminationTest as the soft-light loops run it (gi_illum_probe). light: one index
        or one per ray; an area or rect light takes the sample coefficients r12 [n, 2], -1 takes
        the points p_light [n, 3]. mask: apply the fan's occluder mask. Returns (lit [n] int32,
        the points on the light [n, 3])."""
        ps = np.ascontiguousarray(p_scene, dtype=np.float64).reshape(-1, 3)
        n = len(ps)
        li = np.ascontiguousarray(np.broadcast_to(np.asarray(light, dtype=np.int32), (n,)))
        if r12 is not None:
            r12 = np.ascontiguousarray(r12, dtype=np.float64).reshape(-1, 2)
            assert len(r12) == n
        if p_light is not None:
            p_light = np.ascontiguousarray(p_light, dtype=np.float64).reshape(-1, 3)
            assert len(p_light) == n
        out = np.zeros((n, 3), dtype=np.float64)
        lit = np.zeros(n, dtype=np.int32)
        self._check(lib().gi_illum_probe(
            self._ctx, n, ps.ctypes.data, li.ctypes.data,
            None if r12 is None else r12.ctypes.data,
            None if p_light is None else p_light.ctypes.data, int(bool(mask)), instance,
            out.ctypes.data, lit.ctypes.data))
        return lit, out

    def triangle_planes(self):
        """World-space planes [ntris, 4] (unit normal, offset) of the loaded scene's triangles,
        indexed as IntersectProbe's tri (gi_scene_triangle_planes)."""
        cnt = C.c_int64(0)
        self._check(lib().gi_scene_triangle_planes(self._ctx, 0, None, C.byref(cnt)))
        out = np.zeros((cnt.value, 4), dtype=np.float64)
        self._check(lib().gi_scene_triangle_planes(self._ctx, cnt.value, out.ctypes.data,
                                                   C.byref(cnt)))
        return out


MATH_FNS = {"acos": 0, "sin": 1, "cos": 2, "pow": 3, "atan2": 4, "sqrt": 5, "tan": 6, "asin": 7}


def math_probe(renderer, fn, x, y=None):
    """The device's fp64 acos / sin / cos / pow / atan2 / sqrt of host inputs (gi_math_probe)."""
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    y = np.ascontiguousarray(np.zeros_like(x) if y is None else y, dtype=np.float64).ravel()
    out = np.zeros_like(x)
    renderer._check(lib().gi_math_probe(renderer._ctx, MATH_FNS[fn], len(x), x.ctypes.data,
                                        y.ctypes.data, out.ctypes.data))
    return out


def slab_boxes(scene_path):
    """The boxes of a scene file's slab tests as the loader builds them (gi_scene_slab_boxes; no
    device needed): [n, 20] rows of kind, simple, lo[3], hi[3], inverse transform rows [12]."""
    cnt = C.c_int64(0)
    rc = lib().gi_scene_slab_boxes(scene_path.encode(), 0, None, C.byref(cnt))
    if rc != GI_OK:
        raise GiError(f"gi_scene_slab_boxes({scene_path}) rc={rc}")
    out = np.zeros((cnt.value, 20), dtype=np.float64)
    rc = lib().gi_scene_slab_boxes(scene_path.encode(), cnt.value, out.ctypes.data, C.byref(cnt))
    if rc != GI_OK:
        raise GiError(f"gi_scene_slab_boxes({scene_path}) rc={rc}")
    return out


def write_image(path, rgb):
    """rgb: uint8 [H, W, 3] with row 0 = image row y=0 (bottom), like R2Image."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w, _ = rgb.shape
    rc = lib().gi_write_image(path.encode(), w, h, rgb.ctypes.data)
    if rc != GI_OK:
        raise GiError(f"gi_write_image({path}) rc={rc}")


def write_image_float(path, rgbf):
    """rgbf: float32 [H, W, 3] with row 0 = bottom, written as .pfm or .hdr
    (gi_write_image_float)."""
    rgbf = np.ascontiguousarray(rgbf, dtype=np.float32)
    h, w, _ = rgbf.shape
    rc = lib().gi_write_image_float(path.encode(), w, h, rgbf.ctypes.data)
    if rc != GI_OK:
        raise GiError(f"gi_write_image_float({path}) rc={rc}")
