"""Fixtures shared by tests/test_cpu_denoise.py, tests/test_gpu_aov.py and
tests/test_gpu_denoise.py: frames and ray batches whose feature planes are derived from the
oracle alone (computed once per test session).

For every sample ray of a case -- oracle_lib.camera_rays(args) for a camera frame, ray_cases'
batches for a caller-made one -- oracle_lib.intersect gives hit, point, normal and material
index, and the distance is oracle_lib.math("sqrt", ...) of dx*dx + dy*dy + dz*dz. The pixel
reduction is denoise_ref.reduce_planes. The albedo plane needs each material's kd: the caller
passes the table (gi_get_materials on the device, whose material index is the oracle's:
test_gpu_render.py compares them).
"""
import functools

import numpy as np

import denoise_ref
import oracle_lib
import ray_cases
from gpu_util import scene

# name -> (scene file, width, height, aa, dof_test, further flags)
CAMERA_CASES = {
    "stilllife": ("stilllife.scn", 24, 16, 1, 1, []),
    "cornell": ("cornell.scn", 24, 16, 1, 1, []),
    "teapot_dof": ("teapot.scn", 20, 20, 0, 2, ["-dof", "2", "8.0", "0.05"]),
}
# ray_cases batches (scene, sensor, spp): the cornell panorama has misses (the box is open
# behind the origin)
RAY_BATCHES = [("cornell_dim", "panorama", 3), ("stilllife", "lightfield", 3)]

# the quality case: a noisy and a converged oracle frame of cornell.scn
QUALITY_W, QUALITY_H = 48, 32
QUALITY_FLAGS = ["-resolution", "48", "32", "-aa", "0", "-global", "20000", "-caustic", "20000",
                 "-tt", "4", "-st", "4"]
NOISY_FLAGS = ["-it", "4", "-seed", "2"]
CONVERGED_FLAGS = ["-it", "256", "-seed", "3"]


def camera_args(name):
    scn, w, h, aa, _dof, extra = CAMERA_CASES[name]
    return [scene(scn), "/tmp/x.png", "-resolution", str(w), str(h), "-aa", str(aa)] + extra


def camera_spp(name):
    _scn, _w, _h, aa, dof, _extra = CAMERA_CASES[name]
    return 4 ** aa * dof


def _samples(scene_path, rays):
    hit, _t, p, n, m = oracle_lib.intersect(scene_path, rays["org"], rays["dir"])
    depth = oracle_lib.math("sqrt", denoise_ref.sample_depth(rays["org"], p))
    out = (hit != 0, n, depth, m)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def camera_samples(name):
    """(hit [n] bool, normal [n, 3], depth [n], material [n]) of the oracle on the case's
    camera rays, in gi_camera_rays' order. Shared by the tests: do not modify."""
    rays, _ids = oracle_lib.camera_rays(camera_args(name))
    _scn, w, h, _aa, _dof, _extra = CAMERA_CASES[name]
    assert len(rays) == w * h * camera_spp(name)
    return _samples(camera_args(name)[0], rays)


@functools.lru_cache(maxsize=None)
def batch_samples(name, sensor, spp):
    rays, _ids = ray_cases.batch(name, sensor, spp)
    return _samples(ray_cases.scene_path(name), rays)


def planes(samples, width, height, spp, kd_table):
    """The expected planes from a case's oracle samples and the materials' kd [nmat, 3]."""
    hit, normal, depth, mat = samples
    kd_table = np.asarray(kd_table, dtype=np.float64)
    kd = np.zeros((len(mat), 3))
    kd[hit] = kd_table[mat[hit]]
    return denoise_ref.reduce_planes(width, height, spp, hit, normal, depth, kd)


def camera_planes(name, kd_table):
    _scn, w, h, _aa, _dof, _extra = CAMERA_CASES[name]
    return planes(camera_samples(name), w, h, camera_spp(name), kd_table)


def batch_planes(name, sensor, spp, kd_table):
    return planes(batch_samples(name, sensor, spp), ray_cases.W, ray_cases.H, spp, kd_table)


def coverage_classes(samples, spp):
    """Shares of fully covered, partly covered and empty pixels."""
    hits = samples[0].reshape(-1, spp).sum(1)
    return (float((hits == spp).mean()), float(((hits > 0) & (hits < spp)).mean()),
            float((hits == 0).mean()))


def quality_args(tail):
    return [scene("cornell.scn"), "/tmp/x.png"] + QUALITY_FLAGS + tail


@functools.lru_cache(maxsize=None)
def quality_frames():
    """(noisy, converged) float frames of the oracle on the quality case."""
    noisy = oracle_lib.render_float(quality_args(NOISY_FLAGS), QUALITY_W, QUALITY_H)[0]
    conv = oracle_lib.render_float(quality_args(CONVERGED_FLAGS), QUALITY_W, QUALITY_H)[0]
    noisy.setflags(write=False)
    conv.setflags(write=False)
    return noisy, conv


def rmse(a, b):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return float(np.sqrt((d * d).mean()))
