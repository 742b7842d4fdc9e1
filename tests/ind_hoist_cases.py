"""The fixture of tests/test_gpu_ind_hoist.py and tests/test_cpu_ind_hoist.py: a scene written by
the test with the surfaces that the indirect paths' per-primary and per-material values
(gi_kernels.h Spawn::ind_key / perp, gi_layout.h DMaterial::kd_pd) can get wrong, and the oracle's
renders of it (computed once per test session).

The room is the unit cube, open towards the camera (which looks along +z):

- floor, ceiling and side walls have 1 - |n.z| = 1: Diffuse_ImportanceSample's first tangent
  (n.y, -n.x, 0); the back wall and the free-standing quad have |n.z| = 1: its second tangent
  (n.z, 0, -n.x);
- a slanted triangle, n about (0, -0.68, 0.73): first tangent, all three terms of the normalisation;
- the quad (z = 0.6) and the slanted triangle are wound with their normals away from the camera,
  so the primary hit has cos(theta) < 0 and the sampler flips the normal;
- material 0 (floor, back wall): kd 0.7 0.3 0.5, whose quotients by 0.7 are inexact;
- material 1 (left wall, slanted triangle): kd 0.95 0.6 0.35 and emission 0.08, so that
  max kd + max e + prob_absorb = 1.035 > 1 (montecarlo.cpp's `rnd *= ptot` branch);
- a small glass sphere behind the quad, which no camera ray reaches: it gives the caustic map its
  photons and queues the indirect samples that hit it (ind_cont_kernel), while every global-map
  query of the frame still belongs to an indirect sample (no primary hit spawns Monte Carlo paths);
- a dim point light behind the quad's plane.
"""
import functools
import os

import numpy as np

import oracle_lib
import ray_cases
from camera_cases import tmp_dir

W, H, AA = 16, 12, 1
SCENE_TEXT = """camera 0.5 0.5 -1.6   0 0 1   0 1 0   0.329   0.01 100

material 0 0 0   0.7 0.3 0.5     0 0 0   0 0 0   0 0 0         10 1.0 0
material 0 0 0   0.95 0.6 0.35   0 0 0   0 0 0   0.08 0.08 0.08   10 1.0 0
material 0 0 0   0.2 0.6 0.8     0 0 0   0 0 0   0 0 0         10 1.0 0
material 0 0 0   0.5 0.7 0.3     0 0 0   0 0 0   0 0 0         10 1.0 0
material 0 0 0   0 0 0           0 0 0   1 1 1   0 0 0         5000 1.372 0

# floor
tri 0   1 0 0   0 0 0   0 0 1
tri 0   0 0 1   1 0 1   1 0 0
# back wall
tri 0   1 0 1   0 0 1   0 1 1
tri 0   0 1 1   1 1 1   1 0 1
# right wall (x = 0)
tri 2   0 0 1   0 0 0   0 1 0
tri 2   0 1 0   0 1 1   0 0 1
# left wall (x = 1)
tri 1   1 0 0   1 0 1   1 1 1
tri 1   1 1 1   1 1 0   1 0 0
# ceiling
tri 2   1 1 0   1 1 1   0 1 1
tri 2   0 1 1   0 1 0   1 1 0
# slanted triangle, normal away from the camera
tri 1   0.05 0.02 0.5   0.5 0.02 0.5   0.25 0.5 0.95
# free-standing quad at z = 0.6, normal +z (away from the camera)
tri 3   0.5 0.1 0.6   0.95 0.1 0.6   0.95 0.7 0.6
tri 3   0.95 0.7 0.6   0.5 0.7 0.6   0.5 0.1 0.6
# glass sphere hidden behind the quad
sphere 4   0.74 0.38 0.82   0.09

point_light 0.25 0.25 0.25   0.5 0.85 0.75   0 0 1
"""
FLAGS = ["-resolution", str(W), str(H), "-aa", str(AA), "-it", "8", "-global", "5000",
         "-caustic", "5000", "-seed", "7"]
DOF = ["-dof", "2", "2.2", "0.03"]
GLASS = 4  # the sphere's material index
# the ray batch of the scene (ray_cases.SCENES entry): extent, panorama origin / elevation / span
RAY_SCENE = "ind_hoist"
RAY_SENSOR, RAY_SPP = "panorama", 3  # from inside the room: every surface, both sides of the quad


@functools.lru_cache(maxsize=None)
def scene_path():
    dst = os.path.join(tmp_dir(), "ind_hoist.scn")
    with open(dst, "w") as f:
        f.write(SCENE_TEXT)
    return dst


def args(dof=False):
    return [scene_path(), "/tmp/x.png"] + FLAGS + (DOF if dof else [])


@functools.lru_cache(maxsize=None)
def oracle_frame(dof=False):
    """(rgb8, rgbf, stats) of the oracle on the frame. Shared by the tests: do not modify."""
    rgb, st = oracle_lib.render(args(dof), W, H)
    f, rgb2 = oracle_lib.render_float(args(dof), W, H)
    assert (rgb == rgb2).all()
    for a in (rgb, f):
        a.setflags(write=False)
    return rgb, f, st


@functools.lru_cache(maxsize=None)
def primary_classes(dof=False):
    """Shares among the oracle's primary hits (camera rays, intersections): back-facing, first
    tangent, second tangent; and the number of primary hits on the glass sphere."""
    rays, _ids = oracle_lib.camera_rays(args(dof))
    hit, _t, _p, n, m = oracle_lib.intersect(scene_path(), rays["org"], rays["dir"])
    hit = hit != 0
    ct = -(n * rays["dir"]).sum(1)
    second = 1.0 - np.abs(n[:, 2]) < 0.1
    return (float((ct[hit] < 0).mean()), float((~second[hit]).mean()), float(second[hit].mean()),
            int((m[hit] == GLASS).sum()))


def register_ray_scene():
    """The scene as a ray_cases scene, so that ray_cases.batch / oracle_batch serve it (an
    absolute file name stands for itself in ray_cases.scene_path)."""
    ray_cases.SCENES.setdefault(RAY_SCENE, (scene_path(), FLAGS, 1.0, (0.5, 0.5, 0.3),
                                            (-0.5, 0.5), 0.75))
