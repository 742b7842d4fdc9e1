"""Ray batches shared by tests/test_cpu_rays.py and tests/test_gpu_rays.py: three sensors that
are not the pinhole camera (gi.h: gi_render_rays serves "any sensor"), built in numpy from a
scene's file camera, and the oracle's renders of them (oracle_lib.render_rays, computed once per
test session).

The frame of a scene's `camera` line is t = norm(towards), r = norm(t x up), u = r x t. Every
batch is 24 x 16 pixels (37 x 21 for the batching test) with spp rays per pixel at sub-positions
of a 5 x 5 jitter grid; a = x - 1/2 and b = (y - 1/2) * H / W are a ray's film coordinates.

- orthographic: origin eye + a E r + b E u, direction t: every ray has its own origin, so a hit
  shaded from one common view point shows;
- light-field slice: origin on a square lens of side E / 2 around the eye (seeded rng), aimed at
  eye + 8 t + a E r + b E u;
- panorama: one origin inside the scene, equirectangular directions (azimuth centred on t).

A batch only counts as a fixture if the oracle's own result can show an error: at least 60 % of
its rays hit and at least 60 % of its float channel values lie strictly inside (0, 1)
(test_cpu_rays.py asserts both for every batch below).
"""
import functools

import numpy as np

import oracle_lib
from camera_cases import CORNELL_FLAGS, JENSEN_FLAGS, dimmed_cornell
from gpu_util import scene

W, H = 24, 16
STILLLIFE_FLAGS = ["-resolution", "24", "16", "-aa", "0", "-global", "20000", "-caustic", "40000",
                   "-it", "8", "-tt", "4", "-st", "4", "-seed", "2"]
# sub-positions of a pixel's rays: cells of a 5 x 5 grid, no two in one row or column
JITTER = ((2, 2), (0, 3), (4, 1), (1, 0), (3, 4))
LENS_SEED = 17

# scene -> (file or "dimmed", flags, extent E, panorama origin, panorama elevation range / pi,
#           panorama azimuth span / 2 pi, centred on `towards`). The cornell panorama spans 270
# degrees: the box is open behind the origin, and with the full circle 21 % of the rays leave
# through it, which left the share of values inside (0, 1) at 0.60-0.66, next to the 0.6 bound.
SCENES = {
    "stilllife": ("stilllife.scn", STILLLIFE_FLAGS, 2.0, (0.0, 1.0, 0.0), (-0.5, 0.1), 1.0),
    "jensen": ("jensen.scn", JENSEN_FLAGS, 4.0, (2.78, 2.5, 2.0), (-0.5, 0.5), 1.0),
    "cornell_dim": ("dimmed", CORNELL_FLAGS, 1.0, (0.556, 0.546, 0.3), (-0.5, 0.5), 0.75),
}
SENSORS = ("ortho", "lightfield", "panorama")
# (scene, sensor, spp): every sensor on every scene at spp 3, spp 1 and 5 on one sensor per scene
BATCHES = [(s, k, 3) for s in SCENES for k in SENSORS] + [
    ("stilllife", "lightfield", 1), ("stilllife", "lightfield", 5),
    ("jensen", "ortho", 1), ("jensen", "ortho", 5),
    ("cornell_dim", "panorama", 1), ("cornell_dim", "panorama", 5),
]
# the batches that also run with ids = None (the default id of ray r is r): one per scene
DEFAULT_ID_BATCHES = [("stilllife", "lightfield", 3), ("jensen", "ortho", 5),
                      ("cornell_dim", "panorama", 3)]

# the batching test's batch (test_gpu_rays.py): a frame of odd size, about 33,000 path slots, that
# one batch holds at GI_SLOT_LIMIT = 60000 and that is split at 9000
TILED_BATCH = ("stilllife", "lightfield", 3, 37, 21)


def scene_path(name):
    src = SCENES[name][0]
    return dimmed_cornell() if src == "dimmed" else scene(src)


def scene_args(name, width=W, height=H):
    """The command line of scene `name` at width x height."""
    flags = list(SCENES[name][1])
    i = flags.index("-resolution")
    flags[i + 1], flags[i + 2] = str(width), str(height)
    return [scene_path(name), "/tmp/x.png"] + flags


def file_camera(path):
    """(eye, towards, up) of the scene file's `camera` line, as float64 arrays."""
    with open(path) as f:
        for ln in f:
            if ln.lstrip().startswith("camera"):
                v = np.array([float(x) for x in ln.split()[1:10]])
                return v[0:3], v[3:6], v[6:9]
    raise ValueError(path + ": no camera line")


def frame(towards, up):
    t = towards / np.linalg.norm(towards)
    r = np.cross(t, up)
    r /= np.linalg.norm(r)
    return t, r, np.cross(r, t)


def film(spp, width, height):
    """Film coordinates (a, b) of the width * height * spp rays, pixel-major (row 0 = bottom):
    a in (-1/2, 1/2) across the width, b scaled by height / width (square pixels)."""
    y, x, s = np.meshgrid(np.arange(height), np.arange(width), np.arange(spp), indexing="ij")
    jit = np.array(JITTER, dtype=np.float64)
    fx = (x + (jit[s, 0] + 0.5) / 5.0) / width
    fy = (y + (jit[s, 1] + 0.5) / 5.0) / height
    return (fx - 0.5).ravel(), ((fy - 0.5) * height / width).ravel()


def make_rays(name, sensor, spp, width=W, height=H):
    """The batch's rays [width * height * spp] (oracle_lib.RAY_DTYPE), unit directions."""
    _src, _flags, E, pano_org, pano_el, pano_az = SCENES[name]
    eye, towards, up = file_camera(scene_path(name))
    t, r, u = frame(towards, up)
    a, b = film(spp, width, height)
    n = len(a)
    if sensor == "ortho":
        org = eye + np.outer(a * E, r) + np.outer(b * E, u)
        d = np.broadcast_to(t, (n, 3))
    elif sensor == "lightfield":
        lens = np.random.default_rng(LENS_SEED).random((n, 2)) - 0.5
        org = eye + np.outer(lens[:, 0] * (E / 2), r) + np.outer(lens[:, 1] * (E / 2), u)
        d = eye + 8.0 * t + np.outer(a * E, r) + np.outer(b * E, u) - org
    elif sensor == "panorama":
        org = np.broadcast_to(np.array(pano_org), (n, 3))
        theta = 2.0 * np.pi * pano_az * a
        lo, hi = pano_el
        phi = np.pi * (lo + (hi - lo) * (b * width / height + 0.5))
        d = (np.outer(np.cos(phi) * np.sin(theta), r) + np.outer(np.cos(phi) * np.cos(theta), t)
             + np.outer(np.sin(phi), u))
    else:
        raise ValueError(sensor)
    rays = np.zeros(n, dtype=oracle_lib.RAY_DTYPE)
    rays["org"] = org
    rays["dir"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    return rays


def explicit_ids(n):
    """Stream ids that exceed 32 bits: r * 2654435761 + 2^40."""
    return np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(1 << 40)


@functools.lru_cache(maxsize=None)
def batch(name, sensor, spp, width=W, height=H):
    rays = make_rays(name, sensor, spp, width, height)
    rays.setflags(write=False)
    ids = explicit_ids(len(rays))
    ids.setflags(write=False)
    return rays, ids


@functools.lru_cache(maxsize=None)
def oracle_batch(name, sensor, spp, explicit=True, width=W, height=H):
    """(rgb8, rgbf, the nine counters) of the oracle on the batch, with the explicit ids or with
    ids = None. Shared by the tests: do not modify."""
    rays, ids = batch(name, sensor, spp, width, height)
    rgb, f, st = oracle_lib.render_rays(scene_args(name, width, height), spp, rays,
                                        ids if explicit else None)
    rgb.setflags(write=False)
    f.setflags(write=False)
    return rgb, f, st


def hit_fraction(name, rays):
    hit = oracle_lib.intersect(scene_path(name), rays["org"], rays["dir"])[0]
    return float((hit != 0).mean())


def inside_fraction(f):
    """Share of float channel values strictly inside (0, 1)."""
    return float(((f > 0.0) & (f < 1.0)).mean())
