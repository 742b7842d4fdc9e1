"""The fixtures of tests/test_gpu_path_classes.py and tests/test_cpu_path_classes.py: four small
rooms whose element sets and lights select the path kernels' instances that cornell.scn and
jensen.scn (triangles and spheres) never run, the oracle's renders of them (computed once per
test session) and the oracle's Monte Carlo path statistics of them.

All four are ind_hoist_cases' room without its glass sphere, with a sixth material, a mirror,
and a glass and a mirror solid that the camera sees:

- poly:      two boxes (triangles and boxes: the KINDS_POLY instances), point light;
- all:       two cylinders (the KINDS_ALL instances), point light;
- poly_soft, all_soft: the same with an area light and a 4 x 4 shadow fan (HARD = false).

Path statistics are derived from the oracle's counters as mc_wave_cases.path_stats does
(its module docstring says how), with -md 1 .. 3.
"""
import functools
import os

import ind_hoist_cases
import oracle_lib
from camera_cases import tmp_dir

W, H, AA = ind_hoist_cases.W, ind_hoist_cases.H, 1
MIRROR = "material 0 0 0  0.1 0.1 0.1  0.8 0.8 0.8  0 0 0  0 0 0  200 1.0 0"
SOLIDS = {
    "poly": ["box 4  0.12 0.0 0.15  0.40 0.32 0.42", "box 5  0.6 0.0 0.1  0.85 0.25 0.35"],
    "all": ["cylinder 4  0.26 0.16 0.28  0.13 0.32", "cylinder 5  0.72 0.13 0.22  0.12 0.26"],
}
AREA_LIGHT = "area_light 0.25 0.25 0.25  0.5 0.95 0.5  0 -1 0  0.15  0 0 1"
SCENES = ("all", "all_soft", "poly", "poly_soft")
FLAGS = ["-resolution", str(W), str(H), "-aa", str(AA), "-it", "8", "-tt", "4", "-st", "4",
         "-global", "5000", "-caustic", "5000", "-seed", "7"]
SOFT_FLAGS = ["-lt", "4", "-ss", "4"]
MDS = (1, 2, 3)


def scene_text(name):
    solids = SOLIDS[name.split("_")[0]]
    soft = name.endswith("_soft")
    out, nmat = [], 0
    for ln in ind_hoist_cases.SCENE_TEXT.splitlines():
        if ln.startswith("sphere"):
            continue
        if ln.startswith("point_light"):
            out += solids + [""]
            if soft:
                ln = AREA_LIGHT
        out.append(ln)
        if ln.startswith("material"):
            nmat += 1
            if nmat == 5:
                out.append(MIRROR)
    text = "\n".join(out) + "\n"
    assert text.count("material") == 6 and text.count("\nsphere") == 0
    assert text.count("_light") == 1 and all(s in text for s in solids)
    return text


@functools.lru_cache(maxsize=None)
def scene_path(name):
    dst = os.path.join(tmp_dir(), f"path_class_{name}.scn")
    with open(dst, "w") as f:
        f.write(scene_text(name))
    return dst


def args(name, extra=()):
    soft = SOFT_FLAGS if name.endswith("_soft") else []
    return [scene_path(name), "/tmp/x.png"] + FLAGS + soft + list(extra)


@functools.lru_cache(maxsize=None)
def oracle_frame(name):
    """(rgb8, rgbf, stats) of the oracle on the frame. Shared by the tests: do not modify."""
    rgb, st = oracle_lib.render(args(name), W, H)
    f, rgb2 = oracle_lib.render_float(args(name), W, H)
    assert (rgb == rgb2).all()
    for a in (rgb, f):
        a.setflags(write=False)
    return rgb, f, st


@functools.lru_cache(maxsize=None)
def path_stats(name):
    """The oracle's Monte Carlo path statistics of the frame: the number of paths and
    monte[k] = monte_carlo_rays under -md k (mc_wave_cases' module docstring)."""
    def run(extra):
        return oracle_lib.render(args(name, ["-no_indirect", "-no_caustic"] + extra), W, H)[1]
    none = run(["-no_monte"])
    assert none["monte_carlo_rays"] == 0
    paths = int(none["transmissive_samples"] + none["specular_samples"])
    return {"paths": paths, "monte": {k: int(run(["-md", str(k)])["monte_carlo_rays"]) for k in MDS}}
