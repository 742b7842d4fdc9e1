"""The fixtures of tests/test_gpu_mc_wave.py and tests/test_cpu_mc_wave.py: the two frames of
test_gpu_render.py's test_indirect_continuation_queue_is_exact (32 x 32, hard lights in cornell,
soft lights in jensen), the oracle's renders of them (computed once per test session), the
oracle's path statistics of them, and a room without glass or mirror.

Path statistics. The oracle has no per-path bounce counts, so they are derived from its counters.
A Monte Carlo path (MonteCarlo_PathTrace, montecarlo.cpp:16-171) ends at a diffuse event whether
or not -no_indirect is given, and draws the same random numbers up to there, so the paths of a
frame have the same lengths with and without their indirect sub-paths; with -no_indirect (and
-no_caustic) the counters hold the Monte Carlo paths' bounces alone, and no photon map is
built. From runs with -no_monte and with -md 1 .. 4 and the default -md 128:

- paths:         transmissive_samples and specular_samples under -no_monte (each path counts one
                 sample at the primary hit and, the loop returning at once, nothing else);
- monte[k]:      monte_carlo_rays under -md k, the bounces 1 .. k that hit something; monte[k + 1]
                 - monte[k] paths run a bounce k + 1;
- continued[1]:  (transmissive_samples + specular_samples under -md 1) - paths, the paths whose
                 first bounce sampled a further ray; the others ended at their first bounce.
"""
import functools
import os

import ind_hoist_cases
import oracle_lib
from camera_cases import tmp_dir
from gpu_util import scene

W = H = 32
FLAGS = ["-resolution", str(W), str(H), "-aa", "1", "-it", "32", "-tt", "8", "-st", "8",
         "-seed", "4"]
SCENES = {
    "cornell": ("cornell.scn", ["-global", "20000", "-caustic", "20000"]),
    "jensen": ("jensen.scn", ["-global", "4000", "-caustic", "20000", "-lt", "4", "-ss", "4"]),
}
MD_DEFAULT = 128
COUNTERS = ("screen_rays", "shadow_rays", "monte_carlo_rays", "transmissive_samples",
            "specular_samples", "indirect_samples", "caustic_samples", "knn_queries")


def args(name, extra=()):
    scn, photons = SCENES[name]
    return [scene(scn), "/tmp/x.png"] + FLAGS + photons + list(extra)


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
    """The oracle's Monte Carlo path statistics of the frame (module docstring)."""
    def run(extra):
        return oracle_lib.render(args(name, ["-no_indirect", "-no_caustic"] + extra), W, H)[1]
    none = run(["-no_monte"])
    trans, spec = int(none["transmissive_samples"]), int(none["specular_samples"])
    assert none["monte_carlo_rays"] == 0
    by_md = {k: run(["-md", str(k)]) for k in (1, 2, 3, 4)}
    by_md[MD_DEFAULT] = run([])
    monte = {k: int(st["monte_carlo_rays"]) for k, st in by_md.items()}
    first = by_md[1]
    continued1 = int(first["transmissive_samples"] + first["specular_samples"]) - trans - spec
    return {"transmissive_paths": trans, "specular_paths": spec, "monte": monte,
            "continued1": continued1}


# ind_hoist_cases' room without its glass sphere: no primary hit spawns a Monte Carlo path and
# no indirect sample meets a transmissive or specular surface
PLAIN_TEXT = "\n".join(ln for ln in ind_hoist_cases.SCENE_TEXT.splitlines()
                       if not ln.startswith("sphere")) + "\n"
PLAIN_FLAGS = ["-resolution", "16", "12", "-aa", "1", "-it", "8", "-global", "5000",
               "-no_caustic", "-seed", "7"]


@functools.lru_cache(maxsize=None)
def plain_args():
    assert PLAIN_TEXT.count("sphere") == 1  # the comment line above the removed element
    dst = os.path.join(tmp_dir(), "mc_wave_plain.scn")
    with open(dst, "w") as f:
        f.write(PLAIN_TEXT)
    return [dst, "/tmp/x.png"] + PLAIN_FLAGS
