"""Cases shared by tests/test_gpu_camera.py and tests/test_cli_camera.py: two scenes with a new
camera each, and the oracle's renders of them (computed once per test session).

The reference for a set camera is the oracle rendering a copy of the scene file whose `camera`
line is rewritten: the restatement renders any .scn. Both cameras are used at 24 x 16 (not
square) and have an `up` that is not orthogonal to `towards`, so a width / height swap or a
skipped triad construction shows.
"""
import functools
import os
import tempfile

import oracle_lib
from gpu_util import scene

CORNELL_FLAGS = ["-resolution", "24", "16", "-aa", "1", "-global", "20000", "-caustic", "20000",
                 "-it", "16", "-tt", "8", "-st", "8", "-seed", "5"]
JENSEN_FLAGS = ["-resolution", "24", "16", "-aa", "0", "-global", "4000", "-caustic", "20000",
                "-lt", "4", "-ss", "4", "-it", "16", "-tt", "8", "-st", "8", "-seed", "9"]
# name -> (scene, the new `camera` line's twelve numbers, flags)
CASES = {
    "cornell": ("cornell.scn", "0.95 0.80 -1.2  -0.30 -0.20 1  0.1 1 0.05  0.40  0.01 100",
                CORNELL_FLAGS),
    "jensen": ("jensen.scn", "4.2 4.0 -7.0  -0.18 -0.15 1  0.05 1 0  0.36  0.01 100",
               JENSEN_FLAGS),
}
# cornell.scn's own `camera` line: eye, towards, up, xfov
CORNELL_FILE_CAMERA = ((0.556, 0.546, -1.6), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 0.329)

_tmp = None


def camera_of(line):
    """(eye, towards, up, xfov) of a `camera` line's numbers."""
    v = [float(x) for x in line.split()]
    return tuple(v[0:3]), tuple(v[3:6]), tuple(v[6:9]), v[9]


def rewrite_scene(src, camera_line, dst_dir):
    """Copy of scene file `src` in dst_dir with every `camera` line dropped and the new one
    first (the scenes used here reference no mesh files)."""
    with open(src) as f:
        lines = [ln for ln in f.read().splitlines() if not ln.lstrip().startswith("camera")]
    dst = os.path.join(str(dst_dir), "view_" + os.path.basename(src))
    with open(dst, "w") as f:
        f.write("camera " + camera_line + "\n" + "\n".join(lines) + "\n")
    return dst


@functools.lru_cache(maxsize=None)
def oracle_view(name):
    """(8-bit image, stats) of the oracle on case `name`'s rewritten scene."""
    global _tmp
    if _tmp is None:
        _tmp = tempfile.TemporaryDirectory(prefix="gi_views_")
    scn, cam, flags = CASES[name]
    path = rewrite_scene(scene(scn), cam, _tmp.name)
    return oracle_lib.render([path, "/tmp/x.png"] + flags, 24, 16)


@functools.lru_cache(maxsize=None)
def oracle_file_view():
    """The oracle on cornell.scn as it is (the file's camera), CORNELL_FLAGS."""
    return oracle_lib.render([scene("cornell.scn"), "/tmp/x.png"] + CORNELL_FLAGS, 24, 16)
