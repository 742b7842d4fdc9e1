"""Cases shared by tests/test_gpu_camera.py and tests/test_cli_camera.py: scenes with a new
camera each, and the oracle's renders of them, 8-bit and float (computed once per test session).

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
    # the cornell case on dimmed_cornell(): 59 % of the cornell view's channel values are 255 and
    # 13 % are 0 (a unit point light with 1 / d^2 falloff inside a 1.1-wide box), and an error in
    # a clamped value cannot show
    "cornell_dim": ("dimmed", "0.95 0.80 -1.2  -0.30 -0.20 1  0.1 1 0.05  0.40  0.01 100",
                    CORNELL_FLAGS),
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


def tmp_dir():
    global _tmp
    if _tmp is None:
        _tmp = tempfile.TemporaryDirectory(prefix="gi_views_")
    return _tmp.name


@functools.lru_cache(maxsize=None)
def dimmed_cornell():
    """Copy of cornell.scn (written once per test session) whose point light is 0.2 0.2 0.2
    instead of 1 1 1, so that most values of a view lie strictly inside (0, 1)."""
    with open(scene("cornell.scn")) as f:
        text = f.read()
    assert text.count("point_light 1 1 1") == 1
    dst = os.path.join(tmp_dir(), "dim_cornell.scn")
    with open(dst, "w") as f:
        f.write(text.replace("point_light 1 1 1", "point_light 0.2 0.2 0.2"))
    return dst


def case_scene(name):
    """The scene file case `name` starts from (its own camera line still in it)."""
    scn = CASES[name][0]
    return dimmed_cornell() if scn == "dimmed" else scene(scn)


def _view_args(name):
    _scn, cam, flags = CASES[name]
    return [rewrite_scene(case_scene(name), cam, tmp_dir()), "/tmp/x.png"] + flags


@functools.lru_cache(maxsize=None)
def oracle_view(name):
    """(8-bit image, stats) of the oracle on case `name`'s rewritten scene."""
    return oracle_lib.render(_view_args(name), 24, 16)


@functools.lru_cache(maxsize=None)
def oracle_view_float(name):
    """The oracle's float image of case `name`'s rewritten scene."""
    f, rgb = oracle_lib.render_float(_view_args(name), 24, 16)
    assert (rgb == oracle_view(name)[0]).all()
    return f


@functools.lru_cache(maxsize=None)
def oracle_file_view():
    """The oracle on cornell.scn as it is (the file's camera), CORNELL_FLAGS."""
    return oracle_lib.render([scene("cornell.scn"), "/tmp/x.png"] + CORNELL_FLAGS, 24, 16)


@functools.lru_cache(maxsize=None)
def oracle_file_view_float():
    """The oracle's float image of cornell.scn as it is, CORNELL_FLAGS."""
    f, rgb = oracle_lib.render_float([scene("cornell.scn"), "/tmp/x.png"] + CORNELL_FLAGS, 24, 16)
    assert (rgb == oracle_file_view()[0]).all()
    return f
