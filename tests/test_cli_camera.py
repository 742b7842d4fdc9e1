"""The drop-in CLI's extension flag `-camera ex ey ez tx ty tz ux uy uz xfov` (gi_set_camera
after ReadScene). The CLI takes the flag out of argv itself, before gi_parse_args, which keeps
the reference's flag set: fewer than ten numbers or a non-number is an argument error (the
reference's "Invalid program argument" line, exit 1) raised before any device is opened or the
scene file is looked at.
"""
import os
import subprocess

import numpy as np
import pytest

import gi_amd
import pngio
from camera_cases import CASES, oracle_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "global-illumination_amd", "photonmap")
SCENES = os.path.join(ROOT, "tests", "scenes")


def run(args, timeout=300):
    assert os.path.exists(CLI), f"{CLI} not built (run __graft_entry__.build())"
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("tail", [
    ["-camera", "1", "2", "3"],                                              # too few
    ["-camera"],
    ["-camera", "1", "2", "3", "4", "5", "6", "7", "8", "9"],                # nine
    ["-camera", "1", "2", "3", "4", "5", "6", "7", "8", "x", "0.3"],         # a non-number
    ["-camera", "1", "2", "3", "4", "5", "6", "7", "8", "9", "0.3f"],        # trailing junk
    ["-v", "-camera", "1", "2", "3", "-no_shadow", "4", "5", "6", "7", "8", "9"],
], ids=["three", "none", "nine", "non_number", "junk", "flag_inside"])
def test_bad_camera_flag_is_an_argument_error(tail, tmp_path):
    out = tmp_path / "o.png"
    # the scene does not exist: reaching ReadScene would print its message and exit -1
    r = run([str(tmp_path / "missing.scn"), str(out)] + tail)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert r.stderr == "Invalid program argument: -camera"
    assert r.stdout == ""
    assert not out.exists()


def test_camera_flag_is_removed_before_parse_args(tmp_path):
    """A complete -camera passes the argument stage wherever it stands among the flags: the next
    failure is the missing scene file (or, on a machine without a GPU, the device)."""
    cam = CASES["cornell"][1].split()[:10]
    r = run([str(tmp_path / "missing.scn"), str(tmp_path / "o.png"), "-aa", "0", "-camera"] + cam
            + ["-no_shadow"])
    assert r.returncode == 255, (r.returncode, r.stderr)
    assert "Invalid program argument" not in r.stderr
    # ... and what follows it is still parsed
    r = run([str(tmp_path / "missing.scn"), str(tmp_path / "o.png"), "-camera"] + cam + ["-bogus"])
    assert r.returncode == 1
    assert r.stderr == "Invalid program argument: -bogus"


def test_parse_args_still_rejects_camera():
    cam = CASES["cornell"][1].split()[:10]
    with pytest.raises(ValueError, match=r"^Invalid program argument: -camera$"):
        gi_amd.ParseArgs(["a.scn", "b.png", "-camera"] + cam)


@pytest.mark.gpu
def test_cli_camera_matches_oracle_on_rewritten_scene(tmp_path):
    scn, cam, flags = CASES["cornell"]
    png = str(tmp_path / "view.png")
    r = run([os.path.join(SCENES, scn), png] + flags + ["-camera"] + cam.split()[:10])
    assert r.returncode == 0, r.stderr
    np.testing.assert_array_equal(pngio.read_png(png)[::-1], oracle_view("cornell")[0])
