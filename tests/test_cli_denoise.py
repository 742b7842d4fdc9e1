"""The drop-in CLI's extension flag `-denoise L` (gi_camera_features + gi_denoise after the
render, L = 1..8 levels, other parameters default). Like -camera, the CLI takes the flag out of
argv itself, before gi_parse_args, which keeps the reference's flag set: a missing, non-integer
or out-of-range L is an argument error (the reference's "Invalid program argument" line, exit 1)
raised before any device is opened or the scene file is looked at.
"""
import os
import subprocess

import pytest

import gi_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "global-illumination_amd", "photonmap")


def run(args, timeout=300):
    assert os.path.exists(CLI), f"{CLI} not built (run __graft_entry__.build())"
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("tail", [
    ["-denoise"],                               # missing
    ["-aa", "0", "-denoise"],
    ["-denoise", "x"],                          # not a number
    ["-denoise", "2.5"],                        # not an integer
    ["-denoise", "3x"],                         # trailing junk
    ["-denoise", "0"],                          # out of range
    ["-denoise", "9"],
    ["-denoise", "-1"],
    ["-denoise", "-no_shadow"],                 # a flag where L belongs
    ["-denoise", "5", "-v", "-denoise", "12"],  # the last one counts too
], ids=["none", "none_at_end", "non_number", "float", "junk", "zero", "nine", "negative",
        "flag", "second_bad"])
def test_bad_denoise_flag_is_an_argument_error(tail, tmp_path):
    out = tmp_path / "o.png"
    # the scene does not exist: reaching ReadScene would print its message and exit -1
    r = run([str(tmp_path / "missing.scn"), str(out)] + tail)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert r.stderr == "Invalid program argument: -denoise"
    assert r.stdout == ""
    assert not out.exists()


@pytest.mark.parametrize("levels", ["1", "5", "8"])
def test_denoise_flag_is_removed_before_parse_args(levels, tmp_path):
    """A complete -denoise passes the argument stage wherever it stands among the flags: the
    next failure is the missing scene file (or, on a machine without a GPU, the device)."""
    r = run([str(tmp_path / "missing.scn"), str(tmp_path / "o.png"), "-aa", "0", "-denoise",
             levels, "-no_shadow"])
    assert r.returncode == 255, (r.returncode, r.stderr)
    assert "Invalid program argument" not in r.stderr
    # ... and what follows it is still parsed
    r = run([str(tmp_path / "missing.scn"), str(tmp_path / "o.png"), "-denoise", levels,
             "-bogus"])
    assert r.returncode == 1
    assert r.stderr == "Invalid program argument: -bogus"


def test_denoise_and_camera_flags_together(tmp_path):
    cam = "0.95 0.80 -1.2 -0.30 -0.20 1 0.1 1 0.05 0.40".split()
    r = run([str(tmp_path / "missing.scn"), str(tmp_path / "o.png"), "-denoise", "3", "-camera"]
            + cam + ["-bogus"])
    assert r.returncode == 1
    assert r.stderr == "Invalid program argument: -bogus"
    # a -denoise among the camera's numbers breaks the camera, which is looked at first
    r = run([str(tmp_path / "missing.scn"), str(tmp_path / "o.png"), "-camera"] + cam[:4]
            + ["-denoise", "3"] + cam[4:])
    assert r.returncode == 1
    assert r.stderr == "Invalid program argument: -camera"


def test_parse_args_still_rejects_denoise():
    with pytest.raises(ValueError, match=r"^Invalid program argument: -denoise$"):
        gi_amd.ParseArgs(["a.scn", "b.png", "-denoise", "5"])
