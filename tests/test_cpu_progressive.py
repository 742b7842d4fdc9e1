"""Host side of the progressive photon-map passes: the radius schedule (gi_progressive_radius)
against tests/progressive_ref.py bit for bit, the defaults, and the command-line tool's refusals of
-progressive, all made before a device is opened."""
import math
import os
import struct
import subprocess

import pytest

import gi_amd
import progressive_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "global-illumination_amd", "photonmap")


def bits(x):
    return struct.pack("<d", x)


@pytest.mark.parametrize("r0", [0.05, 0.1, 1.0])
@pytest.mark.parametrize("alpha", [0.5, 0.7, 0.999])
def test_radius_equals_the_restatement_bit_for_bit(r0, alpha):
    prev = math.inf
    for npass in (0, 1, 2, 8, 100, 4095):
        got = gi_amd.progressive_radius(r0, alpha, npass)
        assert bits(got) == bits(pref.radius(r0, alpha, npass)), (r0, alpha, npass)
        assert 0.0 < got < prev or npass == 0   # the schedule shrinks
        prev = got
    assert bits(gi_amd.progressive_radius(r0, alpha, 0)) == bits(math.sqrt(r0 * r0))


@pytest.mark.parametrize("r0,alpha,npass", [
    (0.0, 0.7, 0), (-0.1, 0.7, 0), (math.inf, 0.7, 0), (math.nan, 0.7, 0),
    (0.1, 0.0, 0), (0.1, 1.0, 0), (0.1, -0.5, 3), (0.1, 1.5, 3), (0.1, math.nan, 3),
    (0.1, 0.7, -1), (0.1, 0.7, 1 << 20), (0.1, 0.7, 1 << 40)])
def test_radius_is_nan_for_a_bad_argument(r0, alpha, npass):
    assert math.isnan(gi_amd.progressive_radius(r0, alpha, npass))
    assert math.isnan(pref.radius(r0, alpha, npass))


def test_last_valid_pass_index():
    got = gi_amd.progressive_radius(0.1, 0.7, (1 << 20) - 1)
    assert bits(got) == bits(pref.radius(0.1, 0.7, (1 << 20) - 1)) and got > 0.0


def test_params_default():
    p = gi_amd.progressive_params()
    assert (p.alpha, p.global_radius, p.caustic_radius) == (0.7, 0.0, 0.0)
    assert gi_amd.progressive_params(alpha=0.5, global_radius=0.2).global_radius == 0.2
    with pytest.raises(TypeError):
        gi_amd.progressive_params(beta=1.0)
    assert gi_amd.GI_ESTIMATE_ALL == 1 << 30


def run(args):
    assert os.path.exists(CLI), f"{CLI} not built (run __graft_entry__.build())"
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("flags", [
    ["-progressive", "0.7", "-adaptive", "8", "-noise", "0.05"],
    ["-progressive", "0.7", "-views", "VIEWS"],
    ["-progressive", "0.7", "-cache"],
    ["-progressive", "0.7", "-gpus", "2"],
    ["-progressive", "0"], ["-progressive", "1"], ["-progressive", "-0.2"],
    ["-progressive", "1.5"], ["-progressive", "nan"], ["-progressive", "x"], ["-progressive"],
], ids=lambda f: "_".join(f).replace("-", ""))
def test_cli_refusals_name_the_flag(flags, tmp_path):
    views = tmp_path / "v.txt"
    views.write_text("0.556 0.546 -1.6  0 0 1  0 1 0  0.329\n")
    flags = [str(views) if f == "VIEWS" else f for f in flags]
    out = tmp_path / "o.png"
    # the scene does not exist: reaching ReadScene would print its message instead
    r = run([str(tmp_path / "missing.scn"), str(out), "-resolution", "24", "16", "-passes", "2"] + flags)
    assert r.returncode != 0, r.stderr
    assert "-progressive" in r.stderr, r.stderr
    assert "missing.scn" not in r.stderr
    assert not out.exists()


def test_cli_accepts_a_good_flag(tmp_path):
    """With a good -progressive the run passes the argument stage: the next failure is the scene."""
    r = run([str(tmp_path / "missing.scn"), str(tmp_path / "o.png"), "-resolution", "24", "16",
             "-passes", "2", "-progressive", "0.7"])
    assert r.returncode != 0 and "-progressive" not in r.stderr and "Invalid" not in r.stderr
