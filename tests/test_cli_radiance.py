"""The drop-in CLI's extension flags -passes N, -noise T, -exposure E, -white W and
-radiance FILE: passes under seed, seed + 1, ... from one photon-map build, folded into the
context's accumulator; the written image is gi_tonemap of the unclamped mean, FILE (.pfm / .hdr)
receives that mean. Like -camera and -denoise, the CLI takes the flags out of argv itself before
gi_parse_args: a malformed one is the reference's "Invalid program argument" line and exit 1,
raised before any device is opened or the scene file is looked at. Without any of the flags the
CLI's output is unchanged (tests/test_cli.py).
"""
import os
import re
import subprocess

import numpy as np
import pytest

import gi_amd
import pngio
import radiance_ref as rr
from camera_cases import CORNELL_FLAGS
from gpu_util import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "global-illumination_amd", "photonmap")
W, H = 24, 16


def run(args, timeout=300):
    assert os.path.exists(CLI), f"{CLI} not built (run __graft_entry__.build())"
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("flag,tail", [
    ("-passes", ["-passes"]),                          # missing
    ("-passes", ["-passes", "x"]),
    ("-passes", ["-passes", "2.5"]),                   # not an integer
    ("-passes", ["-passes", "0"]),                     # out of range
    ("-passes", ["-passes", "4097"]),
    ("-passes", ["-passes", "3", "-v", "-passes", "-1"]),   # the last one counts too
    ("-noise", ["-aa", "0", "-noise"]),
    ("-noise", ["-noise", "-0.5"]),
    ("-noise", ["-noise", "nan"]),
    ("-noise", ["-noise", "-no_shadow"]),              # a flag where T belongs
    ("-exposure", ["-exposure", "0"]),
    ("-exposure", ["-exposure", "-2"]),
    ("-exposure", ["-exposure", "inf"]),
    ("-exposure", ["-exposure", "1x"]),
    ("-white", ["-white", "-1"]),
    ("-white", ["-white"]),
    ("-radiance", ["-radiance"]),
    ("-radiance", ["-radiance", "f.png"]),             # neither .pfm nor .hdr
    ("-radiance", ["-radiance", "noextension"]),
])
def test_malformed_flag_is_an_argument_error(flag, tail, tmp_path):
    out = tmp_path / "o.png"
    # the scene does not exist: reaching ReadScene would print its message and exit -1
    r = run([str(tmp_path / "missing.scn"), str(out)] + tail)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert r.stderr == "Invalid program argument: " + flag
    assert r.stdout == ""
    assert not out.exists()


def test_flags_are_removed_before_parse_args(tmp_path):
    """Complete flags pass the argument stage wherever they stand: the next failure is the
    missing scene file (or, on a machine without a GPU, the device)."""
    flags = ["-passes", "3", "-aa", "0", "-noise", "0.01", "-exposure", "0.5", "-no_shadow",
             "-white", "4", "-radiance", str(tmp_path / "f.hdr")]
    r = run([str(tmp_path / "missing.scn"), str(tmp_path / "o.png")] + flags)
    assert r.returncode == 255, (r.returncode, r.stderr)
    assert "Invalid program argument" not in r.stderr
    assert not (tmp_path / "f.hdr").exists()
    r = run([str(tmp_path / "missing.scn"), str(tmp_path / "o.png")] + flags + ["-bogus"])
    assert r.returncode == 1
    assert r.stderr == "Invalid program argument: -bogus"
    with pytest.raises(ValueError, match=r"^Invalid program argument: -passes$"):
        gi_amd.ParseArgs(["a.scn", "b.png", "-passes", "3"])


def test_more_than_one_device_is_refused_with_a_message(tmp_path):
    r = run([str(tmp_path / "missing.scn"), str(tmp_path / "o.png"), "-passes", "2", "-gpus", "2"])
    assert r.returncode == 255, (r.returncode, r.stderr)
    assert "one device" in r.stderr and "-gpus 2" in r.stderr
    assert not (tmp_path / "o.png").exists()


@pytest.fixture(scope="module")
def api_passes(renderer):
    """(mean, variance, N, noise, screen rays so far) after one, two and three cornell passes
    under seeds 5, 6, 7 through the API."""
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs([scene("cornell.scn"), "/tmp/x.png"] + CORNELL_FLAGS)
    renderer.set_params(p)
    renderer.ReadScene(sc, real)
    renderer.MapPhotons()
    renderer.accum_reset(w, h)
    out, rays = [], 0
    for i in range(3):
        p.seed = 5 + i
        renderer.set_params(p)
        rays += renderer.accum_add_image(aa)["screen_rays"]
        out.append(renderer.accum_get() + (rays,))
    return out


@pytest.mark.gpu
def test_passes_and_radiance_file_equal_the_api(api_passes, tmp_path):
    png, pfm = str(tmp_path / "out.png"), str(tmp_path / "f.pfm")
    r = run([scene("cornell.scn"), png] + CORNELL_FLAGS + ["-passes", "3", "-radiance", pfm, "-v"])
    assert r.returncode == 0, r.stderr
    mean, _var, n, noise, screen_rays = api_passes[2]
    assert n == 12
    back, raw = rr.read_pfm(pfm)
    assert raw == mean.tobytes()
    assert back.max() > 1.0                                  # unclamped
    np.testing.assert_array_equal(pngio.read_png(png)[::-1], rr.quantize(rr.tonemap(mean)))
    m = re.search(r"^Accumulated image: (\d+) passes, N = (\d+) samples per pixel, noise = (\S+)$",
                  r.stdout, re.M)
    assert m, r.stdout
    assert (int(m.group(1)), int(m.group(2))) == (3, 12)
    assert float(m.group(3)) == pytest.approx(noise, rel=1e-5)
    # the reference's counters, summed over the passes
    assert f"# Screen Rays = {screen_rays}\n" in r.stdout


@pytest.mark.gpu
def test_exposure_white_hdr_and_denoise(renderer, api_passes, tmp_path):
    png, hdr = str(tmp_path / "out.png"), str(tmp_path / "f.hdr")
    r = run([scene("cornell.scn"), png] + CORNELL_FLAGS + ["-exposure", "0.25", "-passes", "2",
                                                          "-white", "4", "-radiance", hdr])
    assert r.returncode == 0, r.stderr
    mean = api_passes[1][0]
    tm = rr.tonemap(mean, 0.25, 4.0)
    np.testing.assert_array_equal(pngio.read_png(png)[::-1], rr.quantize(tm))
    want = str(tmp_path / "want.hdr")
    gi_amd.write_image_float(want, mean)
    assert open(hdr, "rb").read() == open(want, "rb").read()
    # -denoise filters the tone-mapped frame
    dn = str(tmp_path / "dn.png")
    r = run([scene("cornell.scn"), dn] + CORNELL_FLAGS + ["-exposure", "0.25", "-passes", "2",
                                                         "-white", "4", "-denoise", "3"])
    assert r.returncode == 0, r.stderr
    feat = renderer.camera_features(1, W, H)   # the shared context still holds the cornell scene
    rgb, _ms = renderer.denoise(tm, feat, levels=3)
    np.testing.assert_array_equal(pngio.read_png(dn)[::-1], rgb)


@pytest.mark.gpu
def test_noise_threshold_stops_the_passes(api_passes, tmp_path):
    png = str(tmp_path / "out.png")
    r = run([scene("cornell.scn"), png] + CORNELL_FLAGS + ["-passes", "5", "-noise", "1e9", "-v"])
    assert r.returncode == 0, r.stderr
    assert re.search(r"^Accumulated image: 1 passes, N = 4 samples per pixel, noise = ", r.stdout,
                     re.M), r.stdout
    np.testing.assert_array_equal(pngio.read_png(png)[::-1],
                                  rr.quantize(rr.tonemap(api_passes[0][0])))
    # a threshold of 0 is never met by this frame: every pass runs
    r = run([scene("cornell.scn"), png] + CORNELL_FLAGS + ["-passes", "2", "-noise", "0", "-v"])
    assert r.returncode == 0, r.stderr
    assert re.search(r"^Accumulated image: 2 passes, N = 8 ", r.stdout, re.M), r.stdout
