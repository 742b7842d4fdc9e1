"""The drop-in CLI's extension flag -vdenoise L: one of the radiance flags (-passes defaults to
1, one device); after the passes the accumulator is filtered by L levels of the variance-guided
pass (gi_camera_features + gi_accum_denoise, other parameters default) and the written image is
gi_tonemap of the filtered mean, while -radiance FILE keeps the unfiltered one. Like the other
extension flags it is taken out of argv before gi_parse_args: a malformed one, or one next to
-denoise, is the reference's "Invalid program argument" line and exit 1.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import camera_cases as cc
import gi_amd
import pngio
import radiance_ref as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "global-illumination_amd", "photonmap")
W, H = 24, 16
SEED = 5  # CORNELL_FLAGS' -seed


def run(args, timeout=300):
    assert os.path.exists(CLI), f"{CLI} not built (run __graft_entry__.build())"
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("tail", [
    ["-vdenoise", "0"],
    ["-vdenoise", "9"],
    ["-vdenoise"],                                     # missing
    ["-vdenoise", "2.5"],
    ["-vdenoise", "3", "-denoise", "3"],
    ["-denoise", "3", "-passes", "2", "-vdenoise", "3"],
])
def test_malformed_flag_is_an_argument_error(tail, tmp_path):
    out = tmp_path / "o.png"
    # the scene does not exist: reaching ReadScene would print its message and exit -1
    r = run([str(tmp_path / "missing.scn"), str(out)] + tail)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert r.stderr == "Invalid program argument: -vdenoise"
    assert r.stdout == ""
    assert not out.exists()


def test_flag_is_removed_before_parse_args_and_needs_one_device(tmp_path):
    r = run([str(tmp_path / "missing.scn"), str(tmp_path / "o.png"), "-aa", "1", "-vdenoise", "3",
             "-no_shadow"])
    assert r.returncode == 255, (r.returncode, r.stderr)
    assert "Invalid program argument" not in r.stderr
    r = run([str(tmp_path / "missing.scn"), str(tmp_path / "o.png"), "-vdenoise", "3", "-gpus", "2"])
    assert r.returncode == 255, (r.returncode, r.stderr)
    assert "one device" in r.stderr and "-gpus 2" in r.stderr
    with pytest.raises(ValueError, match=r"^Invalid program argument: -vdenoise$"):
        gi_amd.ParseArgs(["a.scn", "b.png", "-vdenoise", "3"])


@pytest.fixture(scope="module")
def api():
    """A context of its own on the dimmed cornell (the file's camera), maps built."""
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs([cc.dimmed_cornell(), "/tmp/x.png"]
                                                 + cc.CORNELL_FLAGS)
    assert (w, h, aa, p.seed) == (W, H, 1, SEED)
    r = gi_amd.Renderer(0, p)
    r.ReadScene(sc, real)
    r.MapPhotons()
    yield r, p
    r.close()


def test_written_image_is_the_tone_mapped_filtered_accumulator(api, tmp_path):
    r, p = api
    r.accum_reset(W, H)
    for i in range(3):
        p.seed = SEED + i
        r.set_params(p)
        r.accum_add_image(1)
    p.seed = SEED
    r.set_params(p)
    mean = r.accum_get()[0]
    filtered, _vlum, _ms = r.accum_denoise(r.camera_features(1, W, H), levels=3)
    assert (filtered != mean).any()
    want = r.tonemap(filtered, 0.5, 4.0)
    png, pfm = str(tmp_path / "out.png"), str(tmp_path / "m.pfm")
    c = run([cc.dimmed_cornell(), png] + cc.CORNELL_FLAGS
            + ["-passes", "3", "-vdenoise", "3", "-exposure", "0.5", "-white", "4", "-radiance", pfm,
               "-v"])
    assert c.returncode == 0, c.stderr
    np.testing.assert_array_equal(pngio.read_png(png)[::-1], want)
    np.testing.assert_array_equal(want, rr.quantize(rr.tonemap(filtered, 0.5, 4.0)))
    assert (want != r.tonemap(mean, 0.5, 4.0)).any()
    # the radiance file keeps the unfiltered mean
    assert rr.read_pfm(pfm)[1] == mean.tobytes()
    m = re.search(r"^Variance-guided denoise: (\d+) levels, (\S+) ms$", c.stdout, re.M)
    assert m, c.stdout
    assert int(m.group(1)) == 3 and float(m.group(2)) > 0.0
    assert re.search(r"^Accumulated image: 3 passes, N = 12 samples per pixel", c.stdout, re.M)


def test_one_sample_per_pixel_is_the_librarys_error(tmp_path):
    png = tmp_path / "out.png"
    flags = [f for f in cc.CORNELL_FLAGS]
    flags[flags.index("-aa") + 1] = "0"
    c = run([cc.dimmed_cornell(), str(png)] + flags + ["-vdenoise", "3"])
    assert c.returncode == 255, (c.returncode, c.stderr)
    assert "at least 2 samples" in c.stderr
    assert not png.exists()
