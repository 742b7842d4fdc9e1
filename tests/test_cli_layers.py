"""The drop-in CLI's extension flag -layers PREFIX: the frame's light-path layers as float means in
PREFIX_surface.pfm, _specular, _indirect, _global and _caustic, from gi_render_layers (one frame)
or from layered passes over five scene-less contexts (with a radiance flag); the usual image and
-radiance file do not change; with -vdenoise the written image is the tone map of the separately
filtered layers' sum. The refused combinations exit 1 before a device is opened.
"""
import os
import subprocess

import numpy as np
import pytest

import camera_cases as cc
import gi_amd
import layers_ref as lr
import pngio
import radiance_ref as rr
from gpu_util import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "global-illumination_amd", "photonmap")
W, H = 24, 16
SEED = 5  # CORNELL_FLAGS' -seed
FLAGS = cc.CORNELL_FLAGS + ["-it", "4"]


def run(args, timeout=300):
    assert os.path.exists(CLI), f"{CLI} not built (run __graft_entry__.build())"
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("tail", [
    ["-adaptive", "-noise", "0.05"],
    ["-views", "v.txt"],
    ["-progressive", "0.7"],
    ["-save_accum", "a.acc"],
    ["-load_accum", "a.acc"],
    ["-gpus", "2"],
    ["-passes", "2", "-gpus", "2"],
])
def test_refused_combinations_exit_1(tail, tmp_path):
    out = tmp_path / "o.png"
    # the scene does not exist: reaching ReadScene would print its message and exit -1
    r = run([str(tmp_path / "missing.scn"), str(out), "-layers", str(tmp_path / "p")] + tail)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert r.stderr.startswith("-layers ") and "not with" in r.stderr
    assert not out.exists() and not list(tmp_path.glob("p_*"))


def test_missing_prefix_is_an_argument_error(tmp_path):
    r = run([str(tmp_path / "missing.scn"), str(tmp_path / "o.png"), "-layers"])
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert r.stderr == "Invalid program argument: -layers"


@pytest.fixture(scope="module")
def api():
    """A context of its own on cornell.scn under FLAGS with three layered passes (seeds 5, 6, 7)
    folded: (renderer, the five layer contexts)."""
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs([scene("cornell.scn"), "/tmp/x.png"] + FLAGS)
    assert (w, h, aa, p.seed, p.indirect_test) == (W, H, 1, SEED, 4)
    r = gi_amd.Renderer(0, p)
    layers = [gi_amd.Renderer(0) for _ in range(lr.COUNT)]
    r.ReadScene(sc, real)
    r.MapPhotons()
    r.accum_reset(W, H)
    for x in layers:
        x.accum_reset(W, H)
    for i in range(3):
        p.seed = SEED + i
        r.set_params(p)
        r.accum_add_image_layers(1, layers)
    p.seed = SEED
    r.set_params(p)
    yield r, layers
    for x in layers + [r]:
        x.close()


def layer_files(prefix):
    return [rr.read_pfm(f"{prefix}_{name}.pfm") for name in lr.NAMES]


@pytest.mark.gpu
def test_passes_write_the_layers_and_leave_the_usual_outputs(api, tmp_path):
    r, layers = api
    base = [scene("cornell.scn")]
    png, pfm = str(tmp_path / "a.png"), str(tmp_path / "a.pfm")
    png0, pfm0 = str(tmp_path / "b.png"), str(tmp_path / "b.pfm")
    prefix = str(tmp_path / "lay")
    c = run(base + [png] + FLAGS + ["-layers", prefix, "-passes", "3", "-radiance", pfm])
    assert c.returncode == 0, c.stderr
    c0 = run(base + [png0] + FLAGS + ["-passes", "3", "-radiance", pfm0])
    assert c0.returncode == 0, c0.stderr
    assert open(png, "rb").read() == open(png0, "rb").read()
    assert open(pfm, "rb").read() == open(pfm0, "rb").read()
    assert rr.read_pfm(pfm)[1] == r.accum_get()[0].tobytes()
    lit = 0
    for l, (img, raw) in enumerate(layer_files(prefix)):
        assert img.shape == (H, W, 3)
        assert raw == layers[l].accum_get()[0].tobytes(), lr.NAMES[l]
        lit += bool(img.any())
    assert lit >= 3


@pytest.mark.gpu
def test_one_frame_writes_the_layers_of_gi_render_layers(api, tmp_path):
    r, _layers = api
    png, png0 = str(tmp_path / "a.png"), str(tmp_path / "b.png")
    prefix = str(tmp_path / "lay")
    c = run([scene("cornell.scn"), png] + FLAGS + ["-layers", prefix])
    assert c.returncode == 0, c.stderr
    c0 = run([scene("cornell.scn"), png0] + FLAGS)
    assert c0.returncode == 0, c0.stderr
    assert open(png, "rb").read() == open(png0, "rb").read()
    mean = r.render_layers(1, W, H)[0]
    for l, (_img, raw) in enumerate(layer_files(prefix)):
        assert raw == mean[l].tobytes(), lr.NAMES[l]


@pytest.mark.gpu
def test_vdenoise_filters_the_layers_apart(api, tmp_path):
    r, layers = api
    feat = r.camera_features(1, W, H)
    parts = [x.accum_get()[0] if l == lr.SPECULAR else x.accum_denoise(feat, levels=3)[0]
             for l, x in enumerate(layers)]
    summed = lr.filtered_sum(parts)
    want = r.tonemap(summed, 0.5, 4.0)
    png, prefix = str(tmp_path / "out.png"), str(tmp_path / "lay")
    c = run([scene("cornell.scn"), png] + FLAGS
            + ["-layers", prefix, "-passes", "3", "-vdenoise", "3", "-exposure", "0.5", "-white", "4"])
    assert c.returncode == 0, c.stderr
    np.testing.assert_array_equal(pngio.read_png(png)[::-1], want)
    np.testing.assert_array_equal(want, rr.quantize(rr.tonemap(summed, 0.5, 4.0)))
    # not the undivided filter's image, and the layer files hold the unfiltered means
    whole = r.accum_denoise(feat, levels=3)[0]
    assert (want != r.tonemap(whole, 0.5, 4.0)).any()
    for l, (_img, raw) in enumerate(layer_files(prefix)):
        assert raw == layers[l].accum_get()[0].tobytes(), lr.NAMES[l]
