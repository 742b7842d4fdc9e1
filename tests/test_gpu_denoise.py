"""gi_denoise against its numpy restatement (tests/denoise_ref.py), bit for bit.

The frame is a rendered stilllife view of 37 x 21 pixels with its device planes: not a multiple
of the 64 x 4 block, and every step up to 16 (and, at 8 levels, up to 128) meets the borders.
A synthetic 131 x 11 frame spans several blocks in x and y. Also: out_rgb8 = gi_quantize of
out_rgbf, a {0, 0} device set, the CLI's -denoise, and the argument errors.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref
import gi_amd
import pngio
from gpu_util import scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "global-illumination_amd", "photonmap")
W, H = 37, 21
FLAGS = ["-resolution", str(W), str(H), "-aa", "0", "-global", "5000", "-caustic", "5000",
         "-it", "4", "-tt", "2", "-st", "2", "-seed", "2"]
ARGS = [scene("stilllife.scn"), "/tmp/x.png"] + FLAGS


def render_with_planes(r):
    p, sc, _out, w, h, aa, real = gi_amd.ParseArgs(ARGS)
    r.set_params(p)
    r.ReadScene(sc, real)
    r.MapPhotons()
    _rgb, f, _st = r.RenderImage(aa, w, h, want_float=True)
    return f, r.camera_features(aa, w, h)


@pytest.fixture(scope="module")
def frame(renderer):
    """(noisy float frame, its device planes) of the stilllife view. Do not modify."""
    f, feat = render_with_planes(renderer)
    f.setflags(write=False)
    feat.setflags(write=False)
    cov = feat["coverage"]
    assert (cov > 0).any() and (cov == 0).any()  # edges between surface and background
    return f, feat


def assert_same_bits(dev, ref):
    a, b = dev.view(np.uint32), ref.view(np.uint32)
    nd = int((a != b).sum())
    print(f"{nd} of {a.size} values differ")
    assert nd == 0, np.argwhere(a != b)[:8].tolist()


@pytest.mark.parametrize("levels", [1, 3, 5, 8])
def test_filter_matches_restatement(renderer, frame, levels):
    f, feat = frame
    rgb, out, ms = renderer.denoise(f, feat, want_float=True, levels=levels)
    ref = denoise_ref.denoise(f, feat, levels=levels)
    assert (ref != f).any()
    assert_same_bits(out, ref)
    # out_rgb8 = gi_quantize(out_rgbf)
    q = np.zeros((H, W, 3), dtype=np.uint8)
    assert gi_amd.lib().gi_quantize(W, H, out.ctypes.data, q.ctypes.data) == gi_amd.GI_OK
    np.testing.assert_array_equal(rgb, q)
    np.testing.assert_array_equal(rgb, denoise_ref.quantize(ref))
    assert ms > 0.0


def test_filter_matches_restatement_with_other_parameters(renderer, frame):
    f, feat = frame
    par = dict(levels=4, normal_power_log2=0, sigma_color=0.37, sigma_depth=0.21,
               sigma_albedo=0.033)
    _rgb, out, _ms = renderer.denoise(f, feat, want_float=True, **par)
    assert_same_bits(out, denoise_ref.denoise(f, feat, **par))
    assert (out != renderer.denoise(f, feat, want_float=True, levels=4)[1]).any()


def test_default_parameters_are_the_documented_ones(renderer, frame):
    p = gi_amd.default_denoise_params()
    assert {k: getattr(p, k) for k in denoise_ref.DEFAULTS} == denoise_ref.DEFAULTS
    f, feat = frame
    # p == NULL means the defaults
    out0 = np.zeros((H, W, 3), dtype=np.float32)
    rc = gi_amd.lib().gi_denoise(renderer._ctx, W, H, f.ctypes.data, feat.ctypes.data, None,
                                 out0.ctypes.data, None, None)
    assert rc == gi_amd.GI_OK
    assert_same_bits(out0, denoise_ref.denoise(f, feat))
    # only the 8-bit image
    rgb = np.zeros((H, W, 3), dtype=np.uint8)
    rc = gi_amd.lib().gi_denoise(renderer._ctx, W, H, f.ctypes.data, feat.ctypes.data, None,
                                 None, rgb.ctypes.data, None)
    assert rc == gi_amd.GI_OK
    np.testing.assert_array_equal(rgb, denoise_ref.quantize(out0))


def test_synthetic_frame_over_several_blocks_needs_no_scene():
    """131 x 11: three blocks across, three up; random planes with uncovered pixels next to
    covered ones and next to each other. A fresh context: no scene, no maps."""
    rng = np.random.default_rng(11)
    w, h = 131, 11
    f = rng.random((h, w, 3)).astype(np.float32)
    feat = np.zeros((h, w), dtype=gi_amd.FEATURE_DTYPE)
    n = rng.normal(size=(h, w, 3))
    feat["normal"] = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    feat["normal"][:, :70] = (0.0, 0.6, 0.8)
    feat["depth"] = rng.uniform(1.0, 1.2, (h, w)).astype(np.float32)
    feat["albedo"] = (0.5 + 0.05 * rng.random((h, w, 3))).astype(np.float32)
    feat["coverage"] = rng.choice([0.0, 0.25, 1.0], size=(h, w), p=[0.3, 0.2, 0.5])
    r = gi_amd.Renderer(0)
    try:
        for levels in (2, 8):
            _rgb, out, _ms = r.denoise(f, feat, want_float=True, levels=levels)
            assert_same_bits(out, denoise_ref.denoise(f, feat, levels=levels))
    finally:
        r.close()


def test_device_set_returns_the_same_planes_and_image(renderer, frame):
    f, feat = frame
    r = gi_amd.Renderer(devices=[0, 0])
    try:
        f2, feat2 = render_with_planes(r)
        np.testing.assert_array_equal(f2, f)
        assert feat2.tobytes() == feat.tobytes()
        rgb2, out2, _ms = r.denoise(f2, feat2, want_float=True)
    finally:
        r.close()
    rgb, out, _ms = renderer.denoise(f, feat, want_float=True)
    assert_same_bits(out2, out)
    np.testing.assert_array_equal(rgb2, rgb)


def test_cli_denoise_writes_the_filtered_frame(renderer, frame, tmp_path):
    f, feat = frame
    png = str(tmp_path / "dn.png")
    r = subprocess.run([CLI, ARGS[0], png] + FLAGS + ["-denoise", "5"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rgb, _ms = renderer.denoise(f, feat, levels=5)
    np.testing.assert_array_equal(pngio.read_png(png)[::-1], rgb)
    # ... and is not the plain render
    plain = str(tmp_path / "plain.png")
    r = subprocess.run([CLI, ARGS[0], plain] + FLAGS, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (pngio.read_png(plain) != pngio.read_png(png)).any()


def test_denoise_argument_errors(renderer, frame):
    f, feat = frame
    L, ctx = gi_amd.lib(), renderer._ctx
    out = np.zeros((H, W, 3), dtype=np.float32)
    fp, tp, op = f.ctypes.data, feat.ctypes.data, out.ctypes.data

    def call(w=W, h=H, rgbf=fp, planes=tp, o=op, **par):
        p = gi_amd.default_denoise_params()
        for k, v in par.items():
            setattr(p, k, v)
        return L.gi_denoise(ctx, w, h, rgbf, planes, C.byref(p), o, None, None)

    assert call() == gi_amd.GI_OK
    bad = [call(w=0), call(h=-1), call(w=65536, h=32768), call(rgbf=None), call(planes=None),
           call(o=None), call(levels=0), call(levels=9), call(normal_power_log2=-1),
           call(normal_power_log2=9)]
    for name in ("sigma_color", "sigma_depth", "sigma_albedo"):
        bad += [call(**{name: v}) for v in (0.0, -1.0, float("nan"), float("inf"))]
    assert bad == [gi_amd.GI_ERR_ARG] * len(bad)
    with pytest.raises(TypeError):
        renderer.denoise(f, feat, sigma=1.0)
    with pytest.raises(ValueError):
        renderer.denoise(f[:, :-1], feat)
