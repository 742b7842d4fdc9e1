"""Further views from resident photon maps: gi_get_camera / gi_set_camera / gi_camera_rays /
gi_render_rays (gi.h "views from resident photon maps").

- A set camera is checked against the oracle rendering a copy of the scene file whose `camera`
  line is rewritten (the oracle renders any .scn), with the photon maps built once, before the
  camera changes. The new cameras are non-square (24 x 16) with a non-orthogonal `up`. The float
  image is compared too (within one float32 ulp), and one case is a dimmed cornell, whose values
  are not mostly clamped.
- A ray batch replayed from the camera's own rays (camera_rays -> render_rays) must return
  RenderImage's float image, 8-bit image and counters bit for bit, across batches, slot-guard
  re-runs and the tile shards of a device set; a permuted or partly replaced batch shows that
  the image comes from the buffer.
"""
import numpy as np
import pytest

import gi_amd
from camera_cases import (CASES, CORNELL_FILE_CAMERA, CORNELL_FLAGS, camera_of, case_scene,
                          oracle_file_view, oracle_file_view_float, oracle_view,
                          oracle_view_float)
from gpu_util import compare_exact, compare_float_ulp, run_gpu, scene

pytestmark = pytest.mark.gpu

COUNTERS = ("screen_rays", "knn_queries", "knn_photons")
ALL_COUNTERS = ("screen_rays", "shadow_rays", "monte_carlo_rays", "transmissive_samples",
                "specular_samples", "indirect_samples", "caustic_samples", "knn_queries",
                "knn_photons")

def cornell_args(flags=CORNELL_FLAGS):
    return [scene("cornell.scn"), "/tmp/x.png"] + flags


# test 1's one-device float image of the cornell row, for the device-set test
_one_device = {}


@pytest.mark.parametrize("name", ["cornell", "jensen", "cornell_dim"])
def test_set_camera_matches_oracle_on_rewritten_scene(renderer, name):
    _scn, cam, flags = CASES[name]
    rgb0, _f0, _st0, _pst = run_gpu(renderer, [case_scene(name), "/tmp/x.png"] + flags,
                                    want_float=True)
    maps0 = [renderer.photon_map(m).copy() for m in (gi_amd.GLOBAL, gi_amd.CAUSTIC)]
    renderer.set_camera(*camera_of(cam))
    rgb1, f1, st1 = renderer.RenderImage(0 if name == "jensen" else 1, 24, 16, want_float=True)
    ref, ost = oracle_view(name)
    print(name, {k: (st1[k], ost[k]) for k in COUNTERS},
          "differs from file view:", float((rgb0 != rgb1).any(-1).mean()))
    compare_exact(rgb1, ref)
    for k in COUNTERS:
        assert st1[k] == ost[k], k
    compare_float_ulp(f1, oracle_view_float(name))
    for m, before in zip((gi_amd.GLOBAL, gi_amd.CAUSTIC), maps0):
        np.testing.assert_array_equal(renderer.photon_map(m), before)
    assert (rgb0 != rgb1).any(-1).mean() > 0.5  # the view really changed
    if name == "cornell":
        _one_device["f"] = f1


def test_get_camera_round_trip(renderer):
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(cornell_args())
    renderer.set_params(p)
    renderer.ReadScene(sc, real)
    assert renderer.get_camera() == CORNELL_FILE_CAMERA
    renderer.MapPhotons()
    _rgb, f0, _st = renderer.RenderImage(aa, w, h, want_float=True)
    renderer.set_camera(*renderer.get_camera())
    assert renderer.get_camera() == CORNELL_FILE_CAMERA
    _rgb, f1, _st = renderer.RenderImage(aa, w, h, want_float=True)
    np.testing.assert_array_equal(f1, f0)
    new = camera_of(CASES["cornell"][1])
    renderer.set_camera(*new)
    assert renderer.get_camera() == new
    renderer.ReadScene(sc, real)
    assert renderer.get_camera() == CORNELL_FILE_CAMERA


def test_get_camera_needs_a_scene():
    r = gi_amd.Renderer(0)
    try:
        with pytest.raises(gi_amd.GiError, match=rf"^rc={gi_amd.GI_ERR_STATE}\b"):
            r.get_camera()
    finally:
        r.close()


def test_set_camera_rejects_degenerate(renderer):
    _rgb, f0, _st, _pst = run_gpu(renderer, cornell_args(), want_float=True)
    eye, towards, up, xfov = CORNELL_FILE_CAMERA
    bad = [
        (eye, (0.0, 0.0, 0.0), up, xfov),                      # zero towards
        (eye, towards, (0.0, 0.0, 2.5), xfov),                 # up parallel to towards
        (eye, (0.3, -0.2, 1.0), (-0.6, 0.4, -2.0), xfov),      # ... antiparallel, off-axis
        (eye, towards, up, 0.0),                               # xfov 0
        (eye, towards, up, float(np.pi / 2)),                  # xfov at the open bound
        (eye, towards, up, float("nan")),                      # NaN
        ((float("nan"), 0.5, -1.6), towards, up, xfov),
        (eye, towards, (0.0, float("inf"), 0.0), xfov),
    ]
    for cam in bad:
        with pytest.raises(gi_amd.GiError, match=rf"^rc={gi_amd.GI_ERR_ARG}\b"):
            renderer.set_camera(*cam)
        assert renderer.get_camera() == CORNELL_FILE_CAMERA
    _rgb, f1, _st = renderer.RenderImage(1, 24, 16, want_float=True)
    np.testing.assert_array_equal(f1, f0)


def test_set_camera_on_device_set(renderer):
    if "f" not in _one_device:  # run on its own: test 1's one-device image
        run_gpu(renderer, cornell_args())
        renderer.set_camera(*camera_of(CASES["cornell"][1]))
        _one_device["f"] = renderer.RenderImage(1, 24, 16, want_float=True)[1]
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(cornell_args())
    r = gi_amd.Renderer(params=p, devices=[0, 0])
    try:
        r.ReadScene(sc, real)
        r.MapPhotons()
        r.RenderImage(aa, w, h)
        r.set_camera(*camera_of(CASES["cornell"][1]))
        rgb, f, _st = r.RenderImage(aa, w, h, want_float=True)
    finally:
        r.close()
    np.testing.assert_array_equal(f, _one_device["f"])
    compare_exact(rgb, oracle_view("cornell")[0])


def test_camera_rays_replay_is_exact(renderer):
    rgb0, f0, st0, _pst = run_gpu(renderer, cornell_args(), want_float=True)
    rays, ids = renderer.camera_rays(1, 24, 16)
    assert len(rays) == len(ids) == 24 * 16 * 4
    norm = np.sqrt((rays["dir"] ** 2).sum(-1))
    print("dir norm - 1: max abs", float(np.abs(norm - 1.0).max()))
    assert np.abs(norm - 1.0).max() <= 1e-15
    assert (rays["org"] == np.array(CORNELL_FILE_CAMERA[0])).all()
    assert len(np.unique(ids)) == len(ids)
    rgb1, f1, st1 = renderer.render_rays(24, 16, 4, rays, ids, want_float=True)
    np.testing.assert_array_equal(f1, f0)
    np.testing.assert_array_equal(rgb1, rgb0)
    for k in ALL_COUNTERS:
        assert st1[k] == st0[k], k
    ref, ost = oracle_file_view()
    compare_exact(rgb1, ref)
    for k in COUNTERS:
        assert st1[k] == ost[k], k
    compare_float_ulp(f1, oracle_file_view_float())


def test_render_rays_argument_checks(renderer):
    run_gpu(renderer, cornell_args())
    rays, ids = renderer.camera_rays(0, 4, 4)
    assert len(rays) == 16
    with pytest.raises(gi_amd.GiError, match=rf"^rc={gi_amd.GI_ERR_ARG}\b"):
        renderer.render_rays(4, 4, 0, rays, ids)
    st = gi_amd.RenderStats()
    L, ctx = gi_amd.lib(), renderer._ctx
    out = np.zeros((4, 4, 3), np.uint8)
    assert L.gi_render_rays(ctx, 4, 4, 1, None, None, out.ctypes.data, None, gi_amd.C.byref(st)) == gi_amd.GI_ERR_ARG
    # width * height * spp = 2^31 is refused before anything is read
    assert L.gi_render_rays(ctx, 1 << 15, 1 << 15, 2, rays.ctypes.data, None, out.ctypes.data,
                            None, gi_amd.C.byref(st)) == gi_amd.GI_ERR_ARG
    n = gi_amd.C.c_int64(0)
    assert L.gi_camera_rays(ctx, 0, 4, 4, rays.ctypes.data, None, 15, n) == gi_amd.GI_ERR_ARG
    assert n.value == 16


def _aa0_flags():
    flags = list(CORNELL_FLAGS)
    flags[flags.index("-aa") + 1] = "0"
    return flags


def test_render_rays_default_ids_at_aa0(renderer):
    # at -aa 0 the camera's stream id is the row-major pixel index, the default id of ray r
    rgb0, f0, st0, _pst = run_gpu(renderer, cornell_args(_aa0_flags()), want_float=True)
    rays, ids = renderer.camera_rays(0, 24, 16)
    np.testing.assert_array_equal(ids, np.arange(24 * 16, dtype=np.uint64))
    rgb1, f1, st1 = renderer.render_rays(24, 16, 1, rays, None, want_float=True)
    np.testing.assert_array_equal(f1, f0)
    np.testing.assert_array_equal(rgb1, rgb0)
    for k in ALL_COUNTERS:
        assert st1[k] == st0[k], k


def test_render_rays_uses_the_buffer(renderer):
    w, h = 24, 16
    _rgb0, f0, _st0, _pst = run_gpu(renderer, cornell_args(_aa0_flags()), want_float=True)
    rays, ids = renderer.camera_rays(0, w, h)
    # the ray and id of pixel p move to slot perm[p]
    perm = np.random.default_rng(11).permutation(w * h)
    prays, pids = np.empty_like(rays), np.empty_like(ids)
    prays[perm] = rays
    pids[perm] = ids
    _rgb, f1, _st = renderer.render_rays(w, h, 1, prays, pids, want_float=True)
    expect = np.empty_like(f0.reshape(-1, 3))
    expect[perm] = f0.reshape(-1, 3)
    np.testing.assert_array_equal(f1.reshape(-1, 3), expect)
    assert (f1 != f0).any()
    # left half: rays leaving the scene (the camera looks along +z from outside the box);
    # cornell.scn sets no background, so those pixels are the default black
    away = rays.copy().reshape(h, w)
    away["dir"][:, : w // 2] = (0.0, 0.0, -1.0)
    _rgb, f2, st2 = renderer.render_rays(w, h, 1, away.ravel(), ids, want_float=True)
    assert (f2[:, : w // 2] == 0.0).all()
    np.testing.assert_array_equal(f2[:, w // 2:], f0[:, w // 2:])
    assert (f0[:, : w // 2] > 0).any()
    assert 0 < st2["screen_rays"] <= w * h // 2


def test_render_rays_across_batches_and_tiles(renderer, monkeypatch):
    args = [scene("cornell.scn"), "/tmp/x.png", "-resolution", "37", "21", "-aa", "1",
            "-global", "20000", "-caustic", "20000", "-it", "96", "-tt", "8", "-st", "8",
            "-seed", "2"]
    _rgb0, f0, st0, _pst = run_gpu(renderer, args, want_float=True)
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(args)
    monkeypatch.setenv("GI_SLOT_LIMIT", "60000")
    for devices in (None, [0, 0]):
        r = gi_amd.Renderer(0, p, devices=devices)
        try:
            r.ReadScene(sc, real)
            r.MapPhotons()
            rays, ids = r.camera_rays(aa, w, h)
            _rgb, f1, st1 = r.render_rays(w, h, 4, rays, ids, want_float=True)
        finally:
            r.close()
        np.testing.assert_array_equal(f1, f0)
        for k in ALL_COUNTERS:
            assert st1[k] == st0[k], (devices, k)
