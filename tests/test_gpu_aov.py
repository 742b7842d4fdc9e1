"""Per-pixel feature planes (gi_camera_features / gi_ray_features) and gi_get_materials.

- The planes of three camera frames and two caller-made ray batches equal, bit for bit in every
  field of every pixel, the planes derived from the oracle's own rays and intersections
  (tests/feature_cases.py), with each material's kd from gi_get_materials.
- A frame that crosses the 2^22-sample chunk equals the same reduction of the device's own
  gi_camera_rays + gi_intersect_batch output (the oracle would need minutes for it).
- The feature calls need a scene, not the photon maps.
"""
import ctypes as C

import numpy as np
import pytest

import denoise_ref
import feature_cases as fc
import gi_amd
import ray_cases
from gpu_util import scene

pytestmark = pytest.mark.gpu


def load(renderer, args):
    """ParseArgs -> ReadScene, no photon maps."""
    p, sc, _out, w, h, aa, real = gi_amd.ParseArgs(args)
    renderer.set_params(p)
    renderer.ReadScene(sc, real)
    return w, h, aa


def assert_planes_equal(dev, ref):
    assert dev.dtype == gi_amd.FEATURE_DTYPE and dev.shape == ref.shape
    for f in ("normal", "depth", "albedo", "coverage"):
        a = np.ascontiguousarray(dev[f]).view(np.uint32)
        b = np.ascontiguousarray(ref[f]).view(np.uint32)
        nd = int((a != b).sum())
        print(f"{f}: {nd} of {a.size} values differ")
        assert nd == 0, (f, np.argwhere(a != b)[:8].tolist())


def test_feature_dtype_is_the_restatements():
    assert gi_amd.FEATURE_DTYPE == denoise_ref.FEATURE_DTYPE


@pytest.mark.parametrize("name", list(fc.CAMERA_CASES))
def test_camera_features_match_oracle(renderer, name):
    w, h, aa = load(renderer, fc.camera_args(name))
    dev = renderer.camera_features(aa, w, h)
    ref = fc.camera_planes(name, renderer.materials()["kd"])
    full, part, empty = fc.coverage_classes(fc.camera_samples(name), fc.camera_spp(name))
    print(f"{name}: full {full:.3f} partial {part:.3f} empty {empty:.3f}")
    assert (ref["coverage"] > 0).any()
    assert_planes_equal(dev, ref)


@pytest.mark.parametrize("name,sensor,spp", fc.RAY_BATCHES)
def test_ray_features_match_oracle(renderer, name, sensor, spp):
    load(renderer, ray_cases.scene_args(name))
    rays, _ids = ray_cases.batch(name, sensor, spp)
    dev = renderer.ray_features(ray_cases.W, ray_cases.H, spp, rays)
    ref = fc.batch_planes(name, sensor, spp, renderer.materials()["kd"])
    assert_planes_equal(dev, ref)


def test_frame_across_the_sample_chunk_matches_device_rays_and_intersections(renderer):
    """531 x 497 at aa 2: 4,222,512 samples, above one chunk of 2^22, cut at pixel 262,144."""
    w, h, aa = load(renderer, [scene("cornell.scn"), "/tmp/x.png", "-resolution", "531", "497",
                               "-aa", "2"])
    assert w * h * 16 > 1 << 22
    dev = renderer.camera_features(aa, w, h)
    rays, _ids = renderer.camera_rays(aa, w, h)
    hit, _t, p, n, m = renderer.Intersects(rays["org"], rays["dir"])
    depth = gi_amd.math_probe(renderer, "sqrt", denoise_ref.sample_depth(rays["org"], p))
    ref = fc.planes((hit != 0, n, depth, m), w, h, 16, renderer.materials()["kd"])
    assert_planes_equal(dev, ref)
    # the pixels on both sides of the cut are not empty
    flat = dev.reshape(-1)
    assert (flat["coverage"][(1 << 18) - 2:(1 << 18) + 2] > 0).all()


def test_features_do_not_need_photon_maps():
    r = gi_amd.Renderer(0)
    try:
        w, h, aa = load(r, fc.camera_args("cornell"))
        dev = r.camera_features(aa, w, h)
        assert_planes_equal(dev, fc.camera_planes("cornell", r.materials()["kd"]))
    finally:
        r.close()


MATERIAL_LINES = [
    # ka, kd, ks, kt, e, n, ir
    [0.1, 0.2, 0.3, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.0, 1.0, 2.0, 3.0, 12.0, 1.25],
    [0.0, 0.0, 0.0, 0.25, 0.5, 0.125, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 10.0, 1.0],
    [0.0, 0.0, 0.0, 0.3, 0.3, 0.3, 0.3, 0.2, 0.1, 0.9, 0.9, 0.9, 0.0, 0.0, 0.0, 500.0, 1.5],
]


@pytest.mark.parametrize("real", [False, True])
def test_get_materials_returns_the_scene_files_materials(renderer, tmp_path, real):
    path = tmp_path / "mats.scn"
    with open(path, "w") as f:
        f.write("camera 0 0 5  0 0 -1  0 1 0  0.4  0.01 100\npoint_light 1 1 1  0 3 3  0 0 1\n")
        for k, v in enumerate(MATERIAL_LINES):
            f.write("material " + " ".join(repr(x) for x in v) + " 0\n")
            f.write(f"sphere {k} {k - 1.0} 0 0 0.4\n")
    load(renderer, [str(path), "/tmp/x.png"] + (["-real"] if real else []))
    mats = renderer.materials()
    assert len(mats) == len(MATERIAL_LINES)
    for k, v in enumerate(MATERIAL_LINES):
        v = np.array(v)
        kd, ks, kt = v[3:6].copy(), v[6:9].copy(), v[9:12].copy()
        if real:  # R3Scene.cpp:1779-1793: the largest channel sum above 1 scales all three down
            mx = max(1.0, float((kd + ks + kt).max()))
            kd, ks, kt = kd / mx, ks / mx, kt / mx
        np.testing.assert_array_equal(mats[k]["ka"], v[0:3])
        np.testing.assert_array_equal(mats[k]["kd"], kd)
        np.testing.assert_array_equal(mats[k]["ks"], ks)
        np.testing.assert_array_equal(mats[k]["kt"], kt)
        np.testing.assert_array_equal(mats[k]["e"], v[12:15])
        assert mats[k]["n"] == v[15] and mats[k]["ir"] == v[16]
    if real:
        assert (mats[0]["kd"] != np.array(MATERIAL_LINES[0][3:6])).all()
    # the index is the one Intersects returns: a ray at each sphere
    org = np.array([[k - 1.0, 0.0, 5.0] for k in range(3)])
    hit, _t, _p, _n, m = renderer.Intersects(org, np.tile([0.0, 0.0, -1.0], (3, 1)))
    assert hit.all() and m.tolist() == [0, 1, 2]
    # capacity below the count is an argument error, a null buffer reports the count
    n = C.c_int32(0)
    one = np.zeros(1, dtype=gi_amd.MATERIAL_DTYPE)
    assert gi_amd.lib().gi_get_materials(renderer._ctx, one.ctypes.data, 1,
                                         C.byref(n)) == gi_amd.GI_ERR_ARG
    assert n.value == 3


def test_feature_calls_before_a_scene_are_state_errors():
    r = gi_amd.Renderer(0)
    try:
        rays = np.zeros(4, dtype=gi_amd.RAY_DTYPE)
        for call in (lambda: r.camera_features(0, 2, 2), lambda: r.ray_features(2, 2, 1, rays),
                     r.materials):
            with pytest.raises(gi_amd.GiError, match=rf"^rc={gi_amd.GI_ERR_STATE}\b"):
                call()
    finally:
        r.close()


def test_feature_argument_errors(renderer):
    load(renderer, fc.camera_args("cornell"))
    L, ctx = gi_amd.lib(), renderer._ctx
    out = np.zeros(16, dtype=gi_amd.FEATURE_DTYPE)
    rays = np.zeros(16, dtype=gi_amd.RAY_DTYPE)
    rays["dir"][:, 2] = 1.0
    o, r = out.ctypes.data, rays.ctypes.data
    bad = [
        L.gi_camera_features(ctx, 0, 4, 4, None),
        L.gi_camera_features(ctx, -1, 4, 4, o),
        L.gi_camera_features(ctx, 0, 0, 4, o),
        L.gi_camera_features(ctx, 0, 4, -3, o),
        L.gi_ray_features(ctx, 4, 4, 1, None, o),
        L.gi_ray_features(ctx, 4, 4, 1, r, None),
        L.gi_ray_features(ctx, 4, 4, 0, r, o),
        L.gi_ray_features(ctx, 0, 4, 1, r, o),
        L.gi_ray_features(ctx, 65536, 32768, 1, r, o),   # 2^31 samples
        L.gi_ray_features(ctx, 32768, 32768, 2, r, o),
    ]
    assert bad == [gi_amd.GI_ERR_ARG] * len(bad)
    assert L.gi_ray_features(ctx, 4, 4, 1, r, o) == gi_amd.GI_OK
