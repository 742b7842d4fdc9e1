"""The oracle's ray entries (oracle_render_rays, oracle_camera_rays) checked on the CPU, and the
ray-batch fixtures of ray_cases.py checked for their power to show an error. No GPU.

- replay: render_rays on camera_rays returns render's 8-bit image, render_float's float image
  and the nine counters bit for bit (render_image and oracle_camera_rays share one ray function,
  oracle_render_rays restates the per-ray body and the box filter);
- camera formula: camera_rays against the pinhole formula of render.cpp:64-117 recomputed in
  numpy longdouble from the .scn camera numbers, within 4 ulp of each component;
- depth of field: lens origins inside the aperture disk, distinct, aimed at the far-plane point;
- fixture conditions: >= 60 % of a batch's rays hit, >= 60 % of its float values in (0, 1);
- sensitivity: the stilllife light-field batch with every origin moved to the eye differs in
  more than 20 % of its pixels (what that does and does not show: the test's docstring).
"""
import numpy as np
import pytest

import oracle_lib
import ray_cases
from camera_cases import CASES, CORNELL_FLAGS, JENSEN_FLAGS, camera_of
from gpu_util import scene

LD = np.longdouble
FOCUS_DEPTH = 100.0  # the default far-plane distance (-dof's second number replaces it)


def _with(flags, width, height, aa):
    f = list(flags)
    i = f.index("-resolution")
    f[i + 1], f[i + 2] = str(width), str(height)
    f[f.index("-aa") + 1] = str(aa)
    return f


@pytest.mark.parametrize("scn,flags", [("cornell.scn", CORNELL_FLAGS), ("jensen.scn", JENSEN_FLAGS)],
                         ids=["cornell_aa1", "jensen_aa0"])
def test_replay_of_camera_rays_is_the_render(scn, flags):
    args = [scene(scn), "/tmp/x.png"] + flags
    rgb, st = oracle_lib.render(args, 24, 16)
    f, rgb_f = oracle_lib.render_float(args, 24, 16)
    np.testing.assert_array_equal(rgb_f, rgb)
    rays, ids = oracle_lib.camera_rays(args)
    spp = 4 ** int(flags[flags.index("-aa") + 1])
    assert len(rays) == len(ids) == 24 * 16 * spp
    rgb1, f1, st1 = oracle_lib.render_rays(args, spp, rays, ids)
    np.testing.assert_array_equal(rgb1, rgb)
    np.testing.assert_array_equal(f1, f)
    for k in oracle_lib.COUNTER_KEYS:
        assert st1[k] == st[k], k
    print(scn, "replay equal: 8-bit, float and", {k: st1[k] for k in oracle_lib.COUNTER_KEYS})


def pinhole(eye, towards, up, xfov, width, height, aa, focus=FOCUS_DEPTH):
    """Far-plane points and ids of render.cpp:64-98 in longdouble, gi_camera_rays' order
    (dof_test = 1): returns (far_point [n, 3], dir [n, 3], ids [n])."""
    eye, towards, up = (np.array(v, dtype=LD) for v in (eye, towards, up))

    def norm(v):
        return v / np.sqrt((v * v).sum(-1, keepdims=True))
    t = norm(towards)
    r = norm(np.cross(t, up))
    u = np.cross(r, t)
    af = 2 ** aa
    Wf, Hf = width * af, height * af
    y, x, sj, si = np.meshgrid(np.arange(height), np.arange(width), np.arange(af), np.arange(af),
                               indexing="ij")
    i = (x * af + si).ravel()
    j = (y * af + sj).ravel()
    dx = (2 * (i - Wf // 2)).astype(LD) / LD(Wf)
    dy = (2 * (j - Hf // 2)).astype(LD) / LD(Hf)
    tan = np.tan(LD(xfov))
    far = (eye + t * LD(focus)) + np.outer(dx, r * tan * LD(focus)) + np.outer(dy, u * tan * LD(focus))
    ids = (j.astype(np.uint64) * np.uint64(Wf) + i.astype(np.uint64))
    return far, norm(far - eye), ids


CORNELL_CAM = ((0.556, 0.546, -1.6), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 0.329)


def _camera_rays_and_formula(path, cam4, width, height, aa):
    args = [path, "/tmp/x.png"] + _with(CORNELL_FLAGS, width, height, aa)
    rays, ids = oracle_lib.camera_rays(args)
    eye, towards, up, xfov = cam4
    _far, d, want_ids = pinhole(eye, towards, up, xfov, width, height, aa)
    assert len(rays) == width * height * 4 ** aa
    np.testing.assert_array_equal(ids, want_ids)
    assert (rays["org"] == np.array(eye)).all()
    return rays["dir"].astype(LD), d


@pytest.mark.parametrize("width,height,aa", [(24, 16, 1), (37, 21, 2), (5, 3, 0)],
                         ids=["24x16_aa1", "37x21_aa2", "5x3_aa0"])
def test_camera_rays_match_the_pinhole_formula(width, height, aa):
    """cornell.scn's file camera: direction error <= 4 fp64 ulp of each component's own
    magnitude (the three roundings of normalize -- sum of squares, sqrt, divide -- on top of the
    far-point sum's); the odd sizes exercise W / 2 (an integer division)."""
    got, d = _camera_rays_and_formula(scene("cornell.scn"), CORNELL_CAM, width, height, aa)
    d64 = d.astype(np.float64)
    err = np.abs(got - d) / np.spacing(np.abs(d64))
    print(f"{width}x{height} aa {aa}: max direction error {float(err.max()):.3f} ulp "
          "(of the component)")
    assert err.max() <= 4.0


def test_camera_rays_of_a_set_camera_match_the_pinhole_formula(tmp_path):
    """A further case, the rewritten cornell camera (towards and up neither unit nor orthogonal)
    at 37 x 21 aa 2: the triad construction. Here components pass through zero, and the
    far-point sum rounds at the magnitude of focus_depth (100) whatever the component's size, so
    an error counted in the component's own ulps has no bound (thousands near zero). The unit is
    therefore the component's ulp but no less than the ulp of 0.5, the unit vector's scale; the
    bound stays 4. The three file-camera cases above keep the strict unit."""
    from camera_cases import rewrite_scene
    cam = CASES["cornell"][1]
    path = rewrite_scene(scene("cornell.scn"), cam, tmp_path)
    got, d = _camera_rays_and_formula(path, camera_of(cam), 37, 21, 2)
    d64 = d.astype(np.float64)
    own = np.abs(got - d) / np.spacing(np.abs(d64))
    err = np.abs(got - d) / np.maximum(np.spacing(np.abs(d64)), np.spacing(0.5))
    print(f"set camera 37x21 aa 2: max direction error {float(err.max()):.3f} ulp of "
          f"max(component, 0.5); {float(own.max()):.0f} in the component's own ulps")
    assert err.max() <= 4.0


def test_depth_of_field_rays():
    focus, aperture, dof = 12.2282, 0.025, 4
    args = [scene("teapot.scn"), "/tmp/x.png", "-resolution", "16", "16", "-aa", "1", "-dof",
            str(dof), str(focus), str(aperture)]
    rays, ids = oracle_lib.camera_rays(args)
    n = 16 * 16 * 4 * dof
    assert len(rays) == n
    pin, pin_ids = oracle_lib.camera_rays(args[:-4])  # the same frame without depth of field
    eye = pin["org"][0]
    assert (pin["org"] == eye).all()
    # teapot.scn has no camera line: the default camera looks along -z with up +y
    up, right = np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0])
    off = rays["org"] - eye
    assert np.abs(off[:, 2]).max() == 0.0                    # in the plane of up and right
    rad = np.sqrt((off ** 2).sum(-1))
    print("lens radius: max", float(rad.max()), "of", aperture)
    assert rad.max() <= aperture * (1 + 1e-15)
    assert rad.max() > 0.9 * aperture and rad.min() < 0.2 * aperture   # the disk is filled
    np.testing.assert_allclose(off, np.outer(off @ right, right) + np.outer(off @ up, up),
                               rtol=0, atol=1e-18)
    # the dof_test origins of a sub-cell are distinct; ids are (j * W + i) * dof_test + k
    cell = rays["org"].reshape(-1, dof, 3)
    for a in range(dof):
        for b in range(a + 1, dof):
            assert (cell[:, a] != cell[:, b]).any(-1).all()
    np.testing.assert_array_equal(ids.reshape(-1, dof),
                                  pin_ids[:, None] * np.uint64(dof) + np.arange(dof, dtype=np.uint64))
    # every direction points at its sub-cell's far-plane point: eye + pinhole direction * its
    # distance, the point at `focus` along towards (-z)
    far = eye + pin["dir"] * (focus / -pin["dir"][:, 2:3])
    want = np.repeat(far, dof, axis=0) - rays["org"]
    want /= np.sqrt((want ** 2).sum(-1, keepdims=True))
    # `far` is rebuilt from fp64 unit directions: a few ulp of the unit scale, not an exact bound
    err = np.abs(rays["dir"] - want).max()
    print("direction to the far-plane point: max abs error", float(err))
    assert err <= 1e-14


FIXTURES = [b + (ray_cases.W, ray_cases.H) for b in ray_cases.BATCHES] + [ray_cases.TILED_BATCH]


@pytest.mark.parametrize("case", FIXTURES, ids=lambda c: "-".join(str(v) for v in c))
def test_fixture_can_show_an_error(case):
    """Every batch the GPU tests use, judged on the oracle alone."""
    name, sensor, spp, width, height = case
    rays, _ids = ray_cases.batch(name, sensor, spp, width, height)
    _rgb, f, st = ray_cases.oracle_batch(name, sensor, spp, True, width, height)
    hit = ray_cases.hit_fraction(name, rays)
    inside = ray_cases.inside_fraction(f)
    print(f"{name} {sensor} spp {spp} {width}x{height}: hit {hit:.3f}, inside (0, 1) {inside:.3f}")
    assert st["screen_rays"] == round(hit * len(rays))
    assert hit >= 0.6
    assert inside >= 0.6


def test_shading_from_the_eye_would_show():
    """The stilllife light-field batch with every origin replaced by the eye (directions kept)
    must differ from the true one in more than 20 % of the pixels. This construction moves every
    ray, and so every hit point: a purely diffuse scene would pass it as well, and the share it
    measures (all pixels) says that the batch's origins matter, not that the view-dependent term
    is what shows. That a device shading from the camera's eye fails test_gpu_rays.py on this
    batch was shown by one such build, run once (1149 of 1152 float values off)."""
    name, sensor, spp = "stilllife", "lightfield", 3
    rays, ids = ray_cases.batch(name, sensor, spp)
    rgb, _f, _st = ray_cases.oracle_batch(name, sensor, spp)
    wrong = rays.copy()
    wrong["org"] = ray_cases.file_camera(ray_cases.scene_path(name))[0]
    rgb_w, _fw, _stw = oracle_lib.render_rays(ray_cases.scene_args(name), spp, wrong, ids)
    share = float((rgb_w != rgb).any(-1).mean())
    print(f"pixels that change when every ray starts at the eye: {share:.3f}")
    assert share > 0.2
