"""The numpy restatement of the denoise filter (tests/denoise_ref.py), the oracle-derived feature
fixtures (tests/feature_cases.py) and the filter's quality on oracle frames. No GPU: the device
kernels are compared with the same restatement in tests/test_gpu_denoise.py.
"""
import numpy as np
import pytest

import denoise_ref
import feature_cases as fc
import oracle_lib
from gpu_util import scene


def flat_planes(h, w, normal=(0.0, 0.0, 1.0), depth=2.0, albedo=(0.5, 0.5, 0.5), coverage=1.0):
    f = np.zeros((h, w), dtype=denoise_ref.FEATURE_DTYPE)
    f["normal"] = normal
    f["depth"] = depth
    f["albedo"] = albedo
    f["coverage"] = coverage
    return f


def file_kd(path):
    """kd of the scene file's `material` lines, in file order (the material index of a file
    whose shapes all name a material)."""
    with open(path) as f:
        return np.array([[float(x) for x in ln.split()[4:7]] for ln in f
                         if ln.lstrip().startswith("material")])


# ---- fixture conditions, from the oracle alone ----------------------------------------------
def test_stilllife_fixture_has_every_coverage_class_and_three_materials():
    s = fc.camera_samples("stilllife")
    full, part, empty = fc.coverage_classes(s, fc.camera_spp("stilllife"))
    nmat = len(np.unique(s[3][s[0]]))
    print(f"stilllife 24 x 16 aa 1: full {full:.3f} partial {part:.3f} empty {empty:.3f}, "
          f"{nmat} materials")
    assert full > 0 and part > 0 and empty > 0
    assert nmat >= 3


def test_ray_batch_fixtures():
    """The cornell panorama has rays that miss; the teapot frame has two lens samples a pixel."""
    hit = fc.batch_samples("cornell_dim", "panorama", 3)[0]
    assert 0 < hit.mean() < 1
    assert len(fc.camera_samples("teapot_dof")[0]) == 20 * 20 * 2
    assert fc.camera_samples("teapot_dof")[0].any()


def test_reduce_planes_by_hand():
    """Two pixels of three samples: one partly covered, one empty."""
    hit = [1, 0, 1, 0, 0, 0]
    n = np.array([[0, 0, 1], [9, 9, 9], [0, 1, 0], [9, 9, 9], [9, 9, 9], [9, 9, 9]], float)
    d = np.array([1.0, 99.0, 2.0, 99.0, 99.0, 99.0])
    kd = np.array([[0.2, 0.4, 0.6], [9, 9, 9], [0.4, 0.4, 0.2], [9, 9, 9], [9, 9, 9], [9, 9, 9]])
    p = denoise_ref.reduce_planes(2, 1, 3, hit, n, d, kd)
    assert p.shape == (1, 2)
    assert p["coverage"].tolist() == [[np.float32(2 / 3), 0.0]]
    assert p["normal"][0, 0].tolist() == [0.0, 0.5, 0.5]
    assert p["depth"].tolist() == [[1.5, 0.0]]
    np.testing.assert_array_equal(p["albedo"][0, 0],
                                  np.array([(0.2 + 0.4) / 2, (0.4 + 0.4) / 2, (0.6 + 0.2) / 2],
                                           dtype=np.float32))
    assert not p["normal"][0, 1].any() and not p["albedo"][0, 1].any()


# ---- restatement properties -----------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 5, 8])
def test_constant_image_is_returned_bit_for_bit(levels):
    rng = np.random.default_rng(3)
    feat = flat_planes(21, 37)
    feat["depth"] = rng.uniform(1.0, 3.0, (21, 37)).astype(np.float32)
    feat["coverage"][5:9, 7:20] = 0.0
    c = np.empty((21, 37, 3), dtype=np.float32)
    c[...] = np.float32([0.1, 0.7, 0.33333334])
    np.testing.assert_array_equal(denoise_ref.denoise(c, feat, levels=levels), c)


def test_output_stays_inside_input_range():
    rng = np.random.default_rng(4)
    c = rng.random((21, 37, 3)).astype(np.float32)
    feat = flat_planes(21, 37)
    feat["depth"] = rng.uniform(1.0, 3.0, (21, 37)).astype(np.float32)
    feat["albedo"] = rng.random((21, 37, 3)).astype(np.float32)
    feat["coverage"][:, 30:] = 0.0
    out = denoise_ref.denoise(c, feat)
    for ch in range(3):
        assert out[..., ch].min() >= c[..., ch].min()
        assert out[..., ch].max() <= c[..., ch].max()
    assert (out != c).any()


def test_step_edge_with_depth_and_normal_step_keeps_both_sides():
    """Left half: one plane, right half: a perpendicular one further away. n_p . n_q = 0
    across the edge, so no weight crosses it and each side's colour stays exactly."""
    h, w = 16, 24
    feat = flat_planes(h, w)
    feat["normal"][:, w // 2:] = (1.0, 0.0, 0.0)
    feat["depth"][:, w // 2:] = 4.0
    c = np.zeros((h, w, 3), dtype=np.float32)
    c[:, :w // 2] = np.float32([0.2, 0.3, 0.4])
    c[:, w // 2:] = np.float32([0.9, 0.8, 0.7])
    out = denoise_ref.denoise(c, feat)
    np.testing.assert_array_equal(out, c)
    # ... and with noise on each side the side means stay apart, nothing bleeds across
    rng = np.random.default_rng(5)
    noisy = (c + rng.uniform(-0.05, 0.05, c.shape)).astype(np.float32)
    out = denoise_ref.denoise(noisy, feat)
    assert out[:, :w // 2].max() < 0.5 < out[:, w // 2:].min()
    assert out[:, :w // 2].std() < noisy[:, :w // 2].std()


def test_one_level_with_equal_planes_is_the_b3_blur():
    """All planes equal and sigma_color huge: m = 1, xz = xa = 0 and xc below 2^-53 relative
    to 1, so every weight is h and one level is the 5 x 5 B3 blur normalised at the borders."""
    rng = np.random.default_rng(6)
    h, w = 13, 17
    c = rng.random((h, w, 3)).astype(np.float32)
    feat = flat_planes(h, w)
    out = denoise_ref.denoise(c, feat, levels=1, sigma_color=1e30, normal_power_log2=3)
    k = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625])
    sw = np.zeros((h, w))
    sc = np.zeros((h, w, 3))
    c64 = c.astype(np.float64)
    for j in range(-2, 3):          # the same tap order
        for i in range(-2, 3):
            for y in range(max(0, -j), min(h, h - j)):
                for x in range(max(0, -i), min(w, w - i)):
                    sw[y, x] += k[i + 2] * k[j + 2]
                    sc[y, x] += k[i + 2] * k[j + 2] * c64[y + j, x + i]
    np.testing.assert_array_equal(out, (sc / sw[..., None]).astype(np.float32))


def test_unknown_parameter_is_refused():
    with pytest.raises(AssertionError):
        denoise_ref.denoise(np.zeros((2, 2, 3), np.float32), flat_planes(2, 2), sigma=1.0)


# ---- quality on oracle frames ---------------------------------------------------------------
def test_filter_brings_a_noisy_oracle_frame_closer_to_the_converged_one():
    """cornell.scn 48 x 32, -it 4 against -it 256 (feature_cases.QUALITY_FLAGS). Planes from the
    oracle's own intersections of its camera rays; albedo = kd of the scene file's material
    lines (cornell.scn's shapes all name one). Recorded: rmse 0.1080 noisy, 0.0594 filtered,
    ratio 0.550 (DESIGN.md "Feature planes and denoise pass")."""
    args = fc.quality_args(fc.NOISY_FLAGS)
    rays, _ids = oracle_lib.camera_rays(args)
    hit, _t, p, n, m = oracle_lib.intersect(args[0], rays["org"], rays["dir"])
    depth = oracle_lib.math("sqrt", denoise_ref.sample_depth(rays["org"], p))
    table = file_kd(scene("cornell.scn"))
    assert m[hit != 0].max() < len(table)
    feat = fc.planes((hit != 0, n, depth, m), fc.QUALITY_W, fc.QUALITY_H, 1, table)
    noisy, conv = fc.quality_frames()
    filtered = denoise_ref.denoise(noisy, feat)
    e0, e1 = fc.rmse(noisy, conv), fc.rmse(filtered, conv)
    print(f"rmse to the converged frame: noisy {e0:.4f}, filtered {e1:.4f}, ratio {e1 / e0:.3f}")
    assert e1 < e0
