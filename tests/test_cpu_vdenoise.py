"""The numpy restatement of the variance-guided denoise filter (tests/vdenoise_ref.py): its
properties on synthetic frames, and its quality on accumulated oracle frames against the
accumulated mean itself and against the fixed-sigma filter (tests/denoise_ref.py). No GPU: the
device kernels are compared with the same restatement in tests/test_gpu_vdenoise.py.
"""
import functools

import numpy as np
import pytest

import camera_cases
import denoise_ref
import feature_cases as fc
import oracle_lib
import radiance_ref
import vdenoise_ref as vr
from gpu_util import scene


def flat_planes(h, w, normal=(0.0, 0.0, 1.0), depth=2.0, albedo=(0.5, 0.5, 0.5), coverage=1.0):
    f = np.zeros((h, w), dtype=vr.FEATURE_DTYPE)
    f["normal"] = normal
    f["depth"] = depth
    f["albedo"] = albedo
    f["coverage"] = coverage
    return f


def var3(v):
    """Channel variances [H, W, 3] with the same value v [H, W] in every channel."""
    return np.repeat(np.asarray(v, dtype=np.float32)[..., None], 3, axis=-1)


# ---- restatement properties -----------------------------------------------------------------
def test_defaults_are_the_documented_ones():
    assert vr.DEFAULTS == dict(levels=5, normal_power_log2=5, sigma_lum=4.0, sigma_depth=0.05,
                               sigma_albedo=0.1, variance_floor=1e-6)


def test_luminance_variance_by_hand():
    v = np.float32([[[0.5, 0.25, 2.0], [0.0, 0.0, 0.0]]])
    want = np.float32((0.2126 * 0.2126) * 0.5 + (0.7152 * 0.7152) * 0.25 + (0.0722 * 0.0722) * 2.0)
    out = vr.lum_variance(v)
    assert out.dtype == np.float32 and out.tolist() == [[want, 0.0]]


def test_output_stays_inside_input_range():
    rng = np.random.default_rng(4)
    c = (40.0 * rng.random((21, 37, 3))).astype(np.float32)
    v = (10.0 * rng.random((21, 37, 3))).astype(np.float32)
    v[rng.random((21, 37)) < 0.2] = 0.0
    feat = flat_planes(21, 37)
    feat["depth"] = rng.uniform(1.0, 3.0, (21, 37)).astype(np.float32)
    feat["albedo"] = rng.random((21, 37, 3)).astype(np.float32)
    feat["coverage"][:, 30:] = 0.0
    out, vout = vr.denoise(c, v, feat)
    for ch in range(3):
        assert out[..., ch].min() >= c[..., ch].min()
        assert out[..., ch].max() <= c[..., ch].max()
    assert (out != c).any()
    assert vout.min() >= 0.0 and vout.max() <= vr.lum_variance(v).max()


def test_one_level_with_equal_planes_is_the_b3_blur():
    """All planes equal and sigma_lum huge: m = 1, dz = 0, xa = 0 and xl below 2^-53, so every
    weight is (h zz) / zz, which is h where zz is a power of two (depth 2, sigma_depth 0.5: zz =
    4): one level is the 5 x 5 B3 blur normalised at the borders, and v1 = sum h^2 v / (sum
    h)^2."""
    rng = np.random.default_rng(6)
    h, w = 13, 17
    c = (40.0 * rng.random((h, w, 3))).astype(np.float32)
    v0 = rng.uniform(0.1, 1.0, (h, w)).astype(np.float32)
    feat = flat_planes(h, w)
    out, vout = vr.denoise_lum(c, v0, feat, levels=1, sigma_lum=1e30, sigma_depth=0.5,
                               normal_power_log2=3)
    k = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625])
    sw = np.zeros((h, w))
    sc = np.zeros((h, w, 3))
    sv = np.zeros((h, w))
    c64, v64 = c.astype(np.float64), v0.astype(np.float64)
    for j in range(-2, 3):          # the same tap order
        for i in range(-2, 3):
            for y in range(max(0, -j), min(h, h - j)):
                for x in range(max(0, -i), min(w, w - i)):
                    hh = k[i + 2] * k[j + 2]
                    sw[y, x] += hh
                    sc[y, x] += hh * c64[y + j, x + i]
                    sv[y, x] += (hh * hh) * v64[y + j, x + i]
    np.testing.assert_array_equal(out, (sc / sw[..., None]).astype(np.float32))
    np.testing.assert_array_equal(vout, (sv / (sw * sw)).astype(np.float32))
    assert sw.min() == 9 / 64 + 2 * 3 / 32 + 2 * 3 / 128 + 1 / 16 + 2 / 64 + 1 / 256  # a corner


def test_step_edge_with_depth_and_normal_step_keeps_both_sides():
    """Left half: one plane, right half: a perpendicular one further away. n_p . n_q = 0 across
    the edge, so no weight crosses it and each side's colour stays exactly, whatever the
    variance says."""
    h, w = 16, 24
    feat = flat_planes(h, w)
    feat["normal"][:, w // 2:] = (1.0, 0.0, 0.0)
    feat["depth"][:, w // 2:] = 4.0
    c = np.zeros((h, w, 3), dtype=np.float32)
    c[:, :w // 2] = np.float32([0.2, 3.0, 0.4])
    c[:, w // 2:] = np.float32([9.0, 0.8, 0.7])
    v = np.full((h, w, 3), 5.0, dtype=np.float32)
    out, vout = vr.denoise(c, v, feat)
    np.testing.assert_array_equal(out, c)
    assert vout.max() < vr.lum_variance(v).max()   # ... while each side was averaged
    # with noise on each side the sides stay apart and each gets smoother
    rng = np.random.default_rng(5)
    noisy = (c + rng.uniform(-0.05, 0.05, c.shape)).astype(np.float32)
    out, _ = vr.denoise(noisy, var3(np.full((h, w), 0.05 * 0.05 / 3)), feat)
    assert out[:, :w // 2, 0].max() < 1.0 < out[:, w // 2:, 0].min()
    assert out[:, :w // 2].std(axis=(0, 1)).max() < noisy[:, :w // 2].std(axis=(0, 1)).min()


def test_more_input_variance_moves_a_region_further_towards_its_neighbourhood():
    h, w = 15, 19
    feat = flat_planes(h, w)
    c = np.full((h, w, 3), 1.0, dtype=np.float32)
    region = (slice(6, 9), slice(8, 11))
    c[region] = 2.0
    moved = []
    for rv in (0.01, 0.1, 1.0, 10.0):
        v = np.full((h, w), 0.01, dtype=np.float32)
        v[region] = rv
        out, _ = vr.denoise(c, var3(v), feat, levels=2)
        moved.append(float(c[region].astype(np.float64).mean()
                           - out[region].astype(np.float64).mean()))
    print("moved towards the neighbourhood:", moved)
    assert moved[0] > 0.0
    assert all(b > a for a, b in zip(moved, moved[1:])), moved


def test_prefilter_weights_by_hand():
    """3 x 3, k3 = {1/2, 1/4}: a corner sees 4 taps, an edge 6, the interior 9."""
    v = np.arange(1, 21, dtype=np.float32).reshape(4, 5)   # v[y, x] = 5 y + x + 1
    g = vr.prefiltered_variance(v)
    a, b, d = 0.25, 0.125, 0.0625   # centre, side, diagonal
    # corner (0, 0): taps in j-outer, i-inner order (0,0) (1,0) (0,1) (1,1)
    assert g[0, 0] == (a * 1 + b * 2 + b * 6 + d * 7) / (a + b + b + d)
    # bottom edge (y 0, x 2): (1,0) (2,0) (3,0) (1,1) (2,1) (3,1)
    assert g[0, 2] == (b * 2 + a * 3 + b * 4 + d * 7 + b * 8 + d * 9) / (b + a + b + d + b + d)
    # interior (y 1, x 1)
    num = d * 1 + b * 2 + d * 3 + b * 6 + a * 7 + b * 8 + d * 11 + b * 12 + d * 13
    assert g[1, 1] == num / 1.0
    il = vr.inverse_bandwidth(v, 4.0, 1e-6)
    assert il[1, 1] == 1.0 / (16.0 * g[1, 1] + 1e-6)
    # a plane of zeros: the floor alone
    assert (vr.inverse_bandwidth(np.zeros((3, 3), np.float32), 4.0, 1e-6) == 1.0 / 1e-6).all()


@pytest.mark.parametrize("levels", [1, 8])
def test_single_pixel_image_is_returned_unchanged(levels):
    c = np.float32([[[0.1, 37.5, 0.33333334]]])
    v = np.float32([[[0.5, 0.25, 2.0]]])
    for cov in (1.0, 0.0):
        out, vout = vr.denoise(c, v, flat_planes(1, 1, coverage=cov), levels=levels)
        np.testing.assert_array_equal(out, c)
        np.testing.assert_array_equal(vout, vr.lum_variance(v))


def test_unknown_parameter_is_refused():
    with pytest.raises(AssertionError):
        vr.denoise(np.zeros((2, 2, 3), np.float32), np.zeros((2, 2, 3), np.float32),
                   flat_planes(2, 2), sigma_color=1.0)


def test_accumulator_inputs_are_what_accum_get_returns():
    rng = np.random.default_rng(8)
    acc = radiance_ref.Accum((3, 4))
    for S in (1, 4, 2):
        acc.add(rng.random((3, 4, 3)) * 3.0, rng.random((3, 4, 3)), S)
    mean, var, n, _noise = acc.get()
    c, v0 = vr.accum_inputs(acc.mu, acc.A, np.full((3, 4), n))
    np.testing.assert_array_equal(c, mean)
    np.testing.assert_array_equal(v0, vr.lum_variance(var))
    # a pixel with fewer than two samples has variance 0
    counts = np.full((3, 4), n)
    counts[0, 0] = 1
    assert vr.accum_inputs(acc.mu, acc.A, counts)[1][0, 0] == 0.0


# ---- quality on accumulated oracle frames ---------------------------------------------------
def file_kd(path):
    """kd of the scene file's `material` lines, in file order."""
    with open(path) as f:
        return np.array([[float(x) for x in ln.split()[4:7]] for ln in f
                         if ln.lstrip().startswith("material")])


def quality_args(tail):
    return [camera_cases.dimmed_cornell(), "/tmp/x.png"] + fc.QUALITY_FLAGS + tail


@functools.lru_cache(maxsize=None)
def quality_fixture():
    """(passes: eight oracle frames -it 4 under seeds 1..8, the converged -it 256 -seed 99
    frame, the planes from the oracle's own intersections) of the dimmed cornell, 48 x 32."""
    w, h = fc.QUALITY_W, fc.QUALITY_H
    passes = [oracle_lib.render_float(quality_args(["-it", "4", "-seed", str(s)]), w, h)[0]
              for s in range(1, 9)]
    conv = oracle_lib.render_float(quality_args(["-it", "256", "-seed", "99"]), w, h)[0]
    args = quality_args(["-it", "4", "-seed", "1"])
    rays, _ids = oracle_lib.camera_rays(args)
    hit, _t, p, n, m = oracle_lib.intersect(args[0], rays["org"], rays["dir"])
    depth = oracle_lib.math("sqrt", denoise_ref.sample_depth(rays["org"], p))
    table = file_kd(scene("cornell.scn"))
    assert m[hit != 0].max() < len(table)
    feat = fc.planes((hit != 0, n, depth, m), w, h, 1, table)
    return passes, conv, feat


def test_converged_quality_frame_is_mostly_unclamped():
    """The oracle clamps its frame to [0, 1]: the comparison below means something only where
    few values sit at the clamp (measured 3.0 %)."""
    _passes, conv, _feat = quality_fixture()
    share = float((conv >= 1.0).mean())
    print(f"values >= 1 in the converged frame: {100 * share:.1f} %")
    assert share <= 0.10


@pytest.mark.parametrize("npass", [2, 8])
def test_quality_beats_the_accumulated_mean_and_the_fixed_sigma_filter(npass):
    """One sample per pixel and pass (S = 1, M2 = 0) folded by radiance_ref.Accum; RMSE to the
    converged frame. Recorded (DESIGN.md "Variance-guided denoise"), accumulated mean /
    denoise_ref.denoise / variance-guided: 2 passes 0.0867 / 0.0728 / 0.0465, 8 passes 0.0479 /
    0.0716 / 0.0372."""
    passes, conv, feat = quality_fixture()
    acc = radiance_ref.Accum((fc.QUALITY_H, fc.QUALITY_W))
    for f in passes[:npass]:
        acc.add(f.astype(np.float64), np.zeros(f.shape), 1)
    mean, var, n, _noise = acc.get()
    assert n == npass
    fixed = denoise_ref.denoise(mean, feat)
    guided, _v = vr.denoise(mean, var, feat)
    e_mean, e_fixed, e_guided = fc.rmse(mean, conv), fc.rmse(fixed, conv), fc.rmse(guided, conv)
    print(f"{npass} passes, rmse to the converged frame: mean {e_mean:.4f}, fixed sigma "
          f"{e_fixed:.4f}, variance-guided {e_guided:.4f}")
    assert e_guided < e_mean
    assert e_guided < e_fixed
