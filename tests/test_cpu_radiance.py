"""The numpy restatement of the radiance statistics, accumulator and tone map
(tests/radiance_ref.py), the float image writers (gi_write_image_float) and the oracle-side
fixture conditions of tests/test_gpu_radiance.py. No GPU: the device kernels are compared with
the same restatement there.
"""
import numpy as np
import pytest

import gi_amd
import oracle_lib
import radiance_ref as rr
import ray_cases
from camera_cases import CORNELL_FLAGS, dimmed_cornell


# ---- restatement properties -----------------------------------------------------------------
def two_pass(samples):
    s = np.asarray(samples, dtype=np.float64)
    m = s.mean(axis=-2)
    return m, ((s - m[..., None, :]) ** 2).sum(axis=-2)


@pytest.mark.parametrize("split", [(4, 4), (3, 5), (1, 16), (16, 1)])
def test_merge_of_two_parts_is_the_two_pass_statistics_of_the_whole(split):
    rng = np.random.default_rng(sum(split))
    a, b = split
    s = rng.gamma(2.0, 1.5, (5, 7, a + b, 3))   # unclamped radiance: positive, values above 1
    acc = rr.Accum((5, 7))
    acc.add_samples(s[:, :, :a], 1.0 / a)
    acc.add_samples(s[:, :, a:], 1.0 / b)
    m, m2 = two_pass(s)
    assert acc.N == a + b
    np.testing.assert_allclose(acc.mu, m, rtol=1e-12, atol=0)
    np.testing.assert_allclose(acc.A, m2, rtol=1e-12, atol=0)
    # three parts of unequal size
    acc3 = rr.Accum((5, 7))
    cuts = [0, 1, 1 + (a + b - 1) // 2, a + b]
    for lo, hi in zip(cuts, cuts[1:]):
        if hi > lo:
            acc3.add_samples(s[:, :, lo:hi], 1.0 / (hi - lo))
    np.testing.assert_allclose(acc3.mu, m, rtol=1e-12, atol=0)
    np.testing.assert_allclose(acc3.A, m2, rtol=1e-12, atol=1e-300)


def test_merge_into_an_empty_accumulator_is_the_identity():
    rng = np.random.default_rng(1)
    s = rng.gamma(2.0, 1.5, (4, 6, 3, 3))   # S = 3: (m * 3) / 3 need not be m
    m, m2 = rr.pass_stats(s, rr.box_weight(spp=3))
    acc = rr.Accum((4, 6))
    acc.add(m, m2, 3)
    assert acc.N == 3
    assert acc.mu.tobytes() == m.tobytes() and acc.A.tobytes() == m2.tobytes()
    mean, var, n, _noise = acc.get()
    mean1, var1 = rr.mean_variance(s, rr.box_weight(spp=3))
    assert mean.tobytes() == mean1.tobytes() and var.tobytes() == var1.tobytes() and n == 3


def test_one_sample_has_variance_zero():
    s = np.random.default_rng(2).random((3, 3, 1, 3)) * 4
    mean, var = rr.mean_variance(s, rr.box_weight(aa=0))
    np.testing.assert_array_equal(mean, s[:, :, 0].astype(np.float32))
    assert not var.any()


def test_noise_of_a_constant_frame_is_zero_and_of_a_known_one_is_known():
    s = np.full((21, 37, 4, 3), 0.625)
    acc = rr.Accum((21, 37))
    acc.add_samples(s, rr.box_weight(aa=1))
    acc.add_samples(s, rr.box_weight(aa=1))
    assert acc.get()[3] == 0.0
    # grey pixels with samples 0 and 2: mu = 1, variance of the mean = 2 / 1 / 2 = 1, Y = 1,
    # v = sum of the squared weights
    s = np.zeros((2, 300, 2, 3))   # 600 pixels: three blocks, the last one padded
    s[:, :, 1] = 2.0
    acc = rr.Accum((2, 300))
    acc.add_samples(s, 0.5)
    want = np.sqrt(sum(k * k for k in rr.LUMA)) / (sum(rr.LUMA) + 0.01)
    assert acc.get()[3] == pytest.approx(want, rel=1e-14)
    assert rr.noise(acc.mu, acc.A, 1) == 0.0


def test_noise_sum_is_the_padded_tree():
    """777 errors 1, 2, ...: the tree's block sums by hand."""
    rng = np.random.default_rng(3)
    mu = rng.random((21, 37, 3)) + 0.5
    A = rng.random((21, 37, 3))
    e = rr.pixel_errors(mu, A, 8)
    x = np.zeros(1024)
    x[:777] = e

    def tree(v):
        return v[0] if len(v) == 1 else tree(v[:len(v) // 2] + v[len(v) // 2:])
    want = (((0.0 + tree(x[0:256])) + tree(x[256:512])) + tree(x[512:768])) + tree(x[768:1024])
    assert rr.noise(mu, A, 8) == want / 777.0
    assert rr.noise(mu, A, 8) == pytest.approx(e.mean(), rel=1e-13)


def test_tone_curve_is_monotone_maps_white_to_one_and_is_clamped():
    x = np.linspace(0.0, 50.0, 4001, dtype=np.float32).reshape(1, -1, 1).repeat(3, axis=2)
    for white in (0.0, 0.5, 4.0, 30.0):
        for exposure in (0.25, 1.0, 3.0):
            y = rr.tonemap(x, exposure, white)
            assert y.dtype == np.float32
            assert (np.diff(y[0, :, 0].astype(np.float64)) >= 0).all()
            assert y.min() == 0.0 and y.max() <= 1.0
    for white in (0.5, 4.0, 30.0):
        w = np.full((1, 1, 3), white, dtype=np.float32)
        assert (rr.tonemap(w, 1.0, white) == 1.0).all()
        assert (rr.tonemap(w * np.float32(0.5), 2.0, white) == 1.0).all()
        assert (rr.tonemap(w * np.float32(0.99), 1.0, white) < 1.0).all()
    below = np.float32([[[0.0, 0.25, 0.999]]])
    np.testing.assert_array_equal(rr.tonemap(below), below)            # white 0: the identity
    np.testing.assert_array_equal(rr.tonemap(np.float32([[[-1.0, 1.5, 7.0]]])),
                                  np.float32([[[0.0, 1.0, 1.0]]]))


# ---- float image writers --------------------------------------------------------------------
def radiance_image(w, h, seed):
    rng = np.random.default_rng(seed)
    img = (rng.gamma(1.5, 2.0, (h, w, 3)) * 10.0 ** rng.integers(-6, 4, (h, w, 1))).astype(np.float32)
    img[0, 0] = 0.0                              # an all-zero pixel
    img[-1, -1] = (0.0, 3.0, 0.0)                # zero channels next to a bright one
    if w > 2:
        img[0, 2] = (1.0, 0.5, 0.25)             # on byte boundaries
        img[0, 1] = (1e-33, 1e-34, 0.0)          # below Ward's 1e-32: four zero bytes
    return img


@pytest.mark.parametrize("w,h", [(37, 21), (1, 1), (5, 3), (131, 11)])
def test_pfm_file_holds_the_array(tmp_path, w, h):
    img = radiance_image(w, h, w * h)
    path = str(tmp_path / "f.pfm")
    gi_amd.write_image_float(path, img)
    back, raw = rr.read_pfm(path)
    assert back.shape == (h, w, 3)
    assert raw == img.tobytes()                  # rows bottom to top: the project's row order
    with open(path, "rb") as f:
        assert f.read().startswith(b"PF\n%d %d\n-1.0\n" % (w, h))


@pytest.mark.parametrize("w,h", [(37, 21), (1, 1), (5, 3), (131, 11)])
def test_hdr_pixels_decode_to_the_input(tmp_path, w, h):
    img = radiance_image(w, h, w * h + 1)
    path = str(tmp_path / "f.hdr")
    gi_amd.write_image_float(path, img)
    head, res, px = rr.read_hdr(path)
    assert head[0] == b"#?RADIANCE" and b"FORMAT=32-bit_rle_rgbe" in head
    assert res == b"-Y %d +X %d" % (h, w)
    px = px[::-1]                                # the file's first scanline is the top row
    c = img.astype(np.float64)
    zero = c.max(axis=-1) < 1e-32
    assert (w * h == 1 or zero[0, 0]) and (w <= 2 or zero[0, 1])
    assert not px[zero].any()
    assert (px[~zero][:, 3] > 0).all()
    step = np.ldexp(1.0, px[..., 3].astype(np.int64) - 136)[..., None]
    err = np.abs(c - px[..., :3] * step)
    assert (err[~zero] < np.broadcast_to(step, err.shape)[~zero]).all()
    # Ward's encoding: the largest channel's byte is at least 128, bytes are truncated
    assert (px[~zero][:, :3].max(axis=-1) >= 128).all()
    assert ((px[..., :3] * step)[~zero] <= c[~zero]).all()
    if w > 2:
        assert px[0, 2].tolist() == [128, 64, 32, 129]


def test_float_writer_refuses_other_extensions(tmp_path):
    img = radiance_image(5, 3, 0)
    L = gi_amd.lib()
    for name in ("f.png", "f.exr", "f.pfm2", "f", "f.HDR"):
        rc = L.gi_write_image_float(str(tmp_path / name).encode(), 5, 3, img.ctypes.data)
        assert rc == gi_amd.GI_ERR_ARG, name
        assert not (tmp_path / name).exists()
    assert L.gi_write_image_float(str(tmp_path / "f.pfm").encode(), 0, 3, img.ctypes.data) \
        == gi_amd.GI_ERR_ARG
    assert L.gi_write_image_float(str(tmp_path / "f.pfm").encode(), 5, 3, None) == gi_amd.GI_ERR_ARG
    with pytest.raises(gi_amd.GiError):
        gi_amd.write_image_float(str(tmp_path / "f.tga"), img)


# ---- fixture conditions, from the oracle alone ----------------------------------------------
@pytest.mark.parametrize("name,sensor,spp", rr.ORACLE_BATCHES)
def test_oracle_batches_have_most_values_inside_the_clamp(name, sensor, spp):
    """A clamped oracle value pins its sample from one side only: at least 60 % of a batch's
    values lie strictly inside (0, 1) (measured: 67.8 % and 91.2 %)."""
    f = rr.oracle_samples(name, sensor, spp)
    inside = ray_cases.inside_fraction(f)
    print(f"{name} {sensor} spp {spp}: {inside:.3f} of the sample values inside (0, 1)")
    assert inside >= 0.6
    # the per-ray frame reproduces the oracle's own spp-ray frame: clamp, sum in order, 1 / spp
    want = ray_cases.oracle_batch(name, sensor, spp)[1]
    got = rr.clamped_frame(f.astype(np.float64), rr.box_weight(spp=spp))[0]
    assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.maximum(got, want))).all()


def test_mean_of_eight_oracle_passes_is_closer_to_the_converged_frame_than_one():
    """Dimmed cornell 24 x 16, -it 4 under seeds 1..8 against one -it 256 frame: accumulation
    converges. A property, not a tolerance."""
    flags = list(CORNELL_FLAGS)
    flags[flags.index("-aa") + 1] = "0"

    def frame(it, seed):
        f = list(flags)
        f[f.index("-it") + 1] = str(it)
        f[f.index("-seed") + 1] = str(seed)
        return oracle_lib.render_float([dimmed_cornell(), "/tmp/x.png"] + f, 24, 16)[0]

    conv = frame(256, 99).astype(np.float64)
    passes = [frame(4, s).astype(np.float64) for s in range(1, 9)]
    acc = rr.Accum((16, 24))
    for p in passes:
        acc.add(p, np.zeros_like(p), 1)
    np.testing.assert_allclose(acc.mu, np.mean(passes, axis=0), rtol=1e-12, atol=1e-15)

    def rmse(a):
        return float(np.sqrt(((a - conv) ** 2).mean()))
    one, eight = rmse(passes[0]), rmse(acc.mu)
    print(f"rmse to the -it 256 frame: one pass {one:.4f}, mean of eight {eight:.4f}")
    assert eight < one
