"""gi_denoise_radiance and gi_accum_denoise against their numpy restatement
(tests/vdenoise_ref.py), bit for bit: the filtered colour and the filtered luminance variance.

The rendered frame is the stilllife view of test_gpu_denoise.py at 37 x 21 and aa 1 (a variance
needs more than one sample): not a multiple of the 64 x 4 block, and the steps 32 to 128 of eight
levels exceed the frame. Synthetic 131 x 11 and 65 x 5 frames span several blocks in x and y; a
1 x 1 frame has the centre tap alone. The accumulator is filtered where it lies, after whole-frame
passes and after a masked one (unequal counts), and stays as it was.
"""
import ctypes as C

import numpy as np
import pytest

import camera_cases as cc
import gi_amd
import vdenoise_ref as vr
from gpu_util import scene

pytestmark = pytest.mark.gpu

W, H = 37, 21
# test_gpu_denoise.FLAGS at aa 1
FLAGS = ["-resolution", str(W), str(H), "-aa", "1", "-global", "5000", "-caustic", "5000",
         "-it", "4", "-tt", "2", "-st", "2", "-seed", "2"]
ARGS = [scene("stilllife.scn"), "/tmp/x.png"] + FLAGS
CW, CH = 24, 16
OTHER = dict(levels=4, normal_power_log2=0, sigma_lum=1.7, sigma_depth=0.21, sigma_albedo=0.033,
             variance_floor=3e-4)


def same_bits(dev, ref, what):
    dev, ref = np.ascontiguousarray(dev), np.ascontiguousarray(ref)
    assert dev.dtype == ref.dtype == np.float32 and dev.shape == ref.shape, (dev.shape, ref.shape)
    a, b = dev.view(np.uint32), ref.view(np.uint32)
    nd = int((a != b).sum())
    print(f"{what}: {nd} of {a.size} values differ")
    assert nd == 0, (what, np.argwhere(a != b)[:8].tolist())


def check(dev, ref):
    same_bits(dev[0], ref[0], "colour")
    same_bits(dev[1], ref[1], "luminance variance")


def make_context(args, camera=None):
    p, sc, _o, _w, _h, aa, real = gi_amd.ParseArgs(args)
    r = gi_amd.Renderer(0, p)
    r.ReadScene(sc, real)
    if camera is not None:
        r.set_camera(*camera)
    r.MapPhotons()
    return r, p, aa


@pytest.fixture(scope="module")
def still():
    """A context of its own holding the stilllife scene, and its (mean, variance, planes). Do
    not modify."""
    r, _p, aa = make_context(ARGS)
    mean, var, _st = r.render_radiance(aa, W, H)
    feat = r.camera_features(aa, W, H)
    for a in (mean, var, feat):
        a.setflags(write=False)
    cov = feat["coverage"] > 0
    v0 = vr.lum_variance(var)
    print(f"covered {cov.mean():.3f}, v0 > 0 on {(v0[cov] > 0).mean():.3f} of them, "
          f"largest mean value {mean.max():.3f}")
    assert cov.any() and (~cov).any()          # both coverage classes
    assert (v0[cov] > 0).mean() >= 0.5
    assert mean.max() > 1.0                     # unclamped
    yield dict(r=r, mean=mean, var=var, feat=feat)
    r.close()


@pytest.mark.parametrize("levels", [1, 3, 5, 8])
def test_filter_matches_restatement(still, levels):
    mean, var, feat = still["mean"], still["var"], still["feat"]
    out, vlum, ms = still["r"].denoise_radiance(mean, var, feat, levels=levels)
    ref = vr.denoise(mean, var, feat, levels=levels)
    assert (ref[0] != mean).any() and (ref[1] != vr.lum_variance(var)).any()
    check((out, vlum), ref)
    assert ms > 0.0


def test_filter_matches_restatement_with_other_parameters(still):
    mean, var, feat = still["mean"], still["var"], still["feat"]
    out, vlum, _ms = still["r"].denoise_radiance(mean, var, feat, **OTHER)
    check((out, vlum), vr.denoise(mean, var, feat, **OTHER))
    # every parameter matters on this frame
    for k in OTHER:
        par = dict(OTHER)
        par[k] = vr.DEFAULTS[k] if k != "levels" else 3
        o2, v2, _ms = still["r"].denoise_radiance(mean, var, feat, **par)
        assert (o2 != out).any() or (v2 != vlum).any(), k


def test_default_parameters_and_single_outputs(still):
    p = gi_amd.default_vdenoise_params()
    assert {k: getattr(p, k) for k in vr.DEFAULTS} == vr.DEFAULTS
    mean, var, feat = still["mean"], still["var"], still["feat"]
    L, ctx = gi_amd.lib(), still["r"]._ctx
    ref = vr.denoise(mean, var, feat)
    out = np.zeros((H, W, 3), dtype=np.float32)
    vlum = np.zeros((H, W), dtype=np.float32)
    # p == NULL means the defaults
    rc = L.gi_denoise_radiance(ctx, W, H, mean.ctypes.data, var.ctypes.data, feat.ctypes.data,
                               None, out.ctypes.data, vlum.ctypes.data, None)
    assert rc == gi_amd.GI_OK
    check((out, vlum), ref)
    # each output alone
    out1 = np.zeros_like(out)
    rc = L.gi_denoise_radiance(ctx, W, H, mean.ctypes.data, var.ctypes.data, feat.ctypes.data,
                               None, out1.ctypes.data, None, None)
    assert rc == gi_amd.GI_OK
    same_bits(out1, ref[0], "colour alone")
    vlum1 = np.zeros_like(vlum)
    rc = L.gi_denoise_radiance(ctx, W, H, mean.ctypes.data, var.ctypes.data, feat.ctypes.data,
                               None, None, vlum1.ctypes.data, None)
    assert rc == gi_amd.GI_OK
    same_bits(vlum1, ref[1], "variance alone")


def synthetic(rng, w, h):
    """Random planes with uncovered pixels next to covered ones and next to each other (as
    test_gpu_denoise's synthetic frame), colour in [0, 40), variance a mixture of exact 0, 1e-12
    and values up to 10."""
    c = (40.0 * rng.random((h, w, 3))).astype(np.float32)
    v = (10.0 * rng.random((h, w, 3))).astype(np.float32)
    kind = rng.choice(3, size=(h, w), p=[0.2, 0.2, 0.6])
    v[kind == 0] = 0.0
    v[kind == 1] = 1e-12
    feat = np.zeros((h, w), dtype=gi_amd.FEATURE_DTYPE)
    n = rng.normal(size=(h, w, 3))
    feat["normal"] = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    feat["normal"][:, :w // 2 + 5] = (0.0, 0.6, 0.8)
    feat["depth"] = rng.uniform(1.0, 1.2, (h, w)).astype(np.float32)
    feat["albedo"] = (0.5 + 0.05 * rng.random((h, w, 3))).astype(np.float32)
    feat["coverage"] = rng.choice([0.0, 0.25, 1.0], size=(h, w), p=[0.3, 0.2, 0.5])
    return c, v, feat


@pytest.mark.parametrize("w,h", [(131, 11), (65, 5), (1, 1)])
def test_synthetic_frames_over_several_blocks_need_no_scene(w, h):
    """A fresh context: no scene, no maps."""
    c, v, feat = synthetic(np.random.default_rng(11), w, h)
    r = gi_amd.Renderer(0)
    try:
        for levels in (2, 8):
            out, vlum, _ms = r.denoise_radiance(c, v, feat, levels=levels)
            check((out, vlum), vr.denoise(c, v, feat, levels=levels))
        if (w, h) == (1, 1):
            same_bits(out, c, "single pixel")
            same_bits(vlum, vr.lum_variance(v), "single pixel's variance")
    finally:
        r.close()


# ---- the accumulator ------------------------------------------------------------------------
def cornell_args():
    return [cc.dimmed_cornell(), "/tmp/x.png"] + cc.CORNELL_FLAGS


CORNELL_CAMERA = cc.camera_of(cc.CASES["cornell_dim"][1])


@pytest.fixture(scope="module")
def cornell():
    """A context of its own on the dimmed cornell view, 24 x 16, aa 1, with its planes."""
    r, p, aa = make_context(cornell_args(), CORNELL_CAMERA)
    assert aa == 1
    feat = r.camera_features(1, CW, CH)
    feat.setflags(write=False)
    yield dict(r=r, p=p, feat=feat)
    r.close()


def three_passes(d):
    r, p = d["r"], d["p"]
    r.accum_reset(CW, CH)
    for s in (5, 6, 7):
        p.seed = s
        r.set_params(p)
        r.accum_add_image(1)


def check_accum_denoise(d, **par):
    """accum_denoise = denoise_radiance(accum_get) = the restatement, and the accumulator is
    the same before and after."""
    r, feat = d["r"], d["feat"]
    mean, var, n, noise = r.accum_get()
    counts, total = r.accum_get_counts()
    out, vlum, ms = r.accum_denoise(feat, **par)
    assert ms > 0.0
    check((out, vlum), r.denoise_radiance(mean, var, feat, **par)[:2])
    check((out, vlum), vr.denoise(mean, var, feat, **par))
    assert (out != mean).any()
    mean2, var2, n2, noise2 = r.accum_get()
    counts2, total2 = r.accum_get_counts()
    assert mean2.tobytes() == mean.tobytes() and var2.tobytes() == var.tobytes()
    assert (n2, noise2, total2) == (n, noise, total)
    np.testing.assert_array_equal(counts2, counts)
    return counts


def test_accumulator_after_whole_frame_passes(cornell):
    three_passes(cornell)
    counts = check_accum_denoise(cornell)
    assert (counts == 12).all()
    check_accum_denoise(cornell, **OTHER)


def test_accumulator_after_a_checkerboard_pass(cornell):
    three_passes(cornell)
    r, p = cornell["r"], cornell["p"]
    tx, ty = (CW + 7) // 8, (CH + 7) // 8
    mask = (np.add.outer(np.arange(ty), np.arange(tx)) % 2).astype(np.uint8)
    p.seed = 8
    r.set_params(p)
    active, _st = r.accum_add_tiles(1, 8, mask.ravel())
    assert 0 < active < CW * CH
    counts = check_accum_denoise(cornell, levels=3)
    assert sorted(np.unique(counts).tolist()) == [12, 16]


def test_release_scratch_then_the_same_bits(cornell):
    three_passes(cornell)
    r, feat = cornell["r"], cornell["feat"]
    mean, var, _n, _noise = r.accum_get()
    a = r.accum_denoise(feat)
    b = r.denoise_radiance(mean, var, feat)
    r.release_scratch()
    check(r.accum_denoise(feat)[:2], a[:2])
    r.release_scratch()
    check(r.denoise_radiance(mean, var, feat)[:2], b[:2])


# ---- errors ---------------------------------------------------------------------------------
def rc_accum_denoise(r, feat, w, h, params=None):
    out = np.zeros((h, w, 3), dtype=np.float32)
    return gi_amd.lib().gi_accum_denoise(r._ctx, feat.ctypes.data,
                                         None if params is None else C.byref(params),
                                         out.ctypes.data, None, None)


def test_accumulator_state_errors(cornell):
    feat = cornell["feat"]
    fresh = gi_amd.Renderer(0)
    try:
        assert rc_accum_denoise(fresh, feat, CW, CH) == gi_amd.GI_ERR_STATE   # no reset yet
        with pytest.raises(gi_amd.GiError, match="rc=4"):
            fresh.accum_denoise(feat)
    finally:
        fresh.close()
    # one sample per pixel: no variance yet
    r, p = cornell["r"], cornell["p"]
    r.accum_reset(CW, CH)
    assert rc_accum_denoise(r, feat, CW, CH) == gi_amd.GI_ERR_STATE           # N = 0
    p.seed = 5
    r.set_params(p)
    r.accum_add_image(0)
    assert r.accum_get()[2] == 1
    assert rc_accum_denoise(r, feat, CW, CH) == gi_amd.GI_ERR_STATE
    assert b"2 samples" in gi_amd.lib().gi_last_error(r._ctx)
    r.accum_add_image(0)
    assert rc_accum_denoise(r, feat, CW, CH) == gi_amd.GI_OK                  # N = 2


def test_argument_errors(still, cornell):
    mean, var, feat = still["mean"], still["var"], still["feat"]
    L, ctx = gi_amd.lib(), still["r"]._ctx
    out = np.zeros((H, W, 3), dtype=np.float32)
    vlum = np.zeros((H, W), dtype=np.float32)
    mp, vp, tp, op, lp = (a.ctypes.data for a in (mean, var, feat, out, vlum))

    def call(w=W, h=H, m=mp, v=vp, planes=tp, o=op, ol=lp, **par):
        p = gi_amd.default_vdenoise_params(**par)
        return L.gi_denoise_radiance(ctx, w, h, m, v, planes, C.byref(p), o, ol, None)

    assert call() == gi_amd.GI_OK
    bad = [call(w=0), call(h=-1), call(w=65536, h=32768), call(m=None), call(v=None),
           call(planes=None), call(o=None, ol=None), call(levels=0), call(levels=9),
           call(normal_power_log2=-1), call(normal_power_log2=9)]
    names = ("sigma_lum", "sigma_depth", "sigma_albedo", "variance_floor")
    for name in names:
        bad += [call(**{name: x}) for x in (0.0, -1.0, float("nan"), float("inf"))]
    assert bad == [gi_amd.GI_ERR_ARG] * len(bad)
    assert L.gi_denoise_radiance(None, W, H, mp, vp, tp, None, op, lp, None) == gi_amd.GI_ERR_ARG
    # the accumulator's call: the same parameter checks, null planes, no output
    three_passes(cornell)
    r, cfeat = cornell["r"], cornell["feat"]
    assert rc_accum_denoise(r, cfeat, CW, CH) == gi_amd.GI_OK
    bad = [rc_accum_denoise(r, cfeat, CW, CH, gi_amd.default_vdenoise_params(**{k: x}))
           for k, x in [("levels", 0), ("levels", 9), ("normal_power_log2", 9)]
           + [(name, x) for name in names for x in (0.0, float("nan"))]]
    bad.append(L.gi_accum_denoise(r._ctx, None, None, out.ctypes.data, None, None))
    bad.append(L.gi_accum_denoise(r._ctx, cfeat.ctypes.data, None, None, None, None))
    bad.append(L.gi_accum_denoise(None, cfeat.ctypes.data, None, out.ctypes.data, None, None))
    assert bad == [gi_amd.GI_ERR_ARG] * len(bad)
    with pytest.raises(TypeError):
        still["r"].denoise_radiance(mean, var, feat, sigma_color=1.0)
    with pytest.raises(ValueError):
        still["r"].denoise_radiance(mean[:, :-1], var, feat)
    with pytest.raises(ValueError):
        r.accum_denoise(feat)          # the stilllife's planes: not the accumulator's size


def test_device_set_filters_a_given_frame_but_not_the_accumulator(still):
    mean, var, feat = still["mean"], still["var"], still["feat"]
    r = gi_amd.Renderer(devices=[0, 0])
    try:
        out, vlum, _ms = r.denoise_radiance(mean, var, feat)
        assert rc_accum_denoise(r, feat, W, H) == gi_amd.GI_ERR_UNSUPPORTED
    finally:
        r.close()
    check((out, vlum), still["r"].denoise_radiance(mean, var, feat)[:2])
