"""Radiance frames, the accumulator over passes and the tone map (gi.h "radiance frames,
accumulation over passes, tone map") on the device, against tests/radiance_ref.py bit for bit.

- the `samples` output is what the render itself clamps: clamp, sum and box weight in numpy give
  gi_render_image's float and 8-bit frames bit for bit, on a frame most of whose samples clamp
  (and whose unclamped mean therefore differs from the clamped frame) and on a depth-of-field
  frame (a sample = the mean of its lens samples);
- mean and variance are the restatement's of those samples: 1, 4 and 16 samples, ray batches of
  3 and 5, a 37 x 21 batch that the slot guard splits;
- ray samples against the oracle's render of the same rays one per pixel;
- the accumulator: camera passes under three seeds, ray passes of unequal size, 777 pixels (the
  padded noise tree), passes that render twice inside (slot guard, general-instance re-render)
  fold once, the error codes;
- the tone map on a rendered frame and on a synthetic ramp, its argument errors;
- a {0, 0} device set: GI_ERR_UNSUPPORTED from the renders and the accumulator, tone map works.
"""
import ctypes as C

import numpy as np
import pytest

import feature_cases as fc
import gi_amd
import radiance_ref as rr
import ray_cases
from camera_cases import CORNELL_FLAGS
from gpu_util import compare_float_ulp, scene

pytestmark = pytest.mark.gpu

W, H = 24, 16
CORNELL_ARGS = [scene("cornell.scn"), "/tmp/x.png"] + CORNELL_FLAGS
TEAPOT_ARGS = fc.camera_args("teapot_dof") + ["-global", "5000", "-caustic", "5000", "-it", "4",
                                              "-seed", "3"]
COUNTERS = ("screen_rays", "shadow_rays", "monte_carlo_rays", "transmissive_samples",
            "specular_samples", "indirect_samples", "caustic_samples", "knn_queries",
            "knn_photons")


def load(r, args):
    """ParseArgs -> ReadScene -> MapPhotons; returns (params, aa, w, h)."""
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(args)
    r.set_params(p)
    r.ReadScene(sc, real)
    r.MapPhotons()
    return p, aa, w, h


def same_bits(dev, ref, what=""):
    dev, ref = np.ascontiguousarray(dev), np.ascontiguousarray(ref)
    assert dev.dtype == ref.dtype and dev.shape == ref.shape, (dev.dtype, ref.dtype, dev.shape, ref.shape)
    u = {4: np.uint32, 8: np.uint64, 1: np.uint8}[dev.dtype.itemsize]
    nd = int((dev.view(u) != ref.view(u)).sum())
    print(f"{what}: {nd} of {dev.size} values differ")
    assert nd == 0, (what, np.argwhere(dev.view(u) != ref.view(u))[:8].tolist())


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@pytest.fixture(scope="module")
def cornell(renderer):
    """gi_render_image and gi_render_radiance (with samples) of cornell.scn, CORNELL_FLAGS, and
    the passes under seeds 6 and 7 from the same maps. Shared: do not modify."""
    p, aa, w, h = load(renderer, CORNELL_ARGS)
    assert (aa, w, h) == (1, W, H)
    rgb, rgbf, st = renderer.RenderImage(aa, w, h, want_float=True)
    mean, var, smp, st2 = renderer.render_radiance(aa, w, h, want_samples=True)
    passes = {5: smp}
    for seed in (6, 7):   # gi_set_params keeps the maps built under seed 5
        p.seed = seed
        renderer.set_params(p)
        passes[seed] = renderer.render_radiance(aa, w, h, want_samples=True)[2]
    p.seed = 5
    renderer.set_params(p)
    frozen(rgb, rgbf, mean, var, *passes.values())
    return dict(rgb=rgb, rgbf=rgbf, st=st, mean=mean, var=var, smp=smp, st2=st2, passes=passes)


# ---- 1. the samples are the render's own -----------------------------------------------------
def test_cornell_samples_clamped_and_filtered_are_the_rendered_frame(cornell):
    smp, bw = cornell["smp"], rr.box_weight(aa=1)
    assert smp.shape == (H, W, 4, 3) and np.isfinite(smp).all()
    f, q = rr.clamped_frame(smp, bw)
    same_bits(cornell["rgbf"], f, "rgbf")
    same_bits(cornell["rgb"], q, "rgb8")
    for k in COUNTERS:
        assert cornell["st"][k] == cornell["st2"][k], k
    # fixture condition: most samples clamp, and some pixels only in part
    over = smp >= 1.0
    part = over.any(axis=2) & ~over.all(axis=2)
    print(f"{over.mean():.3f} of the sample values are >= 1, {part.mean():.3f} of the pixel "
          "channels are partly clamped")
    assert over.mean() >= 0.5
    assert part.any()
    # ... so the unclamped mean is not the clamped frame
    assert (cornell["mean"] != cornell["rgbf"]).any()
    assert cornell["mean"].max() > 1.0


def test_depth_of_field_samples_are_the_lens_means(renderer):
    _p, aa, w, h = load(renderer, TEAPOT_ARGS)
    assert (aa, w, h) == (0, 20, 20) and renderer.params.dof_test == 2
    rgb, rgbf, st = renderer.RenderImage(aa, w, h, want_float=True)
    mean, var, smp, st2 = renderer.render_radiance(aa, w, h, want_samples=True)
    assert smp.shape == (20, 20, 1, 3)
    f, q = rr.clamped_frame(smp, rr.box_weight(aa=0))
    same_bits(rgbf, f, "rgbf")
    same_bits(rgb, q, "rgb8")
    assert smp.any()
    for k in COUNTERS:
        assert st[k] == st2[k], k
    same_bits(mean, smp[:, :, 0].astype(np.float32), "mean")
    assert not var.any()


# ---- 2. mean and variance --------------------------------------------------------------------
@pytest.mark.parametrize("aa", [0, 1, 2])
def test_camera_mean_and_variance_match_restatement(renderer, cornell, aa):
    load(renderer, CORNELL_ARGS)
    if aa == 1:
        mean, var, smp = cornell["mean"], cornell["var"], cornell["smp"]
    else:
        mean, var, smp, _st = renderer.render_radiance(aa, W, H, want_samples=True)
    assert smp.shape == (H, W, 4 ** aa, 3)
    rm, rv = rr.mean_variance(smp, rr.box_weight(aa=aa))
    same_bits(mean, rm, "mean")
    same_bits(var, rv, "variance")
    assert (var == 0).all() if aa == 0 else (var > 0).any()
    # each output alone
    only_var = np.zeros((H, W, 3), dtype=np.float32)
    rc = gi_amd.lib().gi_render_radiance(renderer._ctx, aa, W, H, None, only_var.ctypes.data,
                                         None, None)
    assert rc == gi_amd.GI_OK
    same_bits(only_var, rv, "variance alone")


@pytest.fixture(scope="module")
def ray_frames(renderer):
    """spp -> (mean, variance, samples) of the stilllife light-field batch at spp 3 and 5."""
    out = {}
    load(renderer, ray_cases.scene_args("stilllife"))
    for spp in (3, 5):
        rays, ids = ray_cases.batch("stilllife", "lightfield", spp)
        mean, var, smp, st = renderer.render_rays_radiance(W, H, spp, rays, ids, want_samples=True)
        rgb, rgbf, st0 = renderer.render_rays(W, H, spp, rays, ids, want_float=True)
        f, q = rr.clamped_frame(smp, rr.box_weight(spp=spp))
        same_bits(rgbf, f, f"spp {spp} rgbf")
        same_bits(rgb, q, f"spp {spp} rgb8")
        for k in COUNTERS:
            assert st[k] == st0[k], k
        out[spp] = frozen(mean, var, smp)
    return out


@pytest.mark.parametrize("spp", [3, 5])
def test_ray_mean_and_variance_match_restatement(ray_frames, spp):
    mean, var, smp = ray_frames[spp]
    assert smp.shape == (H, W, spp, 3)
    rm, rv = rr.mean_variance(smp, rr.box_weight(spp=spp))
    same_bits(mean, rm, "mean")
    same_bits(var, rv, "variance")
    assert (var > 0).any()


@pytest.fixture(scope="module")
def tiled():
    """A context under GI_SLOT_LIMIT=9000 with the 37 x 21 batch loaded (the slot guard re-runs
    its one batch smaller until it is split), and its radiance frame."""
    import os
    name, sensor, spp, w, h = ray_cases.TILED_BATCH
    rays, ids = ray_cases.batch(name, sensor, spp, w, h)
    p, sc, _o, _w, _h, _aa, real = gi_amd.ParseArgs(ray_cases.scene_args(name, w, h))
    old = os.environ.get("GI_SLOT_LIMIT")
    os.environ["GI_SLOT_LIMIT"] = "9000"
    try:
        r = gi_amd.Renderer(0, p)
    finally:
        if old is None:
            del os.environ["GI_SLOT_LIMIT"]
        else:
            os.environ["GI_SLOT_LIMIT"] = old
    r.ReadScene(sc, real)
    r.MapPhotons()
    mean, var, smp, st = r.render_rays_radiance(w, h, spp, rays, ids, want_samples=True)
    yield dict(r=r, w=w, h=h, spp=spp, rays=rays, ids=ids, mean=mean, var=var, smp=smp, st=st)
    r.close()


def test_split_batches_write_every_pixel_once(renderer, tiled):
    w, h, spp = tiled["w"], tiled["h"], tiled["spp"]
    rm, rv = rr.mean_variance(tiled["smp"], rr.box_weight(spp=spp))
    same_bits(tiled["mean"], rm, "mean")
    same_bits(tiled["var"], rv, "variance")
    # the same frame from one batch (the shared context has no slot limit)
    load(renderer, ray_cases.scene_args("stilllife", w, h))
    mean, var, smp, st = renderer.render_rays_radiance(w, h, spp, tiled["rays"], tiled["ids"],
                                                       want_samples=True)
    # (another batch cut sums a sample's paths in another order: fp64 within the suite's 1e-10,
    # float32 within one ulp, as gpu_util.compare_float_ulp states for the oracle's order)
    compare_float_ulp(tiled["smp"].astype(np.float32), smp.astype(np.float32))
    assert tiled["st"]["knn_kernel_launches"] > st["knn_kernel_launches"]


# ---- 3. against the oracle -------------------------------------------------------------------
@pytest.mark.parametrize("name,sensor,spp", rr.ORACLE_BATCHES)
def test_ray_samples_match_the_oracle(renderer, name, sensor, spp):
    rays, ids = ray_cases.batch(name, sensor, spp)
    ref = rr.oracle_samples(name, sensor, spp)
    load(renderer, ray_cases.scene_args(name))
    _m, _v, smp, _st = renderer.render_rays_radiance(W, H, spp, rays, ids, want_samples=True)
    inside = (ref > 0.0) & (ref < 1.0)
    print(f"{inside.mean():.3f} of the oracle's values inside (0, 1), {(ref == 1).mean():.3f} "
          f"at 1, {(ref == 0).mean():.3f} at 0")
    assert inside.mean() >= 0.6
    compare_float_ulp(smp.astype(np.float32)[inside], ref[inside])
    assert (smp[ref == 1.0] >= 1.0 - 2.0 ** -24).all()
    assert (smp[ref == 0.0] <= 2.0 ** -24).all()


# ---- 4. accumulator --------------------------------------------------------------------------
def check_accum(r, ref, what):
    mean, var, n, noise = r.accum_get()
    rmean, rvar, rn, rnoise = ref.get()
    print(f"{what}: N {n}, noise {noise!r} (restatement {rnoise!r})")
    assert n == rn
    same_bits(mean, rmean, what + " mean")
    same_bits(var, rvar, what + " variance")
    assert noise == rnoise
    return noise


def test_three_camera_passes_merge_like_the_restatement(renderer, cornell):
    p, aa, w, h = load(renderer, CORNELL_ARGS)
    ref = rr.Accum((H, W))
    renderer.accum_reset(W, H)
    mean0, var0, n0, noise0 = renderer.accum_get()
    assert n0 == 0 and noise0 == 0.0 and not mean0.any() and not var0.any()
    noises = []
    for seed in (5, 6, 7):
        p.seed = seed
        renderer.set_params(p)
        st = renderer.accum_add_image(aa)
        assert st["screen_rays"] == cornell["st"]["screen_rays"]   # the pass's own counters
        ref.add_samples(cornell["passes"][seed], rr.box_weight(aa=1))
        noises.append(check_accum(renderer, ref, f"after seed {seed}"))
        if seed == 5:   # one pass is gi_render_radiance's frame
            mean, var, n, _noise = renderer.accum_get()
            same_bits(mean, cornell["mean"], "first pass mean")
            same_bits(var, cornell["var"], "first pass variance")
            assert n == 4
    assert renderer.accum_get()[2] == 12
    print("noise after 1, 2, 3 passes:", noises)
    # a reset empties it
    renderer.accum_reset(W, H)
    assert renderer.accum_get()[2] == 0


def test_ray_passes_of_unequal_size_merge_like_the_restatement(renderer, ray_frames):
    load(renderer, ray_cases.scene_args("stilllife"))
    ref = rr.Accum((H, W))
    renderer.accum_reset(W, H)
    for spp in (3, 5):
        rays, ids = ray_cases.batch("stilllife", "lightfield", spp)
        renderer.accum_add_rays(spp, rays, ids)
        ref.add_samples(ray_frames[spp][2], rr.box_weight(spp=spp))
        check_accum(renderer, ref, f"after spp {spp}")
    assert renderer.accum_get()[2] == 8


def test_777_pixels_and_split_batches_fold_once(tiled):
    """37 x 21 = 777 pixels = three blocks of 256 and nine: the padded tree. Under the slot
    limit a pass renders its batch several times; it is folded once."""
    r, w, h, spp = tiled["r"], tiled["w"], tiled["h"], tiled["spp"]
    ref = rr.Accum((h, w))
    r.accum_reset(w, h)
    r.accum_add_rays(spp, tiled["rays"], tiled["ids"])
    ref.add_samples(tiled["smp"], rr.box_weight(spp=spp))
    assert r.accum_get()[2] == spp
    check_accum(r, ref, "one split pass")
    # a second pass under other stream ids
    ids2 = tiled["ids"] + np.uint64(977)
    _m, _v, smp2, _st = r.render_rays_radiance(w, h, spp, tiled["rays"], ids2, want_samples=True)
    assert (smp2 != tiled["smp"]).any()
    r.accum_add_rays(spp, tiled["rays"], ids2)
    ref.add_samples(smp2, rr.box_weight(spp=spp))
    noise = check_accum(r, ref, "two split passes")
    assert r.accum_get()[2] == 2 * spp and noise > 0.0


def test_general_instance_rerender_folds_once(monkeypatch):
    """GI_KNN_GENERAL=-1: the first render of a context misses the general estimate form and
    render_common renders again (test_gpu_knn_variants.py). The pass is folded once and equals
    a normal context's."""
    args = [scene("stilllife.scn"), "/tmp/x.png", "-resolution", str(W), str(H), "-aa", "1",
            "-global", "20000", "-caustic", "40000", "-it", "8", "-tt", "4", "-st", "4", "-seed", "2"]
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(args)
    got = []
    for env in (None, "-1"):
        if env is not None:
            monkeypatch.setenv("GI_KNN_GENERAL", env)
        r = gi_amd.Renderer(0, p)
        try:
            r.ReadScene(sc, real)
            r.MapPhotons()
            r.accum_reset(w, h)
            r.accum_add_image(aa)      # the forced context re-renders inside this call
            got.append(r.accum_get())
        finally:
            r.close()
    assert got[0][2] == got[1][2] == 4
    assert np.isfinite(got[1][0]).all()
    same_bits(got[1][0], got[0][0], "mean")
    same_bits(got[1][1], got[0][1], "variance")
    assert got[1][3] == got[0][3]


def test_accumulator_error_codes(renderer):
    L = gi_amd.lib()
    rays, ids = ray_cases.batch("stilllife", "lightfield", 3)
    r = gi_amd.Renderer(0)
    try:
        n, noise = C.c_int64(-1), C.c_double(-1.0)
        assert L.gi_accum_get(r._ctx, None, None, C.byref(n), C.byref(noise)) == gi_amd.GI_ERR_STATE
        assert L.gi_accum_add_image(r._ctx, 0, None) == gi_amd.GI_ERR_STATE
        assert L.gi_accum_add_rays(r._ctx, 3, rays.ctypes.data, None, None) == gi_amd.GI_ERR_STATE
        for w, h in ((0, 4), (4, -1), (65536, 32768)):
            assert L.gi_accum_reset(r._ctx, w, h) == gi_amd.GI_ERR_ARG
        assert L.gi_accum_add_image(r._ctx, 0, None) == gi_amd.GI_ERR_STATE   # still no reset
        assert L.gi_accum_reset(r._ctx, W, H) == gi_amd.GI_OK
        assert L.gi_accum_add_image(r._ctx, 0, None) == gi_amd.GI_ERR_STATE   # no scene
        assert L.gi_accum_get(r._ctx, None, None, C.byref(n), None) == gi_amd.GI_OK and n.value == 0
    finally:
        r.close()
    load(renderer, ray_cases.scene_args("stilllife"))
    ctx = renderer._ctx
    renderer.accum_reset(W, H)
    assert L.gi_accum_add_rays(ctx, 0, rays.ctypes.data, None, None) == gi_amd.GI_ERR_ARG
    assert L.gi_accum_add_rays(ctx, 3, None, None, None) == gi_amd.GI_ERR_ARG
    assert L.gi_accum_add_image(ctx, -1, None) == gi_amd.GI_ERR_ARG
    assert L.gi_accum_add_image(ctx, 16, None) == gi_amd.GI_ERR_ARG
    with pytest.raises(ValueError):    # a ray pass has the reset's width x height
        renderer.accum_add_rays(5, rays, ids)
    assert renderer.accum_get()[2] == 0   # nothing was folded
    m = np.zeros((H, W, 3), dtype=np.float32)
    bad = [L.gi_render_radiance(ctx, 0, W, H, None, None, None, None),
           L.gi_render_radiance(ctx, -1, W, H, m.ctypes.data, None, None, None),
           L.gi_render_radiance(ctx, 0, 0, H, m.ctypes.data, None, None, None),
           L.gi_render_rays_radiance(ctx, W, H, 3, rays.ctypes.data, None, None, None, None, None),
           L.gi_render_rays_radiance(ctx, W, H, 0, rays.ctypes.data, None, m.ctypes.data, None,
                                     None, None),
           L.gi_render_rays_radiance(ctx, W, H, 3, None, None, m.ctypes.data, None, None, None),
           L.gi_render_rays_radiance(ctx, 65536, 32768, 3, rays.ctypes.data, None, m.ctypes.data,
                                     None, None, None)]
    assert bad == [gi_amd.GI_ERR_ARG] * len(bad)


# ---- 5. tone map -----------------------------------------------------------------------------
SETTINGS = [(1.0, 0.0), (1.0, 4.0), (0.25, 0.0), (0.25, 4.0), (3.0, 0.5)]


def ramp():
    """131 x 11 values from 0 to 50 with zeros: several blocks, both ends of the curve."""
    rng = np.random.default_rng(5)
    f = np.linspace(0.0, 50.0, 131 * 11 * 3, dtype=np.float32)
    rng.shuffle(f)
    f[rng.random(f.size) < 0.1] = 0.0
    return f.reshape(11, 131, 3)


@pytest.mark.parametrize("exposure,white", SETTINGS)
def test_tonemap_matches_restatement(renderer, cornell, exposure, white):
    for name, frame in (("cornell mean", cornell["mean"]), ("ramp", ramp())):
        rgb, out = renderer.tonemap(frame, exposure, white, want_float=True)
        ref = rr.tonemap(frame, exposure, white)
        same_bits(out, ref, name)
        np.testing.assert_array_equal(rgb, rr.quantize(ref))
        assert out.min() >= 0.0 and out.max() <= 1.0
        if name == "ramp":
            assert (out == 1.0).any() and (out < 1.0).any()


def test_tonemap_of_a_frame_below_one_is_the_identity(renderer, cornell):
    f = cornell["rgbf"] * np.float32(0.999)
    rgb, out = renderer.tonemap(f, want_float=True)
    same_bits(out, f, "identity")
    np.testing.assert_array_equal(rgb, rr.quantize(f))


def test_tonemap_argument_errors(renderer):
    L, ctx = gi_amd.lib(), renderer._ctx
    f = ramp()
    out = np.zeros_like(f)
    q = np.zeros(f.shape, dtype=np.uint8)

    def call(w=131, h=11, src=f.ctypes.data, exposure=1.0, white=0.0, o=out.ctypes.data, o8=None):
        return L.gi_tonemap(ctx, w, h, src, exposure, white, o, o8)

    assert call() == gi_amd.GI_OK
    assert call(o=None, o8=q.ctypes.data) == gi_amd.GI_OK      # only the 8-bit image
    np.testing.assert_array_equal(q, rr.quantize(rr.tonemap(f)))
    bad = [call(o=None), call(src=None), call(w=0), call(h=-2), call(w=65536, h=32768)]
    bad += [call(exposure=v) for v in (0.0, -1.0, float("nan"), float("inf"))]
    bad += [call(white=v) for v in (-0.5, float("nan"), float("inf"))]
    assert bad == [gi_amd.GI_ERR_ARG] * len(bad)
    with pytest.raises(ValueError):
        renderer.tonemap(f[..., :2])


# ---- 6. device set ---------------------------------------------------------------------------
def test_device_set_is_unsupported_but_tonemaps(cornell):
    L = gi_amd.lib()
    rays, ids = ray_cases.batch("stilllife", "lightfield", 3)
    m = np.zeros((H, W, 3), dtype=np.float32)
    r = gi_amd.Renderer(devices=[0, 0])
    try:
        load(r, CORNELL_ARGS)
        n = C.c_int64(0)
        got = [L.gi_render_radiance(r._ctx, 1, W, H, m.ctypes.data, None, None, None),
               L.gi_render_rays_radiance(r._ctx, W, H, 3, rays.ctypes.data, ids.ctypes.data,
                                         m.ctypes.data, None, None, None),
               L.gi_accum_reset(r._ctx, W, H),
               L.gi_accum_add_image(r._ctx, 1, None),
               L.gi_accum_add_rays(r._ctx, 3, rays.ctypes.data, ids.ctypes.data, None),
               L.gi_accum_get(r._ctx, m.ctypes.data, None, C.byref(n), None)]
        assert got == [gi_amd.GI_ERR_UNSUPPORTED] * len(got)
        assert not m.any()
        # the clamped render still works on it, and so does the tone map
        rgb, rgbf, _st = r.RenderImage(1, W, H, want_float=True)
        same_bits(rgbf, cornell["rgbf"], "device set rgbf")
        _q, out = r.tonemap(cornell["mean"], 0.25, 4.0, want_float=True)
        same_bits(out, rr.tonemap(cornell["mean"], 0.25, 4.0), "device set tone map")
    finally:
        r.close()
