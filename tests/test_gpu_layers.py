"""Light-path layers (gi.h "light-path layers") on the device.

1. plane TOTAL of gi_render_layers / gi_render_rays_layers is gi_render_radiance's /
   gi_render_rays_radiance's output and counters, bit for bit;
2. under flags that leave light to one layer only, the total equals that layer bit for bit
   wherever the others are exactly 0, on at least the stated number of non-zero pixels;
3. the layers of a sample add up to the total within 1e-12 relative (layers_ref.SUM_BOUND), on
   the cornell frame and on a depth-of-field frame;
4. every plane's mean and variance are radiance_ref's of its samples (1, 4, 16 samples, ray
   batches of 3 and 5), and a frame the slot guard splits is written once;
5. layered passes: the total's accumulator is gi_accum_add_image's, every layer context's is the
   fold of that layer's samples, a NULL entry leaves nothing behind; ray passes of unequal size;
   gi_accum_denoise serves a layer context like any accumulator;
6. the error codes, and that a refused call changes no accumulator.
"""
import ctypes as C
import os

import numpy as np
import pytest

import gi_amd
import layers_ref as lr
import radiance_ref as rr
import ray_cases
import vdenoise_ref as vr
from camera_cases import CORNELL_FLAGS
from gpu_util import scene
from test_gpu_radiance import COUNTERS, TEAPOT_ARGS, frozen, same_bits

pytestmark = pytest.mark.gpu

W, H = 24, 16
CORNELL_ARGS = [scene("cornell.scn"), "/tmp/x.png"] + CORNELL_FLAGS
SEEDS = (5, 6, 7)


def load(r, args):
    """ParseArgs -> ReadScene -> MapPhotons where a flag asks for a map, as the CLI does."""
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(args)
    r.set_params(p)
    r.ReadScene(sc, real)
    if p.indirect_illum or p.caustic_illum or p.direct_photon_illum:
        r.MapPhotons()
    return p, aa, w, h


@pytest.fixture(scope="module")
def cornell(renderer):
    """cornell.scn, CORNELL_FLAGS: gi_render_radiance's frame and gi_render_layers' under seed 5,
    and the layer samples under seeds 6 and 7 from the same maps. Shared: do not modify."""
    p, aa, w, h = load(renderer, CORNELL_ARGS)
    assert (aa, w, h) == (1, W, H)
    rad = renderer.render_radiance(aa, w, h, want_samples=True)
    lay = renderer.render_layers(aa, w, h, want_samples=True)
    passes = {5: lay[2]}
    for seed in SEEDS[1:]:
        p.seed = seed
        renderer.set_params(p)
        passes[seed] = renderer.render_layers(aa, w, h, want_samples=True)[2]
    p.seed = 5
    renderer.set_params(p)
    frozen(*rad[:3], *lay[:3], *passes.values())
    return dict(rad=rad, lay=lay, passes=passes)


@pytest.fixture(scope="module")
def ray_frames(renderer):
    """spp -> (rays, ids, gi_render_rays_radiance's output, gi_render_rays_layers') of the
    stilllife light-field batch."""
    out = {}
    load(renderer, ray_cases.scene_args("stilllife"))
    for spp in (3, 5):
        rays, ids = ray_cases.batch("stilllife", "lightfield", spp)
        rad = renderer.render_rays_radiance(W, H, spp, rays, ids, want_samples=True)
        lay = renderer.render_rays_layers(W, H, spp, rays, ids, want_samples=True)
        frozen(*rad[:3], *lay[:3])
        out[spp] = (rays, ids, rad, lay)
    return out


def check_total_plane(rad, lay, what):
    for k, name in enumerate(("mean", "variance", "samples")):
        assert lay[k].shape == (lr.COUNT + 1,) + rad[k].shape
        same_bits(lay[k][lr.TOTAL], rad[k], f"{what} total {name}")
    for k in COUNTERS:
        assert lay[3][k] == rad[3][k], k
    assert rad[2].any()


def check_sum(samples, what):
    ratio, zeros = lr.sum_ratio(samples)
    print(f"{what}: largest |sum of layers - total| / total = {ratio:.3e}")
    assert zeros
    assert ratio <= lr.SUM_BOUND


# ---- 1. the total plane ------------------------------------------------------------------------
def test_total_plane_is_the_radiance_frame(cornell):
    check_total_plane(cornell["rad"], cornell["lay"], "cornell")


def test_total_plane_of_a_ray_batch_is_the_radiance_frame(ray_frames):
    _rays, _ids, rad, lay = ray_frames[3]
    check_total_plane(rad, lay, "stilllife spp 3")


# ---- 2. a layer alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("layer", range(lr.COUNT), ids=lr.NAMES)
def test_a_layer_alone_is_the_total(renderer, layer):
    flags, floor = lr.ISOLATING[layer]
    _p, aa, w, h = load(renderer, CORNELL_ARGS + flags)
    _mean, _var, smp, _st = renderer.render_layers(aa, w, h, want_samples=True)
    assert (smp >= 0.0).all()            # fixture condition: every term is non-negative
    q = lr.alone(smp, layer)
    u = np.uint64
    assert (smp[lr.TOTAL][q].view(u) == smp[layer][q].view(u)).all()
    pixels = int(lr.alone_pixels(smp, layer).sum())
    print(f"{lr.NAMES[layer]}: alone in {q.mean():.3f} of the samples, non-zero there in {pixels} "
          f"of {w * h} pixels")
    assert pixels >= floor
    if layer == lr.SURFACE:              # the other four are 0 everywhere
        assert q.all()


# ---- 3. the layers add up -----------------------------------------------------------------------
def test_layers_add_up_to_the_total(cornell):
    smp = cornell["lay"][2]
    check_sum(smp, "cornell")
    lit = [lr.NAMES[l] for l in range(lr.COUNT) if smp[l].any()]
    print("layers that are not zero:", lit)
    assert len(lit) >= 3
    assert (smp >= 0.0).all()


def test_depth_of_field_layers_add_up(renderer):
    _p, aa, w, h = load(renderer, TEAPOT_ARGS)
    assert (aa, w, h) == (0, 20, 20) and renderer.params.dof_test == 2
    rad = renderer.render_radiance(aa, w, h, want_samples=True)
    lay = renderer.render_layers(aa, w, h, want_samples=True)
    check_total_plane(rad, lay, "teapot")
    check_sum(lay[2], "teapot")
    assert sum(bool(lay[2][l].any()) for l in range(lr.COUNT)) >= 2


# ---- 4. means and variances ---------------------------------------------------------------------
def check_planes(lay, bw, what):
    mean, var, smp = lay[:3]
    for l in range(lr.COUNT + 1):
        rm, rv = rr.mean_variance(smp[l], bw)
        name = (lr.NAMES + ("total",))[l]
        same_bits(mean[l], rm, f"{what} {name} mean")
        same_bits(var[l], rv, f"{what} {name} variance")


@pytest.mark.parametrize("aa", [0, 1, 2])
def test_camera_planes_match_restatement(renderer, cornell, aa):
    load(renderer, CORNELL_ARGS)
    lay = cornell["lay"] if aa == 1 else renderer.render_layers(aa, W, H, want_samples=True)
    assert lay[2].shape == (lr.COUNT + 1, H, W, 4 ** aa, 3)
    check_planes(lay, rr.box_weight(aa=aa), f"aa {aa}")
    assert not lay[1].any() if aa == 0 else all(lay[1][l].any() for l in (lr.SURFACE, lr.INDIRECT))
    # each output alone
    only_var = np.zeros_like(lay[1])
    rc = gi_amd.lib().gi_render_layers(renderer._ctx, aa, W, H, None, only_var.ctypes.data, None, None)
    assert rc == gi_amd.GI_OK
    same_bits(only_var, lay[1], "variance alone")


def test_kernel_timing_seam(renderer, cornell):
    """gi_layers_timing: the kernel's summed event time of the layered renders while it is on,
    and the planes are the same with it."""
    load(renderer, CORNELL_ARGS)
    assert renderer.layers_timing(True) == 0.0
    lay = renderer.render_layers(1, W, H, want_samples=True)
    renderer.render_radiance(1, W, H)            # not a layered render: adds nothing
    ms = renderer.layers_timing(False)
    print(f"reduce_prim_layers_kernel: {ms:.4f} ms")
    assert 0.0 < ms < 1000.0
    same_bits(lay[2], cornell["lay"][2], "samples under timing")
    renderer.render_layers(1, W, H)
    assert renderer.layers_timing(False) == ms   # off: nothing added


@pytest.mark.parametrize("spp", [3, 5])
def test_ray_planes_match_restatement(ray_frames, spp):
    _rays, _ids, _rad, lay = ray_frames[spp]
    assert lay[2].shape == (lr.COUNT + 1, H, W, spp, 3)
    check_planes(lay, rr.box_weight(spp=spp), f"spp {spp}")
    check_sum(lay[2], f"spp {spp}")


def test_split_batches_write_every_layer_pixel_once():
    """The 37 x 21 batch under GI_SLOT_LIMIT=9000 (the slot guard re-runs its one batch smaller
    until it is split): the planes are those of one write per pixel."""
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
    try:
        r.ReadScene(sc, real)
        r.MapPhotons()
        rad = r.render_rays_radiance(w, h, spp, rays, ids, want_samples=True)
        lay = r.render_rays_layers(w, h, spp, rays, ids, want_samples=True)
    finally:
        r.close()
    check_total_plane(rad, lay, "split")
    check_sum(lay[2], "split")
    check_planes(lay, rr.box_weight(spp=spp), "split")


# ---- 5. layered passes --------------------------------------------------------------------------
@pytest.fixture()
def layer_ctxs():
    """Five scene-less contexts with empty W x H accumulators."""
    rs = [gi_amd.Renderer(0) for _ in range(lr.COUNT)]
    for r in rs:
        r.accum_reset(W, H)
    yield rs
    for r in rs:
        r.close()


def check_state(r, ref, what):
    state, counts = r.accum_export()
    same_bits(state, ref[0], what + " state")
    same_bits(counts, ref[1], what + " counts")


def test_three_layered_camera_passes(renderer, cornell, layer_ctxs):
    p, aa, w, h = load(renderer, CORNELL_ARGS)
    # a second context, given plain passes under the same seeds from the same maps
    plain = gi_amd.Renderer(0)
    try:
        load(plain, CORNELL_ARGS)
        plain.accum_reset(W, H)
        renderer.accum_reset(W, H)
        for seed in SEEDS:
            p.seed = seed
            renderer.set_params(p)
            plain.set_params(p)
            st = renderer.accum_add_image_layers(aa, layer_ctxs)
            st0 = plain.accum_add_image(aa)
            for k in COUNTERS:
                assert st[k] == st0[k], k
        p.seed = 5
        renderer.set_params(p)
        check_state(renderer, plain.accum_export(), "total")
    finally:
        plain.close()
    bw = rr.box_weight(aa=1)
    for l, r in enumerate(layer_ctxs):
        check_state(r, lr.accum_state([(cornell["passes"][s][l], bw) for s in SEEDS]), lr.NAMES[l])
        assert r.accum_get()[2] == 12
    check_state(renderer, lr.accum_state([(cornell["passes"][s][lr.TOTAL], bw) for s in SEEDS]),
                "total against the restatement")
    # a layer's context is an ordinary accumulator: the variance-guided filter of it
    r = layer_ctxs[lr.SURFACE]
    feat = renderer.camera_features(aa, W, H)
    mean, var, _n, _noise = r.accum_get()
    out, vlum, _ms = r.accum_denoise(feat, levels=3)
    ref = vr.denoise(mean, var, feat, levels=3)
    same_bits(out, ref[0], "filtered surface layer")
    same_bits(vlum, ref[1], "its luminance variance")
    assert (out != mean).any()


def test_two_layered_ray_passes_and_a_null_entry(renderer, ray_frames, layer_ctxs):
    load(renderer, ray_cases.scene_args("stilllife"))
    renderer.accum_reset(W, H)
    listed = list(layer_ctxs)
    listed[lr.INDIRECT] = None
    for spp in (3, 5):
        rays, ids, _rad, _lay = ray_frames[spp]
        renderer.accum_add_rays_layers(spp, rays, listed, ids)
    passes = [(ray_frames[spp][3][2], rr.box_weight(spp=spp)) for spp in (3, 5)]
    check_state(renderer, lr.accum_state([(s[lr.TOTAL], bw) for s, bw in passes]), "total")
    plain = gi_amd.Renderer(0)       # a second context, given the same passes without layers
    try:
        load(plain, ray_cases.scene_args("stilllife"))
        plain.accum_reset(W, H)
        for spp in (3, 5):
            plain.accum_add_rays(spp, ray_frames[spp][0], ray_frames[spp][1])
        check_state(renderer, plain.accum_export(), "total against plain passes")
    finally:
        plain.close()
    for l, r in enumerate(layer_ctxs):
        if l == lr.INDIRECT:      # dropped: as the reset left it
            state, counts = r.accum_export()
            assert not state.any() and not counts.any() and r.accum_get()[2] == 0
        else:
            check_state(r, lr.accum_state([(s[l], bw) for s, bw in passes]), lr.NAMES[l])
    assert any(s[lr.INDIRECT].any() for s, _bw in passes)   # there was something to drop


# ---- 6. errors ----------------------------------------------------------------------------------
def ctx_array(rs):
    return (C.c_void_p * lr.COUNT)(*[None if r is None else r._ctx for r in rs])


def test_layer_error_codes_change_nothing(renderer, layer_ctxs):
    L = gi_amd.lib()
    _p, aa, w, h = load(renderer, CORNELL_ARGS)
    rays, ids = ray_cases.batch("stilllife", "lightfield", 3)
    ctx = renderer._ctx
    m = np.zeros((lr.COUNT + 1, H, W, 3), dtype=np.float32)
    # outputs
    assert L.gi_render_layers(ctx, aa, W, H, None, None, None, None) == gi_amd.GI_ERR_ARG
    assert L.gi_render_rays_layers(ctx, W, H, 3, rays.ctypes.data, None, None, None, None,
                                   None) == gi_amd.GI_ERR_ARG
    assert L.gi_render_layers(ctx, -1, W, H, m.ctypes.data, None, None, None) == gi_amd.GI_ERR_ARG
    assert L.gi_render_rays_layers(ctx, W, H, 0, rays.ctypes.data, None, m.ctypes.data, None, None,
                                   None) == gi_amd.GI_ERR_ARG
    # no reset on ctx, then on a layer context
    fresh = gi_amd.Renderer(0)
    other = gi_amd.Renderer(0)
    try:
        load(fresh, CORNELL_ARGS)
        arr = ctx_array(layer_ctxs)
        assert L.gi_accum_add_image_layers(fresh._ctx, aa, arr, None) == gi_amd.GI_ERR_STATE
        assert L.gi_accum_add_rays_layers(fresh._ctx, 3, rays.ctypes.data, None, arr,
                                          None) == gi_amd.GI_ERR_STATE
        fresh.accum_reset(W, H)
        arr = ctx_array(layer_ctxs[:4] + [other])
        assert L.gi_accum_add_image_layers(fresh._ctx, aa, arr, None) == gi_amd.GI_ERR_STATE
        # a layer context of another size, equal to ctx, or listed twice; a null list
        other.accum_reset(W + 1, H)
        before = [r.accum_export() for r in [fresh] + layer_ctxs]
        bad = [ctx_array(layer_ctxs[:4] + [other]), ctx_array(layer_ctxs[:4] + [fresh]),
               ctx_array(layer_ctxs[:4] + [layer_ctxs[0]]), None]
        for arr in bad:
            assert L.gi_accum_add_image_layers(fresh._ctx, aa, arr, None) == gi_amd.GI_ERR_ARG
            assert L.gi_accum_add_rays_layers(fresh._ctx, 3, rays.ctypes.data, None, arr,
                                              None) == gi_amd.GI_ERR_ARG
        # a good list and a bad pass
        arr = ctx_array(layer_ctxs)
        assert L.gi_accum_add_image_layers(fresh._ctx, 16, arr, None) == gi_amd.GI_ERR_ARG
        assert L.gi_accum_add_rays_layers(fresh._ctx, 0, rays.ctypes.data, None, arr,
                                          None) == gi_amd.GI_ERR_ARG
        for r, (state, counts) in zip([fresh] + layer_ctxs, before):
            check_state(r, (state, counts), "after the refused calls")
            assert not counts.any()
    finally:
        fresh.close()
        other.close()


def test_device_set_is_unsupported(layer_ctxs):
    L = gi_amd.lib()
    rays, ids = ray_cases.batch("stilllife", "lightfield", 3)
    m = np.zeros((lr.COUNT + 1, H, W, 3), dtype=np.float32)
    r = gi_amd.Renderer(devices=[0, 0])
    try:
        load(r, CORNELL_ARGS)
        arr = ctx_array(layer_ctxs)
        got = [L.gi_render_layers(r._ctx, 1, W, H, m.ctypes.data, None, None, None),
               L.gi_render_rays_layers(r._ctx, W, H, 3, rays.ctypes.data, ids.ctypes.data,
                                       m.ctypes.data, None, None, None),
               L.gi_accum_add_image_layers(r._ctx, 1, arr, None),
               L.gi_accum_add_rays_layers(r._ctx, 3, rays.ctypes.data, ids.ctypes.data, arr, None)]
        assert got == [gi_amd.GI_ERR_UNSUPPORTED] * len(got)
        assert not m.any()
    finally:
        r.close()
