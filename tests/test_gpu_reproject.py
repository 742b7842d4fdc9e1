"""Reprojection across views (gi.h "reprojection across views") on the device against
tests/reproject_ref.py, bit for bit: gi_get_view, gi_accum_reproject after whole-frame and masked
passes, the passes folded onto the carried history, the selection of the reset tiles and the
error codes.

Fixtures: the dimmed cornell view of camera_cases at 24 x 16 and aa 1 (view A; view B: the eye
moved by +0.15 in x), the 37 x 21 stilllife frame of test_gpu_adaptive.py at aa 1 (both coverage
classes, several materials) and a 131 x 11 frame of the dimmed cornell at aa 0 (three blocks in x,
the last one clipped, and a clipped block row). Every pass's samples come from gi_render_radiance
under the pass's seed and camera.
"""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref as ar
import camera_cases as cc
import gi_amd
import radiance_ref as rr
import ray_cases
import reproject_ref as rp

pytestmark = pytest.mark.gpu

W, H = 24, 16
SW, SH = 37, 21
LW, LH = 131, 11
BW = rr.box_weight(aa=1)
CAMERA_A = cc.camera_of(cc.CASES["cornell_dim"][1])
CAMERA_B = ((CAMERA_A[0][0] + 0.15,) + CAMERA_A[0][1:],) + CAMERA_A[1:]


def same_bits(dev, ref, what=""):
    dev, ref = np.ascontiguousarray(dev), np.ascontiguousarray(ref)
    assert dev.dtype == ref.dtype and dev.shape == ref.shape, (dev.dtype, ref.dtype, dev.shape, ref.shape)
    u = {4: np.uint32, 8: np.uint64, 1: np.uint8}[dev.dtype.itemsize]
    nd = int((dev.view(u) != ref.view(u)).sum())
    print(f"{what}: {nd} of {dev.size} values differ")
    assert nd == 0, (what, np.argwhere(dev.view(u) != ref.view(u))[:8].tolist())


def make_context(args, camera=None):
    p, sc, _o, _w, _h, _aa, real = gi_amd.ParseArgs(args)
    r = gi_amd.Renderer(0, p)
    r.ReadScene(sc, real)
    if camera is not None:
        r.set_camera(*camera)
    r.MapPhotons()
    return r, p


def seed(r, p, s):
    p.seed = s
    r.set_params(p)


def view_fixture(r, p, aa, w, h, cam_a, cam_b, seeds_a, seeds_b):
    """The samples of every pass, the planes and the pinhole frames of the two cameras."""
    d = dict(r=r, p=p, aa=aa, w=w, h=h, cam=(cam_a, cam_b), smp={}, feat=[], view=[],
             bw=rr.box_weight(aa=aa))
    for cam, seeds in ((cam_a, seeds_a), (cam_b, seeds_b)):
        r.set_camera(*cam)
        for s in seeds:
            seed(r, p, s)
            d["smp"][s] = r.render_radiance(aa, w, h, want_samples=True)[2]
            d["smp"][s].setflags(write=False)
        d["feat"].append(r.camera_features(aa, w, h))
        d["view"].append(r.get_view())
    return d


def cornell_args():
    return [cc.dimmed_cornell(), "/tmp/x.png"] + cc.CORNELL_FLAGS


@pytest.fixture(scope="module")
def cornell():
    r, p = make_context(cornell_args(), CAMERA_A)
    yield view_fixture(r, p, 1, W, H, CAMERA_A, CAMERA_B, (5, 6, 7), (8,))
    r.close()


@pytest.fixture(scope="module")
def still():
    p, sc, _o, _w, _h, _aa, real = gi_amd.ParseArgs(ray_cases.scene_args("stilllife", SW, SH))
    r = gi_amd.Renderer(0, p)
    radius = r.ReadScene(sc, real)["radius"]
    r.MapPhotons()
    eye, towards, up, xfov = r.get_camera()
    moved = ((eye[0] + 0.04 * radius, eye[1] + 0.02 * radius, eye[2]), towards, up, xfov)
    yield view_fixture(r, p, 1, SW, SH, (eye, towards, up, xfov), moved, (5, 6), (8,))
    r.close()


def passes_in_a(f, seeds, release=False):
    """Camera A, a reset and the whole-frame passes under `seeds`; the restatement's accumulator."""
    r, p = f["r"], f["p"]
    r.set_camera(*f["cam"][0])
    r.accum_reset(f["w"], f["h"])
    ref = ar.Accum((f["h"], f["w"]))
    for s in seeds:
        seed(r, p, s)
        r.accum_add_image(f["aa"])
        ref.add_samples(f["smp"][s], f["bw"])
    if release:
        r.release_scratch()
    return ref


def reproject_to_b(f, ref, **params):
    """gi_set_camera to B and gi_accum_reproject, on the device and in the restatement."""
    r = f["r"]
    r.set_camera(*f["cam"][1])
    st, ms = r.accum_reproject(f["view"][0], f["feat"][0], f["feat"][1], **params)
    out, rst, _taps = rp.reproject(ref, f["view"][0], f["feat"][0], r.get_view(), f["feat"][1], **params)
    print(f"reprojection: {st}, kernel {ms:.4f} ms")
    assert st == rst
    assert st["kept_pixels"] + st["reset_pixels"] == f["w"] * f["h"]
    return out, st


def check(r, ref, what):
    """gi_accum_get and gi_accum_get_counts against the restatement."""
    mean, var, n, noise = r.accum_get()
    counts, total = r.accum_get_counts()
    rmean, rvar, rn, rnoise = ref.get()
    print(f"{what}: smallest count {n}, total {total}, noise {noise!r} (restatement {rnoise!r})")
    np.testing.assert_array_equal(counts, ref.n)
    assert total == int(ref.n.sum()) and n == rn
    same_bits(mean, rmean, what + " mean")
    same_bits(var, rvar, what + " variance")
    assert noise == rnoise
    return mean, var, counts, noise


def then_a_pass_in_b(f, out, s=8, what=""):
    """One more whole-frame pass on the carried history: the fp64 state behind the float outputs."""
    seed(f["r"], f["p"], s)
    f["r"].accum_add_image(f["aa"])
    out.add_samples(f["smp"][s], f["bw"])
    return check(f["r"], out, what + " + a pass in B")


# ---- gi_get_view ------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(24, 16), (7, 5)])
def test_get_view_is_the_frame_of_the_camera_rays(cornell, w, h):
    r, p = cornell["r"], cornell["p"]
    r.set_camera(*CAMERA_A)
    rays, _ids = r.camera_rays(0, w, h)
    v = rp.as_view(r.get_view())
    ys, xs = np.mgrid[0:h, 0:w]
    dx = (2 * (xs - w // 2)).astype(np.float64) / float(w)      # camera_ray's dx and dy
    dy = (2 * (ys - h // 2)).astype(np.float64) / float(h)
    D = [((v.far_org[k] + v.far_right[k] * dx) + v.far_up[k] * dy) - v.eye[k] for k in range(3)]
    ln = np.sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2])
    want = np.stack([D[k] / ln for k in range(3)], axis=-1).reshape(-1, 3)
    same_bits(rays["dir"], want, f"{w} x {h} ray directions")
    same_bits(rays["org"], np.broadcast_to(v.eye, want.shape).copy(), "ray origins")
    mine = rp.view_of(CAMERA_A, p.focus_depth)
    for a, b in zip(v, mine):
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, p.focus_depth)


def test_get_view_follows_focus_depth(cornell):
    r, p = cornell["r"], cornell["p"]
    r.set_camera(*CAMERA_A)
    v1 = rp.as_view(r.get_view())
    old = p.focus_depth
    try:
        p.focus_depth = 2.5 * old
        r.set_params(p)
        v2 = rp.as_view(r.get_view())
        mine = rp.view_of(CAMERA_A, p.focus_depth)
    finally:
        p.focus_depth = old
        r.set_params(p)
    same_bits(v2.eye, v1.eye, "eye")
    for a, b, c in zip(v2[1:], mine[1:], v1[1:]):
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, 2.5 * old)
        assert (a != c).any()
    assert np.abs((v2.far_right / v1.far_right) - 2.5).max() <= 1e-12
    same_bits(np.array(list(r.get_view().far_up)), v1.far_up, "the view after focus_depth is put back")


# ---- gi_accum_reproject against the restatement -------------------------------------------------
def test_cornell_reprojection_and_a_pass_on_top_match_restatement(cornell):
    ref = passes_in_a(cornell, (5, 6, 7))
    out, st = reproject_to_b(cornell, ref)
    assert 0 < st["reset_pixels"] < W * H and st["kept_samples"] == 12 * st["kept_pixels"]
    _m, _v, counts, _n = check(cornell["r"], out, "cornell A -> B")
    assert set(np.unique(counts)) == {0, 12}
    then_a_pass_in_b(cornell, out, what="cornell")


def test_stilllife_reprojection_over_unequal_counts_matches_restatement(still):
    r, p = still["r"], still["p"]
    ref = passes_in_a(still, (5,))
    board = ar.checkerboard(SW, SH, 8)
    seed(r, p, 6)
    r.accum_add_tiles(1, 8, board)
    ref.add_samples(still["smp"][6], BW, ar.pixel_mask(board, SW, SH, 8))
    assert set(np.unique(ref.n)) == {4, 8}
    cov = still["feat"][1]["coverage"]
    assert (cov == 0).any() and (cov == 1).any()       # both coverage classes
    # the albedo stop acts: with it wide open more pixels keep history
    kept_default = rp.reproject(ref, still["view"][0], still["feat"][0], still["view"][1], still["feat"][1])[1]
    kept_open = rp.reproject(ref, still["view"][0], still["feat"][0], still["view"][1], still["feat"][1],
                             albedo_tol=10.0)[1]
    print("kept pixels, default / albedo stop open:", kept_default["kept_pixels"], kept_open["kept_pixels"])
    assert kept_open["kept_pixels"] > kept_default["kept_pixels"]
    out, st = reproject_to_b(still, ref)
    assert 0 < st["reset_pixels"] < SW * SH
    _m, _v, counts, _n = check(r, out, "stilllife A -> B")
    assert {4, 8} <= set(np.unique(counts))
    then_a_pass_in_b(still, out, what="stilllife")


def test_wide_frame_of_several_blocks_matches_restatement():
    r, p = make_context(cornell_args(), CAMERA_A)
    try:
        f = view_fixture(r, p, 0, LW, LH, CAMERA_A, CAMERA_B, (5, 6), (8,))
        ref = passes_in_a(f, (5, 6))
        out, st = reproject_to_b(f, ref)
        assert 0 < st["reset_pixels"] < LW * LH
        check(r, out, "131 x 11")
        then_a_pass_in_b(f, out, what="131 x 11")
    finally:
        r.close()


def test_reset_tiles_are_core_and_an_adaptive_pass_refines_exactly_them(cornell):
    r, p = cornell["r"], cornell["p"]
    ref = passes_in_a(cornell, (5, 6, 7))
    out, _st = reproject_to_b(cornell, ref)
    reset = out.n == 0
    tiles = np.array([reset[y:y + 4, x:x + 4].any() for y in range(0, H, 4) for x in range(0, W, 4)])
    assert 0 < tiles.sum() < tiles.size
    kw = dict(tile_px=4, threshold=1e9, min_samples=8)   # the threshold leaves every tile inactive
    mask, _err, at, ap = r.accum_select(**kw)
    np.testing.assert_array_equal(mask, tiles.astype(np.uint8))
    assert at == int(tiles.sum()) and ap == 16 * at
    seed(r, p, 8)
    mask2, ap2, _stats = r.accum_add_adaptive(1, **kw)
    np.testing.assert_array_equal(mask2, mask)
    where = ar.pixel_mask(mask, W, H, 4)
    out.add_samples(cornell["smp"][8], BW, where)
    _m, _v, counts, _n = check(r, out, "adaptive pass over the reset tiles")
    before = np.where(reset, 0, 12)
    np.testing.assert_array_equal(counts - before, np.where(where, 4, 0))
    assert ap2 == int(where.sum())


def test_nothing_counting_leaves_the_state_of_a_reset(cornell):
    r = cornell["r"]
    ref = passes_in_a(cornell, (5, 6))
    closed = dict(depth_tol=0.0, normal_min=1.0, albedo_tol=0.0)
    out, st = reproject_to_b(cornell, ref, **closed)
    assert not out.n.any()                               # the fixture condition, on the restatement
    assert st == dict(kept_pixels=0, reset_pixels=W * H, kept_samples=0)
    mean, var, n, noise = r.accum_get()
    counts, total = r.accum_get_counts()
    assert not mean.any() and not var.any() and not counts.any()
    assert (n, total, noise) == (0, 0, 0.0)
    then_a_pass_in_b(cornell, out, what="an emptied accumulator")


def test_release_scratch_before_the_reprojection_changes_nothing(cornell):
    r = cornell["r"]
    ref = passes_in_a(cornell, (5, 6, 7), release=True)
    out, _st = reproject_to_b(cornell, ref)
    check(r, out, "after gi_release_scratch")
    r.release_scratch()
    then_a_pass_in_b(cornell, out, what="released again")


def test_null_parameters_are_the_defaults_and_outputs_are_optional(cornell):
    r, L = cornell["r"], gi_amd.lib()
    view, fa, fb = cornell["view"][0], cornell["feat"][0], cornell["feat"][1]
    got = []
    for params, want_stats, want_ms in ((None, True, True), (gi_amd.reproject_params(), False, True),
                                        (None, True, False), (None, False, False)):
        passes_in_a(cornell, (5, 6))
        r.set_camera(*CAMERA_B)
        st, ms = gi_amd.ReprojectStats(), C.c_double(-1.0)
        rc = L.gi_accum_reproject(r._ctx, C.byref(view), fa.ctypes.data, fb.ctypes.data,
                                  None if params is None else C.byref(params),
                                  C.byref(st) if want_stats else None,
                                  C.byref(ms) if want_ms else None)
        assert rc == gi_amd.GI_OK
        assert (ms.value >= 0.0) == want_ms
        if want_stats:
            assert st.kept_pixels + st.reset_pixels == W * H and st.kept_pixels > 0
        got.append(r.accum_get() + r.accum_get_counts())
    for g in got[1:]:
        same_bits(g[0], got[0][0], "mean")
        same_bits(g[1], got[0][1], "variance")
        np.testing.assert_array_equal(g[4], got[0][4])
        assert g[2:4] == got[0][2:4]
    dflt = gi_amd.reproject_params()
    assert (dflt.max_history, dflt.depth_tol, dflt.normal_min, dflt.albedo_tol) == (32, 0.02, 0.9, 0.05)


def test_error_codes(cornell):
    L = gi_amd.lib()
    view, fa, fb = cornell["view"][0], cornell["feat"][0], cornell["feat"][1]

    def call(ctx, v=view, a=fa, b=fb, **kw):
        return L.gi_accum_reproject(ctx, None if v is None else C.byref(v),
                                    None if a is None else a.ctypes.data,
                                    None if b is None else b.ctypes.data,
                                    C.byref(gi_amd.reproject_params(**kw)), None, None)

    r = gi_amd.Renderer(0)
    try:
        v = gi_amd.View()
        assert L.gi_get_view(r._ctx, C.byref(v)) == gi_amd.GI_ERR_STATE      # no scene
        assert call(r._ctx) == gi_amd.GI_ERR_STATE                           # no accumulator
        r.accum_reset(W, H)
        assert call(r._ctx) == gi_amd.GI_ERR_STATE                           # still no scene
        r.ReadScene(cc.dimmed_cornell())
        assert L.gi_get_view(r._ctx, C.byref(v)) == gi_amd.GI_OK
        assert L.gi_get_view(r._ctx, None) == gi_amd.GI_ERR_ARG
        assert call(r._ctx) == gi_amd.GI_OK                  # an empty accumulator: nothing to carry
        assert not r.accum_get_counts()[0].any()
    finally:
        r.close()
    r2 = gi_amd.Renderer(0)
    try:   # a scene but no reset
        r2.ReadScene(cc.dimmed_cornell())
        assert call(r2._ctx) == gi_amd.GI_ERR_STATE
    finally:
        r2.close()
    ctx = cornell["r"]._ctx
    passes_in_a(cornell, (5, 6))
    before = cornell["r"].accum_get() + cornell["r"].accum_get_counts()
    nan, inf = float("nan"), float("inf")
    bad = [call(ctx, v=None), call(ctx, a=None), call(ctx, b=None)]
    for kw in (dict(max_history=1), dict(max_history=0), dict(max_history=-5), dict(depth_tol=-0.1),
               dict(depth_tol=nan), dict(depth_tol=inf), dict(albedo_tol=-0.1), dict(albedo_tol=nan),
               dict(albedo_tol=inf), dict(normal_min=-0.1), dict(normal_min=1.1), dict(normal_min=nan)):
        bad.append(call(ctx, **kw))
    assert bad == [gi_amd.GI_ERR_ARG] * len(bad)
    with pytest.raises(ValueError):
        cornell["r"].accum_reproject(view, fa[:, :-1], fb)
    after = cornell["r"].accum_get() + cornell["r"].accum_get_counts()
    same_bits(after[0], before[0], "mean after the refused calls")
    same_bits(after[1], before[1], "variance after the refused calls")
    np.testing.assert_array_equal(after[4], before[4])
    assert after[2:4] == before[2:4]
    r3 = gi_amd.Renderer(devices=[0, 0])
    try:
        assert call(r3._ctx) == gi_amd.GI_ERR_UNSUPPORTED
    finally:
        r3.close()
