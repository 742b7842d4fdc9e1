"""Adaptive passes (gi.h "adaptive passes") on the device against tests/adaptive_ref.py, bit for
bit: the per-pixel sample counts, the tile error and selection kernels, masked passes and the
calls built on them.

Fixtures: the dimmed cornell view of camera_cases ("cornell_dim": most values inside (0, 1)) at
24 x 16, and the 37 x 21 stilllife frame of test_gpu_radiance.py (clipped tiles, 777 pixels),
both at aa 1; the depth-of-field teapot at aa 0. Every pass's samples come from
gi_render_radiance of the whole frame under the pass's seed: a camera sample's RNG stream is
keyed by its place in the frame, so a masked pass must reproduce them.
"""
import ctypes as C
import os

import numpy as np
import pytest

import adaptive_ref as ar
import camera_cases as cc
import feature_cases as fc
import gi_amd
import radiance_ref as rr
import ray_cases

pytestmark = pytest.mark.gpu

W, H = 24, 16
SW, SH = 37, 21
BW = rr.box_weight(aa=1)
# the depth-of-field teapot of test_gpu_radiance.py: 20 x 20, aa 0, two lens samples
TEAPOT_ARGS = fc.camera_args("teapot_dof") + ["-global", "5000", "-caustic", "5000", "-it", "4",
                                              "-seed", "3"]
COUNTERS = ("screen_rays", "shadow_rays", "monte_carlo_rays", "transmissive_samples",
            "specular_samples", "indirect_samples", "caustic_samples", "knn_queries",
            "knn_photons")


def same_bits(dev, ref, what=""):
    dev, ref = np.ascontiguousarray(dev), np.ascontiguousarray(ref)
    assert dev.dtype == ref.dtype and dev.shape == ref.shape, (dev.dtype, ref.dtype, dev.shape, ref.shape)
    u = {4: np.uint32, 8: np.uint64, 1: np.uint8}[dev.dtype.itemsize]
    nd = int((dev.view(u) != ref.view(u)).sum())
    print(f"{what}: {nd} of {dev.size} values differ")
    assert nd == 0, (what, np.argwhere(dev.view(u) != ref.view(u))[:8].tolist())


def make_context(args, camera=None, env=None):
    """A context of its own with the scene read and the maps built; (renderer, params, aa)."""
    p, sc, _o, _w, _h, aa, real = gi_amd.ParseArgs(args)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        r = gi_amd.Renderer(0, p)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    r.ReadScene(sc, real)
    if camera is not None:
        r.set_camera(*camera)
    r.MapPhotons()
    return r, p, aa


def seed(r, p, s):
    p.seed = s
    r.set_params(p)


def frame_samples(r, p, aa, w, h, seeds):
    """seed -> samples [H, W, 4^aa, 3] of the whole frame (read-only)."""
    out = {}
    for s in seeds:
        seed(r, p, s)
        out[s] = r.render_radiance(aa, w, h, want_samples=True)[2]
        out[s].setflags(write=False)
    return out


def pixel_hits(r, aa, w, h):
    """[H, W]: how many of each pixel's primary rays (gi_camera_rays under the current parameters)
    hit the scene. screen_rays counts those, as the reference's -v report does: a pass over a
    pixel list reports the sum over its pixels, which is pixels * 4^aa * dof_test where every ray
    hits."""
    rays, _ids = r.camera_rays(aa, w, h)
    hit = r.Intersects(rays["org"], rays["dir"])[0]
    return (hit != 0).reshape(h, w, -1).sum(axis=2)


def check_screen_rays(st, hits, where, per_pixel):
    want = int(hits[where].sum())
    print(f"screen rays {st['screen_rays']}, hits {want}, primary rays {int(where.sum()) * per_pixel}")
    assert st["screen_rays"] == want
    if (hits[where] == per_pixel).all():
        assert st["screen_rays"] == int(where.sum()) * per_pixel


def cornell_args():
    return [cc.dimmed_cornell(), "/tmp/x.png"] + cc.CORNELL_FLAGS


CORNELL_CAMERA = cc.camera_of(cc.CASES["cornell_dim"][1])


@pytest.fixture(scope="module")
def cornell():
    r, p, aa = make_context(cornell_args(), CORNELL_CAMERA)
    assert aa == 1
    d = dict(r=r, p=p, w=W, h=H, smp=frame_samples(r, p, 1, W, H, (5, 6, 7)))
    yield d
    r.close()


@pytest.fixture(scope="module")
def cornell2():
    """A second context on the same scene, camera and maps (the maps are a function of the seed)."""
    r, p, _aa = make_context(cornell_args(), CORNELL_CAMERA)
    yield dict(r=r, p=p, w=W, h=H)
    r.close()


@pytest.fixture(scope="module")
def still():
    r, p, _aa = make_context(ray_cases.scene_args("stilllife", SW, SH))
    d = dict(r=r, p=p, w=SW, h=SH, smp=frame_samples(r, p, 1, SW, SH, (5, 6)))
    yield d
    r.close()


def two_passes(f):
    """Reset and fold the whole-frame passes under seeds 5 and 6; the restatement's accumulator
    (when the fixture holds the samples)."""
    r, p = f["r"], f["p"]
    r.accum_reset(f["w"], f["h"])
    ref = ar.Accum((f["h"], f["w"])) if "smp" in f else None
    for s in (5, 6):
        seed(r, p, s)
        r.accum_add_image(1)
        if ref is not None:
            ref.add_samples(f["smp"][s], BW)
    return ref


def check(r, ref, what):
    """gi_accum_get and gi_accum_get_counts against the restatement."""
    mean, var, n, noise = r.accum_get()
    counts, total = r.accum_get_counts()
    rmean, rvar, rn, rnoise = ref.get()
    print(f"{what}: smallest count {n}, total {total}, noise {noise!r} (restatement {rnoise!r})")
    np.testing.assert_array_equal(counts, ref.n)
    assert total == int(ref.n.sum())
    assert n == rn == int(counts.min())
    same_bits(mean, rmean, what + " mean")
    same_bits(var, rvar, what + " variance")
    assert noise == rnoise
    return mean, var, counts, noise


def median_threshold(err, frac=0.5):
    """The midpoint of two adjacent, different values of the sorted tile errors, the nearest pair
    to the median (or to another quantile): no tile sits on it."""
    s = np.sort(err)
    k0 = int(len(s) * frac)
    for k in sorted(range(1, len(s)), key=lambda k: abs(k - k0)):
        if s[k - 1] < s[k]:
            return 0.5 * (float(s[k - 1]) + float(s[k]))
    raise AssertionError("every tile has the same error")


# ---- 1. selection ----------------------------------------------------------------------------
@pytest.mark.parametrize("which,T,grid", [("cornell", 4, (6, 4)), ("still", 8, (5, 3))])
def test_selection_matches_restatement(request, which, T, grid):
    f = request.getfixturevalue(which)
    r, w, h = f["r"], f["w"], f["h"]
    ref = two_passes(f)
    assert ar.tile_grid(w, h, T) == grid
    tx, ty = grid
    err, nmin, inside = ar.tile_errors(ref, T)
    assert (nmin == 8).all()
    thr = median_threshold(err)
    share = float((err > thr).mean())
    print(f"{which}: threshold {thr!r}, {share:.3f} of {len(err)} tiles above it")
    assert 0.25 <= share <= 0.75           # the fixture condition, on the restatement alone
    got_err = None
    for dilate in (0, 1):
        want = ar.select(err, nmin, tx, ty, dilate=dilate, threshold=thr)
        assert (want["by_error"] == (err > thr)).all()
        mask, derr, at, ap = r.accum_select(tile_px=T, dilate=dilate, threshold=thr)
        same_bits(derr, err, f"{which} tile error (dilate {dilate})")
        np.testing.assert_array_equal(mask, want["active"].astype(np.uint8))
        assert at == int(want["active"].sum()) and ap == int(inside[want["active"]].sum())
        if dilate:
            assert want["dilated"].any() and at > int((err > thr).sum())
        got_err = derr
        # max_samples equal to the count every pixel has: nothing left to refine
        mask, derr, at, ap = r.accum_select(tile_px=T, dilate=dilate, threshold=thr, max_samples=8)
        assert not mask.any() and (at, ap) == (0, 0)
        same_bits(derr, err, "tile error under max_samples")
    # min_samples above the count: every tile, whatever its error
    mask, _e, at, ap = r.accum_select(tile_px=T, threshold=1e9, min_samples=9)
    assert mask.all() and at == tx * ty and ap == w * h
    # only the counts: the optional outputs may be null
    at2 = C.c_int64(-1)
    p = gi_amd.adaptive_params(tile_px=T, threshold=thr, dilate=0)
    assert gi_amd.lib().gi_accum_select(r._ctx, C.byref(p), None, None, C.byref(at2), None) == gi_amd.GI_OK
    assert at2.value == int((got_err > thr).sum())


# ---- 2.-4. masked passes ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def masked(cornell):
    """Seeds 5 and 6 whole, then seed 7 over a checkerboard of 4 x 4 tiles and over its complement;
    seeds 5, 6 and 7 whole on a fresh accumulator."""
    r, p = cornell["r"], cornell["p"]
    ref = two_passes(cornell)
    before = r.accum_get()
    board = ar.checkerboard(W, H, 4)
    where = ar.pixel_mask(board, W, H, 4)
    seed(r, p, 7)
    hits = pixel_hits(r, 1, W, H)
    ap, st = r.accum_add_tiles(1, 4, board)
    ref.add_samples(cornell["smp"][7], BW, where)
    half = check(r, ref, "checkerboard pass")
    ap2, st2 = r.accum_add_tiles(1, 4, 1 - board)
    ref.add_samples(cornell["smp"][7], BW, ~where)
    both = check(r, ref, "complement pass")
    two_passes(cornell)
    seed(r, p, 7)
    st_full = r.accum_add_image(1)
    full = r.accum_get()
    return dict(before=before, where=where, hits=hits, ap=ap, st=st, half=half, ap2=ap2, st2=st2, both=both,
                st_full=st_full, full=full)


def test_masked_pass_matches_restatement_and_leaves_the_rest(masked):
    where = masked["where"]
    assert where.sum() == W * H // 2 == masked["ap"] == masked["ap2"]
    mean0, var0, n0, _noise0 = masked["before"]
    mean, var, counts, noise = masked["half"]
    assert n0 == 8
    same_bits(mean[~where], mean0[~where], "inactive mean")
    same_bits(var[~where], var0[~where], "inactive variance")
    assert (mean[where] != mean0[where]).any()
    assert (counts[where] == 12).all() and (counts[~where] == 8).all()
    assert noise > 0.0


def test_mask_and_complement_are_the_whole_frame_pass(masked):
    mean, var, counts, noise = masked["both"]
    fmean, fvar, fn, fnoise = masked["full"]
    assert (counts == 12).all() and fn == 12
    same_bits(mean, fmean, "mean")
    same_bits(var, fvar, "variance")
    assert noise == fnoise
    # counters: the two halves add up to the frame's, each of the nine
    check_screen_rays(masked["st"], masked["hits"], masked["where"], 4)
    check_screen_rays(masked["st2"], masked["hits"], ~masked["where"], 4)
    assert masked["hits"].max() == 4
    for k in COUNTERS:
        print(k, masked["st"][k], masked["st2"][k], masked["st_full"][k])
        assert masked["st"][k] + masked["st2"][k] == masked["st_full"][k], k
    assert masked["st"]["knn_queries"] > 0


def test_all_ones_mask_is_a_whole_frame_pass(cornell, masked):
    r, p = cornell["r"], cornell["p"]
    two_passes(cornell)
    seed(r, p, 7)
    ap, st = r.accum_add_tiles(1, 4, np.ones(24, dtype=np.uint8))
    assert ap == W * H
    mean, var, n, noise = r.accum_get()
    fmean, fvar, fn, fnoise = masked["full"]
    same_bits(mean, fmean, "mean")
    same_bits(var, fvar, "variance")
    assert (n, noise) == (fn, fnoise)
    for k in COUNTERS:
        assert st[k] == masked["st_full"][k], k
    # another tile size cuts the same frame
    two_passes(cornell)
    seed(r, p, 7)
    ap, st = r.accum_add_tiles(1, 64, np.ones(1, dtype=np.uint8))
    assert ap == W * H
    same_bits(r.accum_get()[0], fmean, "one 64 x 64 tile")


# ---- 5. a masked pass that the slot guard splits ---------------------------------------------
def test_split_masked_pass_equals_the_unsplit_one(still):
    board = ar.checkerboard(SW, SH, 8)
    where = ar.pixel_mask(board, SW, SH, 8)
    got = []
    small, ps, _aa = make_context(ray_cases.scene_args("stilllife", SW, SH), env={"GI_SLOT_LIMIT": "9000"})
    try:
        for r, p in ((still["r"], still["p"]), (small, ps)):
            r.accum_reset(SW, SH)
            seed(r, p, 5)
            r.accum_add_image(1)
            seed(r, p, 6)
            ap, st = r.accum_add_tiles(1, 8, board)
            assert ap == int(where.sum())
            check_screen_rays(st, pixel_hits(r, 1, SW, SH), where, 4)
            got.append(r.accum_get() + r.accum_get_counts() + (st,))
    finally:
        small.close()
    a, b = got
    print("k-NN launches unsplit / split:", a[6]["knn_kernel_launches"], b[6]["knn_kernel_launches"])
    assert b[6]["knn_kernel_launches"] > a[6]["knn_kernel_launches"]    # the list was split
    np.testing.assert_array_equal(a[4], b[4])
    assert (a[4][where] == 8).all() and (a[4][~where] == 4).all() and a[2] == b[2] == 4
    for k in COUNTERS:
        assert a[6][k] == b[6][k], k
    same_bits(b[0], a[0], "mean")
    same_bits(b[1], a[1], "variance")
    assert b[3] == a[3]
    # and both are the restatement's
    ref = ar.Accum((SH, SW))
    ref.add_samples(still["smp"][5], BW)
    ref.add_samples(still["smp"][6], BW, where)
    same_bits(a[0], ref.get()[0], "mean against the restatement")
    same_bits(a[1], ref.get()[1], "variance against the restatement")
    assert a[3] == ref.get()[3]


# ---- 6. depth of field -----------------------------------------------------------------------
def test_depth_of_field_masked_pass_matches_restatement():
    r, p, aa = make_context(TEAPOT_ARGS)
    try:
        assert aa == 0 and p.dof_test == 2
        smp = frame_samples(r, p, 0, 20, 20, (3, 4))
        board = ar.checkerboard(20, 20, 4)
        where = ar.pixel_mask(board, 20, 20, 4)
        ref = ar.Accum((20, 20))
        r.accum_reset(20, 20)
        seed(r, p, 3)
        r.accum_add_image(0)
        ref.add_samples(smp[3], 1.0)
        seed(r, p, 4)
        hits = pixel_hits(r, 0, 20, 20)                 # two lens samples per sub-cell
        ap, st = r.accum_add_tiles(0, 4, board)
        ref.add_samples(smp[4], 1.0, where)
        assert ap == int(where.sum()) == 208
        check_screen_rays(st, hits, where, 2)
        _m, _v, counts, _n = check(r, ref, "teapot -dof")
        assert (counts[where] == 2).all() and (counts[~where] == 1).all()
        assert smp[4][where].any()
    finally:
        r.close()


# ---- 7. gi_accum_add_adaptive ----------------------------------------------------------------
def test_add_adaptive_is_select_then_add_tiles(cornell, cornell2):
    ref = two_passes(cornell)
    two_passes(cornell2)
    err, nmin, _inside = ar.tile_errors(ref, 4)
    thr = median_threshold(err, 0.75)
    want = ar.select(err, nmin, 6, 4, threshold=thr)["active"]
    assert 0 < want.sum() < 24            # the fixture condition: a part of the frame
    for f in (cornell, cornell2):
        seed(f["r"], f["p"], 7)
    mask, ap, st = cornell["r"].accum_add_adaptive(1, tile_px=4, threshold=thr)
    mask2, _err, at2, ap2 = cornell2["r"].accum_select(tile_px=4, threshold=thr)
    ap3, st3 = cornell2["r"].accum_add_tiles(1, 4, mask2)
    np.testing.assert_array_equal(mask, mask2)
    np.testing.assert_array_equal(mask, want.astype(np.uint8))
    assert ap == ap2 == ap3 == 16 * at2
    for k in COUNTERS:
        assert st[k] == st3[k], k
    a, b = cornell["r"].accum_get(), cornell2["r"].accum_get()
    same_bits(a[0], b[0], "mean")
    same_bits(a[1], b[1], "variance")
    assert a[2:] == b[2:]
    np.testing.assert_array_equal(cornell["r"].accum_get_counts()[0], cornell2["r"].accum_get_counts()[0])
    ref.add_samples(cornell["smp"][7], BW, ar.pixel_mask(mask, W, H, 4))
    check(cornell["r"], ref, "adaptive pass")


# ---- 8. the loop a caller runs ---------------------------------------------------------------
def run_loop(f, limit, **kw):
    """gi_accum_add_adaptive under seeds 5, 6, ... from an empty accumulator until a pass selects
    nothing (at most `limit` calls); the active tiles of every call."""
    r, p = f["r"], f["p"]
    r.accum_reset(f["w"], f["h"])
    active = []
    for i in range(limit):
        seed(r, p, 5 + i)
        mask, ap, _st = r.accum_add_adaptive(1, **kw)
        active.append(int(mask.sum()))
        assert ap == 16 * active[-1]
        if ap == 0:
            break
    print("active tiles per call:", active)
    return active


def test_loop_ends_with_no_active_tile(cornell):
    """With threshold 0 a tile with any error is active in every pass until its smallest count
    reaches max_samples (and so are the tiles it dilates into): max_samples / 4^aa passes, and the
    next call selects nothing. With a threshold inside the errors' range a tile can become active
    late; then each pass with an active tile raises the smallest count of at least one tile that
    is below max_samples by 4^aa, which bounds the passes by tiles * max_samples / 4^aa."""
    r = cornell["r"]
    max_samples, S = 16, 4
    limit = max_samples // S + 1
    kw = dict(tile_px=4, threshold=0.0, max_samples=max_samples)
    active = run_loop(cornell, limit, **kw)
    assert active[-1] == 0 and len(active) <= limit
    assert active[0] == active[1] == 24          # below min_samples: whole frames
    counts, total = r.accum_get_counts()
    assert counts.max() <= max_samples + S - 1 and counts.min() >= 8
    assert total == 16 * S * sum(active)
    assert r.accum_select(**kw)[2] == 0
    # a threshold at the median of the errors after two passes
    thr = median_threshold(ar.tile_errors(two_passes(cornell), 4)[0])
    kw["threshold"] = thr
    active = run_loop(cornell, 24 * max_samples // S + 1, **kw)
    assert active[-1] == 0
    assert active[0] == active[1] == 24 and 0 < active[2] < 24
    counts, total = r.accum_get_counts()
    assert counts.max() <= max_samples + S - 1 and counts.min() >= 8
    assert total == 16 * S * sum(active)
    assert counts.min() < counts.max()           # the samples went where the error is
    assert r.accum_select(**kw)[2] == 0


# ---- 9. empty mask ---------------------------------------------------------------------------
def test_empty_mask_renders_nothing(cornell):
    r, p = cornell["r"], cornell["p"]
    two_passes(cornell)
    before = r.accum_get()
    counts0, total0 = r.accum_get_counts()
    st = gi_amd.RenderStats()
    st.screen_rays, st.render_s = 77, 1.5
    ap = C.c_int64(-1)
    zeros = np.zeros(24, dtype=np.uint8)
    rc = gi_amd.lib().gi_accum_add_tiles(r._ctx, 1, 4, zeros.ctypes.data, C.byref(ap), C.byref(st))
    assert rc == gi_amd.GI_OK and ap.value == 0
    assert bytes(st) == bytes(C.sizeof(st))
    after = r.accum_get()
    same_bits(after[0], before[0], "mean")
    same_bits(after[1], before[1], "variance")
    assert after[2:] == before[2:]
    counts, total = r.accum_get_counts()
    np.testing.assert_array_equal(counts, counts0)
    assert total == total0 == 8 * W * H
    # an adaptive pass that selects nothing
    mask, ap2, st2 = r.accum_add_adaptive(1, tile_px=4, threshold=1e9)
    assert not mask.any() and ap2 == 0 and st2["screen_rays"] == 0
    assert r.accum_get()[2:] == before[2:]


# ---- 10. a whole-frame ray pass over unequal counts ------------------------------------------
def test_ray_pass_after_a_masked_pass_matches_restatement(cornell):
    r, p = cornell["r"], cornell["p"]
    rays, ids = ray_cases.batch("cornell_dim", "panorama", 3)
    seed(r, p, 7)
    smp = r.render_rays_radiance(W, H, 3, rays, ids, want_samples=True)[2]
    board = ar.checkerboard(W, H, 4, phase=1)
    where = ar.pixel_mask(board, W, H, 4)
    ref = ar.Accum((H, W))
    r.accum_reset(W, H)
    seed(r, p, 5)
    r.accum_add_image(1)
    ref.add_samples(cornell["smp"][5], BW)
    seed(r, p, 6)
    r.accum_add_tiles(1, 4, board)
    ref.add_samples(cornell["smp"][6], BW, where)
    seed(r, p, 7)
    r.accum_add_rays(3, rays, ids)
    ref.add_samples(smp, rr.box_weight(spp=3))
    _m, _v, counts, _n = check(r, ref, "image, masked, rays")
    assert (counts[where] == 11).all() and (counts[~where] == 7).all()
    # and a whole camera frame on top
    seed(r, p, 7)
    r.accum_add_image(1)
    ref.add_samples(cornell["smp"][7], BW)
    check(r, ref, "image, masked, rays, image")


# ---- 11. error codes -------------------------------------------------------------------------
def test_error_codes(cornell):
    L = gi_amd.lib()
    ones = np.ones(24, dtype=np.uint8)
    dflt = gi_amd.adaptive_params(tile_px=4)
    cnt = np.zeros((H, W), dtype=np.int64)
    r = gi_amd.Renderer(0)
    try:   # before a reset
        got = [L.gi_accum_select(r._ctx, C.byref(dflt), None, None, None, None),
               L.gi_accum_add_tiles(r._ctx, 1, 4, ones.ctypes.data, None, None),
               L.gi_accum_add_adaptive(r._ctx, 1, C.byref(dflt), None, None, None),
               L.gi_accum_get_counts(r._ctx, cnt.ctypes.data, None)]
        assert got == [gi_amd.GI_ERR_STATE] * 4
        # a reset accumulator without a scene: the selection works, a pass has nothing to render
        assert L.gi_accum_reset(r._ctx, W, H) == gi_amd.GI_OK
        at = C.c_int64(-1)
        assert L.gi_accum_select(r._ctx, C.byref(dflt), None, None, C.byref(at), None) == gi_amd.GI_OK
        assert at.value == 24                 # no pixel has min_samples yet
        assert L.gi_accum_add_tiles(r._ctx, 1, 4, ones.ctypes.data, None, None) == gi_amd.GI_ERR_STATE
        total = C.c_int64(-1)
        assert L.gi_accum_get_counts(r._ctx, cnt.ctypes.data, C.byref(total)) == gi_amd.GI_OK
        assert total.value == 0 and not cnt.any()
    finally:
        r.close()
    ctx = cornell["r"]._ctx
    two_passes(cornell)
    before = cornell["r"].accum_get()

    def params(**kw):
        return C.byref(gi_amd.adaptive_params(**kw))

    bad = [L.gi_accum_select(ctx, None, None, None, None, None)]
    for kw in (dict(tile_px=3), dict(tile_px=65), dict(tile_px=0), dict(min_samples=-1),
               dict(max_samples=-1), dict(dilate=2), dict(dilate=-1), dict(threshold=-0.5),
               dict(threshold=float("nan")), dict(threshold=float("inf"))):
        bad.append(L.gi_accum_select(ctx, params(**kw), None, None, None, None))
        bad.append(L.gi_accum_add_adaptive(ctx, 1, params(**kw), None, None, None))
    bad += [L.gi_accum_add_adaptive(ctx, -1, params(tile_px=4), None, None, None),
            L.gi_accum_add_adaptive(ctx, 16, params(tile_px=4), None, None, None),
            L.gi_accum_add_adaptive(ctx, 1, None, None, None, None),
            L.gi_accum_add_tiles(ctx, 1, 4, None, None, None),
            L.gi_accum_add_tiles(ctx, -1, 4, ones.ctypes.data, None, None),
            L.gi_accum_add_tiles(ctx, 16, 4, ones.ctypes.data, None, None),
            L.gi_accum_add_tiles(ctx, 1, 3, ones.ctypes.data, None, None),
            L.gi_accum_add_tiles(ctx, 1, 65, ones.ctypes.data, None, None)]
    assert bad == [gi_amd.GI_ERR_ARG] * len(bad)
    with pytest.raises(ValueError):
        cornell["r"].accum_add_tiles(1, 4, ones[:23])
    after = cornell["r"].accum_get()
    same_bits(after[0], before[0], "mean after the refused calls")
    assert after[2:] == before[2:]
    # a {0, 0} device set
    r = gi_amd.Renderer(devices=[0, 0])
    try:
        got = [L.gi_accum_select(r._ctx, C.byref(dflt), None, None, None, None),
               L.gi_accum_add_tiles(r._ctx, 1, 4, ones.ctypes.data, None, None),
               L.gi_accum_add_adaptive(r._ctx, 1, C.byref(dflt), None, None, None),
               L.gi_accum_get_counts(r._ctx, cnt.ctypes.data, None)]
        assert got == [gi_amd.GI_ERR_UNSUPPORTED] * 4
    finally:
        r.close()
