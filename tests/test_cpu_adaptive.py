"""Properties of tests/adaptive_ref.py, the numpy restatement of gi.h "adaptive passes": the
accumulator with per-pixel counts against radiance_ref.Accum, the tile error's definition on
planes whose result is known, and the selection's clauses one at a time. No GPU.
"""
import numpy as np

import adaptive_ref as ar
import radiance_ref as rr


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def random_passes(shape, sizes, seed=11):
    rng = np.random.default_rng(seed)
    return [rng.gamma(0.7, 0.9, size=tuple(shape) + (S, 3)) for S in sizes]


def test_equal_counts_are_the_frame_count_accumulator_bit_for_bit():
    shape = (7, 9)
    old, new = rr.Accum(shape), ar.Accum(shape)
    for smp in random_passes(shape, (4, 3, 5)):
        bw = rr.box_weight(spp=smp.shape[-2])
        old.add_samples(smp, bw)
        new.add_samples(smp, bw)
        assert (bits(new.mu) == bits(old.mu)).all() and (bits(new.A) == bits(old.A)).all()
        assert (new.n == old.N).all()
        (m0, v0, n0, e0), (m1, v1, n1, e1) = old.get(), new.get()
        assert (bits(m0) == bits(m1)).all() and (bits(v0) == bits(v1)).all()
        assert n0 == n1 and e0 == e1
        assert (bits(ar.pixel_errors(new.mu, new.A, new.n).reshape(-1))
                == bits(rr.pixel_errors(old.mu, old.A, old.N))).all()
    assert old.N == 12


def test_masked_add_leaves_the_other_pixels_alone():
    shape = (16, 24)
    p = random_passes(shape, (4, 4, 4))
    where = ar.pixel_mask(ar.checkerboard(24, 16, 4), 24, 16, 4)
    acc, full = ar.Accum(shape), ar.Accum(shape)
    for smp in p[:2]:
        acc.add_samples(smp, 0.25)
        full.add_samples(smp, 0.25)
    before = (acc.mu.copy(), acc.A.copy())
    acc.add_samples(p[2], 0.25, where)
    full.add_samples(p[2], 0.25)
    assert (acc.n[where] == 12).all() and (acc.n[~where] == 8).all()
    assert (bits(acc.mu[where]) == bits(full.mu[where])).all()
    assert (bits(acc.A[where]) == bits(full.A[where])).all()
    assert (bits(acc.mu[~where]) == bits(before[0][~where])).all()
    assert (bits(acc.A[~where]) == bits(before[1][~where])).all()
    assert acc.get()[2] == 8
    # a pixel without samples takes a masked pass as is
    empty = ar.Accum(shape)
    empty.add_samples(p[0], 0.25, where)
    m, m2 = rr.pass_stats(p[0], 0.25)
    assert (bits(empty.mu[where]) == bits(m[where])).all() and not empty.mu[~where].any()
    assert (bits(empty.A[where]) == bits(m2[where])).all() and empty.get()[2] == 0


def test_tile_error_of_a_constant_error_plane_is_that_error():
    # 0.375 and the pixel counts 16, 64 and 1024 are exact in binary: every partial sum is exact
    for T, w, h in ((4, 24, 16), (8, 32, 16), (32, 64, 32)):
        e = np.full((h, w), 0.375)
        n = np.full((h, w), 8, dtype=np.int64)
        err, nmin, inside = ar.tile_errors_of(e, n, T)
        assert len(err) == (w // T) * (h // T)
        assert (err == 0.375).all() and (nmin == 8).all() and (inside == T * T).all()


def test_clipped_tiles_divide_by_their_own_pixel_count():
    w, h, T = 37, 21, 8
    assert ar.tile_grid(w, h, T) == (5, 3)
    e = np.full((h, w), 0.375)
    n = np.arange(h * w, dtype=np.int64).reshape(h, w) + 2
    err, nmin, inside = ar.tile_errors_of(e, n, T)
    assert inside.reshape(3, 5).tolist() == [[64, 64, 64, 64, 40]] * 2 + [[40, 40, 40, 40, 25]]
    assert int(inside.sum()) == w * h
    assert (err == 0.375).all()       # 0.375 * 40 / 40 and 0.375 * 25 / 25 are exact
    # the smallest count of a tile is its bottom-left pixel's here
    assert nmin.reshape(3, 5)[2, 4] == 16 * w + 32 + 2 and nmin[0] == 2
    # the order of the sum: slots by row of the tile, lane = slot % 64, then the tree
    rng = np.random.default_rng(3)
    e = rng.random((h, w))
    err, _n, _i = ar.tile_errors_of(e, n, T)
    sub = np.zeros((8, 8))
    sub[:5, :5] = e[16:21, 32:37]
    x = sub.reshape(-1).copy()
    for hh in (32, 16, 8, 4, 2, 1):
        x[:hh] = x[:hh] + x[hh:2 * hh]
    assert err[14] == x[0] / 25.0
    # T = 16: four slots per lane, in ascending slot order
    e16 = rng.random((16, 16))
    err16, _n, _i = ar.tile_errors_of(e16, np.full((16, 16), 4, dtype=np.int64), 16)
    q = e16.reshape(4, 64)
    x = ((q[0] + q[1]) + q[2]) + q[3]
    for hh in (32, 16, 8, 4, 2, 1):
        x[:hh] = x[:hh] + x[hh:2 * hh]
    assert err16[0] == x[0] / 256.0


def test_pixels_below_two_samples_have_no_error():
    acc = ar.Accum((4, 4))
    acc.add_samples(random_passes((4, 4), (1,))[0], 1.0)
    assert (acc.n == 1).all() and not ar.pixel_errors(acc.mu, acc.A, acc.n).any()
    err, nmin, _i = ar.tile_errors(acc, 4)
    assert err[0] == 0.0 and nmin[0] == 1


def grid(tx, ty, hot, value=1.0):
    err = np.zeros((ty, tx))
    for x, y in hot:
        err[y, x] = value
    return err.reshape(-1)


def test_dilation_adds_exactly_the_eight_neighbours():
    tx, ty = 7, 5
    nmin = np.full(tx * ty, 8, dtype=np.int64)
    for hot in ((3, 2), (0, 0), (6, 4), (0, 3)):
        err = grid(tx, ty, [hot])
        off = ar.select(err, nmin, tx, ty, dilate=0, threshold=0.5)
        on = ar.select(err, nmin, tx, ty, dilate=1, threshold=0.5)
        assert off["active"].sum() == 1 and not off["dilated"].any()
        want = np.zeros((ty, tx), dtype=bool)
        want[max(0, hot[1] - 1):hot[1] + 2, max(0, hot[0] - 1):hot[0] + 2] = True
        assert (on["active"].reshape(ty, tx) == want).all()
        assert on["core"].sum() == 1 and on["dilated"].sum() == want.sum() - 1
    # a tile on the threshold is not above it
    assert not ar.select(grid(tx, ty, [(3, 2)], 0.5), nmin, tx, ty, threshold=0.5)["active"].any()


def test_max_samples_removes_a_tile_from_core_and_dilated():
    tx, ty = 5, 3
    err = grid(tx, ty, [(2, 1), (3, 1)])
    nmin = np.full(tx * ty, 8, dtype=np.int64)
    nmin[1 * tx + 3] = 32       # a hot tile that has reached max_samples
    nmin[0 * tx + 1] = 32       # a neighbour of the other hot tile that has reached it
    s = ar.select(err, nmin, tx, ty, max_samples=32, threshold=0.5)
    a = s["active"].reshape(ty, tx)
    assert not a[1, 3] and not s["core"].reshape(ty, tx)[1, 3]
    assert not a[0, 1] and not s["dilated"].reshape(ty, tx)[0, 1]
    assert a[1, 2] and a[0, 2] and a[2, 1]
    # (4, 1) neighbours only the finished hot tile: that tile is not core by its error
    assert not a[1, 4]
    assert a.sum() == 7
    # everything at max_samples: nothing is active
    assert not ar.select(err, np.full(tx * ty, 32), tx, ty, max_samples=32, threshold=0.5)["active"].any()


def test_min_samples_forces_a_tile_below_the_threshold():
    tx, ty = 5, 3
    err = np.full(tx * ty, 0.001)
    nmin = np.full(tx * ty, 8, dtype=np.int64)
    nmin[7] = 7
    s = ar.select(err, nmin, tx, ty, min_samples=8, threshold=0.5)
    assert s["active"].tolist() == [i == 7 for i in range(tx * ty)]
    assert s["core"][7] and not s["by_error"].any()
    # ... and it does not dilate: dilation follows the error clause only
    assert not s["dilated"].any()
