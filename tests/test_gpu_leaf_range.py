"""The kd leaves' photon ranges as the k-NN kernels compute them (csrc/gi_layout.h kd_leaf_range:
start(j) = (j * n) >> levels, where the kernels used to divide by nleaves), against the oracle.

The 64-bit division the shift replaced had a 32-bit path for products below 2^32 and a long one
above, so the cases sit on both sides of that line and at ragged leaves:

  big     300,001 photons at GI_LEAF_SIZE=16: L = 32,768 leaves of 9 or 10 photons (n % L != 0),
          and leaf * n >= 2^32 from leaf 14,317 on. 2,048 queries, 1,024 in a patch whose whole
          neighbourhood lies in leaves below that index and 1,024 in one above it, each half in
          Morton order as test_gpu_estimate_bits.py sorts its clustered set, so that 64
          consecutive queries fit a chunk's LDS and the chunk kernels serve them themselves.
  ragged  1,000 photons at the same leaf size: L = 64, 15 or 16 photons per leaf.
  tiny    17 photons: L = 2, leaves of 8 and 9, and K = 50 > n (num < K).

Per map: kinds 7, 1, 3 and 0 at K = 50, kinds 8 and 1 at K = 225, kind 10 (the fixed-radius
estimate) with K above n. The neighbour sets (FindClosestQuick), out_n and out_maxd2 equal the
oracle's exactly; out within rtol 1e-10 (fp64 sums in another order: the tolerance of
test_gpu_knn_variants.py). Where the K-th and (K+1)-th fp32 distances of a query are equal the
two sides may keep either photon, so `out` is compared on the other
queries, as test_caustic_focus_rim does."""
import functools

import numpy as np
import pytest

import oracle_lib
import synth
from gi_amd import DISK, GLOBAL
from test_gpu_knn_variants import make_renderer

pytestmark = pytest.mark.gpu

LEAF = 16
N_BIG, L_BIG, LEVELS_BIG = 300001, 32768, 15
T_BIG = -(-(1 << 32) // N_BIG)   # first j with j * N_BIG >= 2^32
ALL = 1 << 30

# (kind, K, r of the big map): r well above the K-neighbourhood there (0.02 at K = 50, 0.04 at
# K = 225), so num == K; the range estimate's r holds ~120 photons
KINDS = [(7, 50, 0.5), (1, 50, 0.5), (3, 50, 0.5), (0, 50, 0.5), (8, 225, 0.225), (1, 225, 0.225),
         (10, ALL, 0.03)]
IDS = [f"kind{k}-K{'all' if K == ALL else K}" for k, K, _ in KINDS]


def env_of(kind):
    return {"GI_KNN_KERNEL": str(kind), "GI_LEAF_SIZE": str(LEAF)}


def start(n, levels, j):
    return (j * n) >> levels


@functools.lru_cache(maxsize=None)
def photons(n):
    return synth.photon_map(n, seed=n + 5)


def morton(pts):
    """Order of pts along a 10-bit Morton curve over their own bounding box."""
    lo, hi = pts.min(0), pts.max(0)
    g = np.clip(((pts - lo) / np.maximum(hi - lo, 1e-12) * 1024).astype(np.int64), 0, 1023)
    key = np.zeros(len(pts), dtype=np.int64)
    for b in range(10):
        for ax in range(3):
            key |= ((g[:, ax] >> b) & 1) << (3 * b + ax)
    return np.argsort(key, kind="stable")


@functools.lru_cache(maxsize=None)
def big_setup():
    """(leaf of every photon by emission index, the two patches' query points and normals)."""
    ph = photons(N_BIG)
    r_ = make_renderer(env_of(7))
    try:
        r_.set_photon_map(GLOBAL, ph)
        _, perm, nl = r_.kd_tree(GLOBAL)
    finally:
        r_.close()
    assert nl == L_BIG == 1 << LEVELS_BIG and len(perm) == N_BIG
    assert sorted(perm.tolist()) == list(range(N_BIG))
    starts = np.array([start(N_BIG, LEVELS_BIG, j) for j in range(L_BIG + 1)], dtype=np.int64)
    assert starts[-1] == N_BIG and set(np.diff(starts).tolist()) == {9, 10}
    leaf_kd = np.searchsorted(starts, np.arange(N_BIG), side="right") - 1
    leaf = np.zeros(N_BIG, dtype=np.int64)
    leaf[perm] = leaf_kd
    pos = ph["pos"].astype(np.float64)
    rng = np.random.default_rng(53)
    box = np.float32(1.1)

    def patch(cands, ok):
        # the first anchor (four consecutive leaves) around which every photon within 0.12, past
        # the K = 225 neighbourhood of any query of the patch, is in a leaf on the wanted side
        for a in cands:
            anchor = perm[starts[a]:starts[a + 4]]
            c = pos[anchor].mean(0)
            near = ((pos - c) ** 2).sum(1) <= 0.12 ** 2
            if near.sum() >= 1000 and ok(leaf[near]).all():
                break
        else:
            raise AssertionError("no anchor leaf with a one-sided neighbourhood")
        p = pos[rng.choice(anchor, 1024)]
        on_face = (ph["pos"][anchor[0]] == 0) | (ph["pos"][anchor[0]] == box)
        ax = int(np.argmax(on_face))
        jit = (rng.random((1024, 3)) - 0.5) * 0.01
        jit[:, ax] = 0.0
        p = np.clip(p + jit, 0.0, float(box))
        p[:, ax] = pos[anchor[0], ax]
        nrm = np.zeros((1024, 3))
        nrm[:, ax] = 1.0 if pos[anchor[0], ax] == 0 else -1.0
        o = morton(p)
        return p[o], nrm[o]

    lo_p, lo_n = patch(range(500, T_BIG - 500, 250), lambda l: l + 1 < T_BIG)
    hi_p, hi_n = patch(range(T_BIG + 500, L_BIG - 500, 250), lambda l: l >= T_BIG)
    return leaf, np.concatenate([lo_p, hi_p]), np.concatenate([lo_n, hi_n])


def big_queries(K, r):
    _, pts, nrm = big_setup()
    q = synth.queries(len(pts), seed=19, k=K, r=r, filt=DISK, spec=True)
    q["ks"][(np.arange(len(pts)) // 96) % 2 == 1] = 0.0
    q["point"] = pts
    q["normal"] = nrm
    return q


def small_queries(K, r):
    """Scattered queries and a dense Morton-ordered patch."""
    cl = synth.clustered_queries(256, 17, K, r, DISK)
    cl = cl[morton(cl["point"])]
    return np.concatenate([synth.queries(320, seed=7, k=K, r=r, filt=DISK, spec=True), cl])


@functools.lru_cache(maxsize=None)
def reference(n, K, r):
    """(queries, oracle estimate, oracle k-NN lists or None, queries whose K-th distance is untied)."""
    ph = photons(n)
    q = big_queries(K, r) if n == N_BIG else small_queries(K, r)
    est = oracle_lib.estimate_radiance(ph, q)
    if K == ALL:
        return q, est, None, np.ones(len(q), dtype=bool)
    lists = oracle_lib.knn(ph, q["point"], K, r)
    _, od, on = oracle_lib.knn(ph, q["point"], K + 1, r)
    tied = (on == K + 1) & (od[:, K - 1] == od[:, min(K, od.shape[1] - 1)])
    return q, est, lists, ~tied


def run_and_check(n, kind, K, r):
    ph = photons(n)
    q, (o, on, om), lists, untied = reference(n, K, r)
    r_ = make_renderer(env_of(kind))
    try:
        r_.set_photon_map(GLOBAL, ph)
        g, gn, gm = r_.EstimateRadiance(GLOBAL, q)
        if lists is not None:
            gi, gd, gln = r_.FindClosestQuick(GLOBAL, q["point"], K, r)
    finally:
        r_.close()
    print(f"n {n} kind {kind} K {K}: photons per query {on.min()}..{on.max()}, tied {(~untied).sum()}")
    assert untied.mean() > 0.99
    np.testing.assert_array_equal(gn, on)
    np.testing.assert_array_equal(gm.view(np.uint32), om.view(np.uint32))
    np.testing.assert_allclose(g[untied], o[untied], rtol=1e-10, atol=1e-300)
    if lists is None:
        return
    oi, od, oln = lists
    np.testing.assert_array_equal(gln, oln)
    for i in range(len(q)):
        m = gln[i]
        np.testing.assert_array_equal(np.sort(gd[i, :m]), od[i, :m])
        order = np.lexsort((gi[i, :m], gd[i, :m]))
        got = gi[i, :m][order]
        mism = got != oi[i, :m]
        assert np.all(gd[i, :m][order][mism] == od[i, m - 1]), (i, got[mism])


def test_big_map_queries_sit_on_both_sides_of_2_32():
    """The premise of the big case: every neighbour of the first 1,024 queries lies in a leaf whose
    two starts have products below 2^32, every neighbour of the others in one at or above it."""
    leaf, pts, _ = big_setup()
    for K, r in ((50, 0.5), (225, 0.225)):
        oi, _, on = reference(N_BIG, K, r)[2]
        assert (on == K).all()
        lo, hi = leaf[oi[:1024]], leaf[oi[1024:]]
        assert ((lo + 1) * N_BIG < 1 << 32).all()
        assert (hi * N_BIG >= 1 << 32).all()
    on = reference(N_BIG, ALL, 0.03)[1][1]
    assert on.min() > 0 and on.max() > 64


@pytest.mark.parametrize("kind,K,r", KINDS, ids=IDS)
def test_products_cross_2_32(kind, K, r):
    run_and_check(N_BIG, kind, K, r)


@pytest.mark.parametrize("n", [1000, 17])
@pytest.mark.parametrize("kind,K,r", KINDS, ids=IDS)
def test_ragged_leaves(n, kind, K, r):
    # r = 2.5 holds the whole map: num = min(K, n), so the 17-photon map has num < K for every K;
    # the range estimate keeps a radius that holds a part of the 1,000-photon map
    run_and_check(n, kind, K, 0.3 if K == ALL else 2.5)
