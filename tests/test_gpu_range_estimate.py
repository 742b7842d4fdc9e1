"""The fixed-radius estimate (k-NN kind 10, gi_range.hip) against the oracle restatement.

EstimateRadiance (photon_utils.cpp:72-162) with fewer than K photons inside max_dist normalises
by max_dist^2, so an estimate size above the map's photon count *is* the fixed-radius estimate,
and the unmodified oracle restates it. The photon metric is fp32 and identical on both sides:
the photon counts must be equal and max_d2 bit-equal; the fp64 sums run in another order, within
rtol 1e-10 (the suite's estimate tolerance, test_gpu_knn.py)."""
import functools

import numpy as np
import pytest

import gi_amd
import oracle_lib
import synth
from gi_amd import CONE, DISK, GAUSS, GLOBAL
from gpu_util import compare_exact, compare_float_ulp, scene
from test_gpu_configs import COUNTERS
from test_gpu_knn_variants import make_renderer

pytestmark = pytest.mark.gpu

ALL = 1 << 30
CASES = [(DISK, 0.05, False), (DISK, 0.3, True), (CONE, 0.3, False), (GAUSS, 0.3, True),
         (DISK, 2.5, False)]


@functools.lru_cache(maxsize=None)
def big_map():
    return synth.photon_map(30000, seed=7)


def case_queries(filt, r, spec):
    """1000 queries over the box (15 full chunks + 40) and 1000 dense ones on one face."""
    return np.concatenate([synth.queries(1000, seed=3, k=ALL, r=r, filt=filt, spec=spec),
                           synth.clustered_queries(1000, seed=11, k=ALL, r=r, filt=filt)])


def fk_of(filt):
    return 1.25 if filt == CONE else 1.0


def estimate(renderer, ph, q, fk=1.0):
    p = renderer.params
    p.filter_const_k = fk
    renderer.set_params(p)
    try:
        renderer.set_photon_map(GLOBAL, ph)
        return renderer.EstimateRadiance(GLOBAL, q)
    finally:
        p.filter_const_k = 1.0
        renderer.set_params(p)


def check(got, want, r):
    g, gn, gm = got
    o, on, om = want
    np.testing.assert_array_equal(gn, on)
    np.testing.assert_array_equal(gm.view(np.uint32), om.view(np.uint32))
    if r is not None:   # fixed radius: max_dist^2 wherever a photon was found, else 0
        r2f = np.float32(r * r)
        np.testing.assert_array_equal(gm, np.where(gn > 0, r2f, np.float32(0)))
    np.testing.assert_allclose(g, o, rtol=1e-10, atol=1e-300)
    assert (g[gn == 0] == 0).all()


@pytest.mark.parametrize("filt,r,spec", CASES)
def test_seam_matches_oracle(renderer, filt, r, spec):
    ph = big_map()
    q = case_queries(filt, r, spec)
    fk = fk_of(filt)
    got = estimate(renderer, ph, q, fk)
    want = oracle_lib.estimate_radiance(ph, q, filter_k=fk)
    print("photons per query", want[1].min(), want[1].mean(), want[1].max())
    if r == 2.5:
        assert (want[1] == len(ph)).all()   # every photon, many tiles per query
    check(got, want, r)


def test_queries_with_no_photon_in_range(renderer):
    """A radius at which most queries find nothing: their result, count and max_d2 are 0."""
    ph = big_map()
    q = synth.queries(1000, seed=3, k=ALL, r=0.004, filt=DISK, spec=True)
    got = estimate(renderer, ph, q)
    want = oracle_lib.estimate_radiance(ph, q)
    assert (want[1] == 0).sum() > 100 and (want[1] > 0).sum() > 100
    check(got, want, 0.004)


@pytest.fixture(scope="module")
def renderer10():
    r = make_renderer({"GI_KNN_KERNEL": "10"})
    yield r
    r.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_small_shapes(renderer10, n):
    ph = synth.photon_map(n, seed=n + 2)
    for nq in (1, 63, 64, 65, 129):
        q = synth.queries(nq, seed=nq, k=1200, r=2.5, filt=DISK, spec=(nq % 2 == 1))
        got = estimate(renderer10, ph, q)
        want = oracle_lib.estimate_radiance(ph, q)
        check(got, want, 2.5)
        assert (got[1] == n).all()
        if n == 0:
            assert (got[0] == 0).all() and (got[2] == 0).all()


def test_inclusive_bound(renderer):
    """d2 == r2f counts, the next float above does not."""
    ph = synth.photon_map(103, seed=4)
    ph["pos"] += np.float32(5.0)   # 100 far ones
    ph["pos"][0] = (0.5, 0, 0)
    ph["pos"][1] = (np.nextafter(np.float32(0.5), np.float32(1)), 0, 0)
    ph["pos"][2] = (0, 0.5, 0)
    q = synth.queries(1, seed=1, k=ALL, r=0.5, filt=DISK, spec=True)
    q["point"] = 0.0
    q["normal"] = (0.0, 0.0, 1.0)
    assert np.float32(0.5 * 0.5) == 0.25
    got = estimate(renderer, ph, q)
    want = oracle_lib.estimate_radiance(ph, q)
    assert got[1][0] == 2 and want[1][0] == 2
    check(got, want, 0.5)


def test_threshold_between_knn_and_range(renderer):
    """K == n stays with the k-NN kinds (all n photons may be in range: max_d2 is the farthest
    photon's); K == n + 1 is the fixed-radius estimate."""
    n, r = 1200, 2.5
    ph = synth.photon_map(n, seed=9)
    for k in (n, n + 1):
        q = synth.queries(200, seed=5, k=k, r=r, filt=DISK, spec=True)
        got = estimate(renderer, ph, q)
        want = oracle_lib.estimate_radiance(ph, q)
        assert (want[1] == n).all()
        check(got, want, r if k > n else None)
        if k == n:
            d = q["point"].astype(np.float32)[:, None, :] - ph["pos"][None, :, :]
            far = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).max(1)
            assert (got[2] < np.float32(r * r)).all()
            np.testing.assert_allclose(got[2], far, rtol=1e-6)


def test_order_does_not_change_a_query(renderer):
    """A query adds its photons in ascending kd order whatever else is in its chunk: shuffled
    queries return bit-identical results, and so does the same call made twice."""
    filt, r, spec = CASES[1]
    ph = big_map()
    q = synth.queries(1000, seed=3, k=ALL, r=r, filt=filt, spec=spec)
    a = estimate(renderer, ph, q)
    b = estimate(renderer, ph, q)
    perm = np.random.default_rng(17).permutation(len(q))
    c = estimate(renderer, ph, q[perm])
    assert a[1].max() > 64
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes()
        assert x[perm].tobytes() == z.tobytes()


BASE = ["-resolution", "16", "16", "-aa", "0", "-global", "20000", "-caustic", "20000",
        "-it", "4", "-tt", "2", "-st", "2", "-seed", "5"]
RENDERS = {
    "cornell": ("cornell.scn", BASE + ["-gs", "1000000000", "-gd", "0.1", "-cs", "1000000000",
                                       "-cd", "0.05"]),
    "jensen": ("jensen.scn", BASE + ["-lt", "4", "-ss", "4", "-gs", "1000000000", "-cs",
                                     "1000000000", "-gf", "cone", "1.25", "-cf", "gauss",
                                     "-gd", "0.3", "-cd", "0.1"]),
}


def render_gpu(renderer, args):
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(args)
    renderer.set_params(p)
    renderer.ReadScene(sc, real)
    pst = renderer.MapPhotons()
    rgb, f, st = renderer.RenderImage(aa, w, h, want_float=True)
    return rgb, f, st, pst


@pytest.mark.parametrize("name", sorted(RENDERS))
def test_render_matches_oracle(name):
    sc, flags = RENDERS[name]
    args = [scene(sc), "/tmp/range.png"] + flags
    r = gi_amd.Renderer(0)
    try:
        rgb, f, st, pst = render_gpu(r, args)
        if name == "cornell":
            i = args.index("-gs")
            rgb50, f50, st50, _ = render_gpu(r, args[:i + 1] + ["50"] + args[i + 2:])
    finally:
        r.close()
    ref, ost = oracle_lib.render(args, 16, 16)
    reff, ref8 = oracle_lib.render_float(args, 16, 16)
    assert (ref8 == ref).all()
    print("kinds", st["knn_map_kind"], "queries", st["knn_map_queries"], "photons",
          st["knn_map_photons"], "stored", pst["global_stored"], pst["caustic_stored"])
    assert pst["global_stored"] == ost["global_stored"]
    assert pst["caustic_stored"] == ost["caustic_stored"]
    diff = {k: (st[k], int(ost[k])) for k in COUNTERS if st[k] != int(ost[k])}
    compare_exact(rgb, ref)
    compare_float_ulp(f, reff)
    assert not diff, diff
    assert st["knn_map_kind"] == [10, 10]
    assert st["knn_queries"] > 0 and st["knn_photons"] > 0
    if name == "cornell":
        assert st50["knn_map_kind"][0] == 7
        assert not np.array_equal(f, f50)
