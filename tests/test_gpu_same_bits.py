"""One seed renders to the same bits every time (DESIGN.md "Accumulator state", "Renders of one
seed have the same bits"). A chunk's queries share their photon visits, so a query's last bit
depends on which queries it is chunked with; the chunk k-NN's hand-on lists and the launch order
of the Monte Carlo appends used to follow the arrival of atomics, and the same frame then visited
one of two photon counts and moved single samples by one fp64 ulp from launch to launch. Six
renders of cornell.scn (CORNELL_FLAGS, seed 7: glass and mirror pixels append queries, and every
global query goes through the second chunk pass) in one context, and the first render of a second
context, must agree in every sample bit and in the photons each map's k-NN visited."""
import numpy as np
import pytest

import gi_amd
from camera_cases import CORNELL_FLAGS
from gpu_util import scene

pytestmark = pytest.mark.gpu

ARGS = [scene("cornell.scn"), "/tmp/x.png"] + CORNELL_FLAGS
COUNTERS = ("knn_map_queries", "knn_map_photons", "knn_map_visited", "knn_map_pass2_queries",
            "knn_map_fallback_queries", "monte_carlo_rays")


def renders(r, n):
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(ARGS)
    r.set_params(p)
    r.ReadScene(sc, real)
    r.MapPhotons()
    p.seed = 7
    r.set_params(p)
    out = []
    for _ in range(n):
        _mean, _var, smp, st = r.render_radiance(aa, w, h, want_samples=True)
        out.append((smp, {k: st[k] for k in COUNTERS}))
    return out


def test_renders_of_one_seed_have_the_same_bits(renderer):
    runs = renders(renderer, 6)
    second = gi_amd.Renderer(0)
    try:
        runs += renders(second, 1)     # a context's first render: cold buffers, other timing
    finally:
        second.close()
    smp0, st0 = runs[0]
    print("counters:", st0)
    # the fixture exercises both places: appended queries and a second chunk pass
    assert st0["monte_carlo_rays"] > 0 and st0["knn_map_pass2_queries"][0] > 0
    for i, (smp, st) in enumerate(runs[1:], 1):
        nd = int((smp.view(np.uint64) != smp0.view(np.uint64)).sum())
        print(f"render {i}: {nd} of {smp.size} sample values differ, visited {st['knn_map_visited']}")
        assert st == st0, (i, st, st0)
        assert nd == 0, (i, np.argwhere(smp.view(np.uint64) != smp0.view(np.uint64))[:4].tolist())
