"""The k-NN kind a render's launches run with (gi_host.cpp knn_kind, reported per map as
gi_render_stats::knn_map_kind): the automatic choice by estimate size and mode, and what becomes
of a GI_KNN_KERNEL override that cannot serve the launch. Kinds: 7 lane-select chunk kernel
(K <= 64), 8 large-K chunk kernel (K > 64, needs the per-photon dk bounds), 3 per-lane kernel
with LDS heaps (K * 512 bytes <= 64 KiB), 1 query per wave (K + 64 <= 1024), 0 per-lane kernel
with global-memory heaps, 9 the cached-radiance lookup (-cache, global map only)."""
import pytest

from gpu_util import run_gpu, scene
from test_gpu_knn_variants import make_renderer

pytestmark = pytest.mark.gpu

# (environment, extra arguments, kind of the global map's launches, kind of the caustic map's:
# its estimate size stays at the default, 225)
CASES = [
    ({}, ["-gs", "50"], 7, 8),
    ({}, ["-gs", "225"], 8, 8),
    ({"GI_KNN_KERNEL": "7"}, ["-gs", "225"], 8, 8),    # K > 64: the override cannot serve
    ({"GI_KNN_KERNEL": "8"}, ["-gs", "50"], 8, 8),     # the large-K kernel serves any K <= 960
    ({"GI_KNN_DK": "0"}, ["-gs", "225"], 1, 1),        # no dk bounds: query per wave
    ({"GI_KNN_KERNEL": "3"}, ["-gs", "225"], 8, 8),    # K * 512 > 64 KiB of LDS
    ({"GI_KNN_KERNEL": "1"}, ["-gs", "1000"], 0, 1),   # K + 64 > 1024
    ({}, ["-cache"], 9, 8),
]


@pytest.mark.parametrize("env,extra,kind0,kind1", CASES,
                         ids=["-".join([f"{k[3:]}{v}" for k, v in c[0].items()] + ["".join(c[1]).lstrip("-")])
                              for c in CASES])
def test_knn_kind(env, extra, kind0, kind1):
    args = [scene("cornell.scn"), "/tmp/x.png", "-resolution", "16", "16", "-aa", "0", "-it", "8",
            "-tt", "4", "-st", "4", "-lt", "4", "-ss", "4", "-seed", "2",
            "-global", "5000", "-caustic", "5000"] + extra
    r = make_renderer(env)
    try:
        _, st, pst = run_gpu(r, args)
    finally:
        r.close()
    print("kinds", st["knn_map_kind"], "queries", st["knn_map_queries"],
          "stored", pst["global_stored"], pst["caustic_stored"])
    assert pst["global_stored"] > 0
    assert st["knn_map_kind"][0] == kind0
    # the caustic map's launches exist only where caustic photons were stored and queried
    if pst["caustic_stored"] > 0 and st["knn_map_queries"][1] > 0:
        assert st["knn_map_kind"][1] == kind1
