"""The radiance estimate's bits, per k-NN kernel: the raw bytes of EstimateRadiance's three
outputs (out, out_n, out_maxd2) hashed and compared with tests/golden/estimate_bits.json.

The estimate (csrc/gi_estimate.h) is shared by every k-NN kernel; each kernel keeps its own
visiting order and reduction, so each has its own bits, and a change to the shared code must
change none of them. The oracle comparisons elsewhere allow rtol 1e-10: they would not notice a
re-association. The golden file was recorded from the library as it was before the estimate
was defined once (tools/record_estimate_bits.py writes it; re-record only with a change that
is meant to alter the bits, and say so).

Query sets (K, r and the filter set per case):
  spec       512 scattered queries, materials with a specular term (the general term with pow)
  diff       512 scattered queries, no specular term (the disk / diffuse-only term)
  clustered  2,048 dense queries on one face in Morton order (the chunk kernels serve them
             themselves); runs of 96 alternate between specular and
             diffuse-only materials, so 64-query chunks are all-specular, all-diffuse (the chunk
             kernels' shared-term path under the disk filter) or mixed
The irradiance branch and the cached lookup: the float image of test_gpu_knn_kind.py's 16x16
cornell render with -cache."""
import hashlib
import json
import os

import numpy as np
import pytest

import gi_amd
import synth
from gi_amd import GLOBAL, DISK, CONE, GAUSS
from gpu_util import run_gpu, scene

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "estimate_bits.json")
FILTERS = {"disk": DISK, "cone": CONE, "gauss": GAUSS}
N_PHOTONS, N_SCATTERED, N_CLUSTERED = 20000, 512, 2048


def _cases():
    out = []
    for kind in (0, 1, 3, 7, 8):
        for f in FILTERS:
            for r in (2.5, 0.05):  # the small radius: num < K
                out.append((f"kind{kind}-{f}-K50-r{r}", {"GI_KNN_KERNEL": str(kind)}, f, 50, r))
    for kind in (0, 1, 8):
        for f in FILTERS:
            out.append((f"kind{kind}-{f}-K225-r0.225", {"GI_KNN_KERNEL": str(kind)}, f, 225, 0.225))
    # the lane-select chunk kernel again: shared terms off, general instances only, per-lane
    # kernel as the last fallback
    for tag, extra in (("dbg256", {"GI_KNN_DBG": "256"}), ("general1", {"GI_KNN_GENERAL": "1"}),
                       ("fbwave0", {"GI_FB_WAVE": "0"})):
        for f in FILTERS:
            out.append((f"kind7-{tag}-{f}-K50-r2.5", dict({"GI_KNN_KERNEL": "7"}, **extra), f, 50, 2.5))
    return out


CASES = _cases()
CACHE_ID = "cornell16-cache-float-image"


def make_renderer(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return gi_amd.Renderer(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def query_sets(k, r, filt):
    cl = synth.clustered_queries(N_CLUSTERED, 17, k, r, filt)
    # in Morton order over the face, as the render's queries are: 64 consecutive ones then lie
    # close enough together for a chunk's photons to fit its LDS (unsorted, every chunk
    # overflows and the chunk kernels hand all of them to their fallback)
    g = np.clip(((cl["point"][:, [0, 2]] - [0.4, 0.5]) / 0.2 * 1024).astype(np.int64), 0, 1023)
    key = np.zeros(N_CLUSTERED, dtype=np.int64)
    for b in range(10):
        key |= ((g[:, 0] >> b) & 1) << (2 * b) | ((g[:, 1] >> b) & 1) << (2 * b + 1)
    cl = cl[np.argsort(key, kind="stable")]
    cl["ks"][(np.arange(N_CLUSTERED) // 96) % 2 == 1] = 0.0
    return {"spec": synth.queries(N_SCATTERED, seed=5, k=k, r=r, filt=filt, spec=True),
            "diff": synth.queries(N_SCATTERED, seed=7, k=k, r=r, filt=filt, spec=False),
            "clustered": cl}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def case_bits(env, fname, k, r, photons):
    """{query set: {"out", "out_n", "out_maxd2": SHA-256 of the raw bytes, "sum": fp64 sum of out}}"""
    filt = FILTERS[fname]
    r_ = make_renderer(env)
    try:
        p = gi_amd.default_params()
        p.filter_const_k = 1.25 if filt == CONE else 1.0
        r_.set_params(p)
        r_.set_photon_map(GLOBAL, photons)
        got = {}
        for name, q in query_sets(k, r, filt).items():
            g, gn, gm = r_.EstimateRadiance(GLOBAL, q)
            got[name] = {"out": sha(g), "out_n": sha(gn), "out_maxd2": sha(gm), "sum": float(g.sum())}
    finally:
        r_.close()
    return got


def cache_bits():
    args = [scene("cornell.scn"), "/tmp/x.png", "-resolution", "16", "16", "-aa", "0", "-it", "8",
            "-tt", "4", "-st", "4", "-lt", "4", "-ss", "4", "-seed", "2",
            "-global", "5000", "-caustic", "5000", "-cache"]
    r_ = make_renderer({})
    try:
        _, f, st, _ = run_gpu(r_, args, want_float=True)
    finally:
        r_.close()
    assert st["knn_map_kind"][0] == 9
    f = np.asarray(f, dtype=np.float32)
    return {"image": sha(f), "sum": float(f.astype(np.float64).sum())}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def photons():
    return synth.photon_map(N_PHOTONS, seed=41)


@pytest.mark.parametrize("cid,env,fname,k,r", CASES, ids=[c[0] for c in CASES])
def test_estimate_bits(cid, env, fname, k, r, golden, photons):
    got = case_bits(env, fname, k, r, photons)
    want = golden[cid]
    for name in want:
        print(cid, name, "sum", repr(got[name]["sum"]), "golden", repr(want[name]["sum"]))
    assert sorted(got) == sorted(want)
    for name in want:
        for key in ("out", "out_n", "out_maxd2"):
            assert got[name][key] == want[name][key], (cid, name, key, got[name]["sum"], want[name]["sum"])


def test_cached_image_bits(golden):
    got = cache_bits()
    want = golden[CACHE_ID]
    print(CACHE_ID, "sum", repr(got["sum"]), "golden", repr(want["sum"]))
    assert got["image"] == want["image"], (got["sum"], want["sum"])
