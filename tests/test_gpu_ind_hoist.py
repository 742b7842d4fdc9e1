"""The indirect sample paths' hoisted values against the oracle: the RNG stream key's prefix and
the diffuse sampler's tangent that primary_shade stores per primary sample (gi_kernels.h Spawn),
the per-material query weight kd / max kd (gi_layout.h DMaterial::kd_pd) and the split kernel's
two ballot counters. The scene (ind_hoist_cases.py) has both tangent branches, a slanted
surface, back-facing primary hits, kd quotients that are inexact and a material whose event
probabilities sum above one; test_cpu_ind_hoist.py checks on the oracle that it can show an error.

- the frame, pinhole and with depth of field (the stream id then carries a lens index): 8-bit
  image and the nine counters equal the oracle's, float image within one float32 ulp;
- the scene as a ray batch with 64-bit caller ids and with the default ids, the same;
- the frame in several batches with slot-guard re-runs (GI_SLOT_LIMIT), on one device and on a
  two-entry device set: identical to the one-batch frame;
- the split kernel (GI_SPLIT_IND=1, which reads the stored values) against the one-loop kernel
  (GI_SPLIT_IND=0, which computes them per sample): identical float image and counters.
"""
import numpy as np
import pytest

import gi_amd
import ind_hoist_cases as cases
import oracle_lib
import ray_cases
from gpu_util import compare_exact, compare_float_ulp, run_gpu

pytestmark = pytest.mark.gpu

# GI_SLOT_LIMIT of the batching test. The frame has 768 primary samples with 7 or 8 indirect
# samples each: 768 base slots, 768 query slots and 12 tiles of 8 rows of 64 tiled slots, about
# 7,700 in all. At 2,500 the whole frame and its half do not fit, its quarter (about 1,900) does;
# a shard of a two-entry device set (half the pixels) is re-run once.
SLOT_LIMIT = 2500


def check_against_oracle(got, want):
    rgb, f, st = got
    ref, ref_f, ost = want
    print({k: (st[k], ost[k]) for k in oracle_lib.COUNTER_KEYS})
    ndiff = compare_float_ulp(f, ref_f)
    compare_exact(rgb, ref)
    for k in oracle_lib.COUNTER_KEYS:
        assert st[k] == ost[k], k
    return ndiff


@pytest.mark.parametrize("dof", [False, True], ids=["pinhole", "dof2"])
def test_frame_matches_oracle(renderer, dof):
    rgb, f, st, pst = run_gpu(renderer, cases.args(dof), want_float=True)
    ref, ref_f, ost = cases.oracle_frame(dof)
    assert pst["global_stored"] == ost["global_stored"]
    assert pst["caustic_stored"] == ost["caustic_stored"]
    assert st["indirect_samples"] > 0 and st["transmissive_samples"] > 0
    check_against_oracle((rgb, f, st), (ref, ref_f, ost))


@pytest.mark.parametrize("explicit", [True, False], ids=["ids", "default_ids"])
def test_ray_batch_matches_oracle(renderer, explicit):
    cases.register_ray_scene()
    name, sensor, spp = cases.RAY_SCENE, cases.RAY_SENSOR, cases.RAY_SPP
    rays, ids = ray_cases.batch(name, sensor, spp)
    assert ids.min() > 1 << 32
    want = ray_cases.oracle_batch(name, sensor, spp, explicit)
    p, sc, _o, _w, _h, _aa, real = gi_amd.ParseArgs(ray_cases.scene_args(name))
    renderer.set_params(p)
    renderer.ReadScene(sc, real)
    renderer.MapPhotons()
    got = renderer.render_rays(ray_cases.W, ray_cases.H, spp, rays, ids if explicit else None,
                               want_float=True)
    assert got[2]["indirect_samples"] > 0
    check_against_oracle(got, want)


def _frame(env, monkeypatch, devices=None):
    """(rgb8, rgbf, stats) of the pinhole frame from a context of its own under `env`."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(cases.args())
    r = gi_amd.Renderer(0, p, devices=devices)
    try:
        r.ReadScene(sc, real)
        r.MapPhotons()
        return r.RenderImage(aa, w, h, want_float=True)
    finally:
        r.close()
        for k in env:
            monkeypatch.delenv(k)


def assert_identical(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    for k in oracle_lib.COUNTER_KEYS:
        assert got[2][k] == want[2][k], k


def test_batches_and_slot_guard_reruns_are_exact(monkeypatch):
    one = _frame({}, monkeypatch)
    check_against_oracle(one, cases.oracle_frame())
    for devices in (None, [0, 0]):
        split = _frame({"GI_SLOT_LIMIT": str(SLOT_LIMIT)}, monkeypatch, devices)
        print(f"devices {devices}: {split[2]['knn_kernel_launches']:.0f} k-NN launches, one batch "
              f"{one[2]['knn_kernel_launches']:.0f}")
        assert_identical(split, one)
        # a batch launches its own k-NN kernels: more launches, more batches
        assert split[2]["knn_kernel_launches"] > one[2]["knn_kernel_launches"]


def test_split_and_one_loop_kernels_agree(monkeypatch):
    split = _frame({"GI_SPLIT_IND": "1"}, monkeypatch)
    loop = _frame({"GI_SPLIT_IND": "0"}, monkeypatch)
    assert_identical(loop, split)
    check_against_oracle(split, cases.oracle_frame())
