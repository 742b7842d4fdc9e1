"""The breadth-first Monte Carlo schedule (GI_MC_WAVE = R: mc_wave_begin_kernel, R - 1
single-bounce launches of mc_wave_step_kernel over the compacted live list, one tail launch)
against one path per lane (mc_kernel, GI_MC_WAVE=0). A path's arithmetic, RNG stream, query keys,
base slot and queue stripe depend on its index alone, so the float frame and the -v counters are
identical, not close:

- R = 1 (every bounce after the first in the tail), 3 (rounds and tail) and 200 (the tail finds
  an empty list) on a hard-light and a soft-light frame, plain and with the sub-paths skipping
  mc_sub_kernel (GI_MC_SUB=0), with the depth cap inside the begin kernel (-md 1) and inside the
  rounds (-md 3), and with the batch re-run after a continuation queue overflow (GI_IND_FRAC),
  which has to reset the lists and counters; test_cpu_mc_wave.py checks on the oracle that the
  frames' paths have the lengths this needs. The renderer reports no re-run count, so that
  variant rests on the premise of test_gpu_render.py's test_indirect_continuation_queue_is_exact,
  whose frames and GI_IND_FRAC these are: at that fraction a stripe of the indirect continuation
  queue holds 64 entries (2,048 tiled entries per stripe, times 0.00001, rounded up to one row),
  which the frames' 114,000 indirect samples overflow if more than 3.6 % of them hit the glass
  or the mirror sphere (an estimate, not asserted here);
- one run of each frame against the oracle: 8-bit image and counters equal, float image within one
  float32 ulp;
- a room without glass or mirror (no Monte Carlo path: no launch is made, no buffer sized);
- a ray batch (the RAYS instances of the begin kernel) and a packed tile shard, on a 33 x 31
  frame, so that the path counts are no multiples of 64 or 128.
"""
import numpy as np
import pytest

import gi_amd
import mc_wave_cases as cases
import oracle_lib
import ray_cases
from gpu_util import compare_exact, compare_float_ulp

pytestmark = pytest.mark.gpu

ROUNDS = ("1", "3", "200")
# name -> (environment, extra flags)
VARIANTS = {
    "plain": ({}, []),
    "mc_sub0": ({"GI_MC_SUB": "0"}, []),
    "md1": ({}, ["-md", "1"]),
    "md3": ({}, ["-md", "3"]),
    "requeue": ({"GI_IND_FRAC": "0.00001"}, []),
}


def context(monkeypatch, args, env, rounds):
    """A context of its own (the switches are read when it is made) with the scene and maps."""
    monkeypatch.setenv("GI_MC_PERSIST", "0")
    monkeypatch.setenv("GI_MC_WAVE", rounds)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(args)
    r = gi_amd.Renderer(0, p)
    try:
        r.ReadScene(sc, real)
        if p.indirect_illum or p.caustic_illum:
            r.MapPhotons()
    except Exception:
        r.close()
        raise
    return r, (aa, w, h)


def frame(monkeypatch, args, env, rounds):
    r, (aa, w, h) = context(monkeypatch, args, env, rounds)
    try:
        return r.RenderImage(aa, w, h, want_float=True)
    finally:
        r.close()


def assert_identical(got, want):
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0], want[0])
    for k in cases.COUNTERS:
        assert got[2][k] == want[2][k], k


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_rounds_equal_one_path_per_lane(monkeypatch, name, variant):
    env, extra = VARIANTS[variant]
    args = cases.args(name, extra)
    base = frame(monkeypatch, args, env, "0")
    print({k: base[2][k] for k in cases.COUNTERS})
    assert base[2]["transmissive_samples"] > 0 and base[2]["specular_samples"] > 0
    for rounds in ROUNDS:
        assert_identical(frame(monkeypatch, args, env, rounds), base)


@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_frame_matches_oracle(monkeypatch, name):
    rgb, f, st = frame(monkeypatch, cases.args(name), {}, "3")
    ref, ref_f, ost = cases.oracle_frame(name)
    print({k: (st[k], ost[k]) for k in oracle_lib.COUNTER_KEYS})
    compare_float_ulp(f, ref_f)
    compare_exact(rgb, ref)
    for k in oracle_lib.COUNTER_KEYS:
        assert st[k] == ost[k], k


def test_frame_without_monte_carlo_paths(monkeypatch):
    off = frame(monkeypatch, cases.plain_args(), {}, "0")
    on = frame(monkeypatch, cases.plain_args(), {}, "3")
    assert off[2]["transmissive_samples"] == 0 and off[2]["specular_samples"] == 0
    assert off[2]["indirect_samples"] > 0
    assert_identical(on, off)


def test_ray_batch(monkeypatch):
    name, sensor, spp, w, h = "cornell_dim", "panorama", 3, 33, 31
    rays, ids = ray_cases.batch(name, sensor, spp, w, h)
    out = []
    for rounds in ("0", "3"):
        r, _ = context(monkeypatch, ray_cases.scene_args(name, w, h), {}, rounds)
        try:
            out.append(r.render_rays(w, h, spp, rays, ids, want_float=True))
        finally:
            r.close()
    assert out[0][2]["transmissive_samples"] > 0 and out[0][2]["specular_samples"] > 0
    assert_identical(out[1], out[0])


def test_packed_tile_shard(monkeypatch):
    import torch
    w, h, tile, shard, nshards = 33, 31, 8, 1, 2
    args = cases.args("cornell", ["-resolution", str(w), str(h)])
    out = []
    for rounds in ("0", "3"):
        r, (aa, _w, _h) = context(monkeypatch, args, {}, rounds)
        try:
            n = r.shard_pixels(w, h, tile, shard, nshards)
            assert 0 < n < w * h
            buf = torch.full((n, 4), -1.0, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            npx, st = r.render_tiles_packed(aa, w, h, tile, shard, nshards, buf.data_ptr(), n)
            torch.cuda.synchronize()
            assert npx == n
            out.append((buf.cpu().numpy().view(np.uint32), st))
        finally:
            r.close()
    assert out[0][1]["transmissive_samples"] > 0
    np.testing.assert_array_equal(out[1][0], out[0][0])
    for k in cases.COUNTERS:
        assert out[1][1][k] == out[0][1][k], k
