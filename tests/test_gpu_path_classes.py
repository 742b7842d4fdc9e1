"""The Monte Carlo path schedules on the element sets and lights that cornell.scn and jensen.scn
(triangles and spheres) do not reach: the host picks a path kernel's instance from the scene's
element kinds and from whether its lights are all hard, so the forced-schedule instances for
boxes / meshes (KINDS_POLY) and for every element kind (KINDS_ALL), with hard and with soft
lights, run only on scenes such as path_class_cases' four rooms.

For each room the frames under one path per lane (GI_MC_PERSIST=0, GI_MC_WAVE=0), breadth first
with every later bounce in the tail (GI_MC_WAVE=1), breadth first with rounds (GI_MC_WAVE=3) and
the persistent kernel (GI_MC_PERSIST=3) are identical: float image, 8-bit image and the eight
counters. The first of them equals the oracle's frame (8-bit image and counters; float image
within one float32 ulp). test_cpu_path_classes.py checks on the oracle that the rooms have the
paths this needs.

One replay for the ray-batch (RAYS) instances: on `all`, the camera's own rays rendered as a ray
batch under GI_MC_WAVE=3 give the camera frame bit for bit.
"""
import numpy as np
import pytest

import gi_amd
import oracle_lib
import path_class_cases as cases
from gpu_util import compare_exact, compare_float_ulp
from mc_wave_cases import COUNTERS

pytestmark = pytest.mark.gpu

# (GI_MC_PERSIST, GI_MC_WAVE); the first is the reference
SCHEDULES = (("0", "0"), ("0", "1"), ("0", "3"), ("3", "0"))


def context(monkeypatch, name, persist, wave):
    """A context of its own (the switches are read when it is made) with the scene and maps."""
    monkeypatch.setenv("GI_MC_PERSIST", persist)
    monkeypatch.setenv("GI_MC_WAVE", wave)
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(cases.args(name))
    r = gi_amd.Renderer(0, p)
    try:
        r.ReadScene(sc, real)
        r.MapPhotons()
    except Exception:
        r.close()
        raise
    return r, (aa, w, h)


def frame(monkeypatch, name, persist, wave):
    r, (aa, w, h) = context(monkeypatch, name, persist, wave)
    try:
        return r.RenderImage(aa, w, h, want_float=True)
    finally:
        r.close()


def assert_identical(got, want):
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0], want[0])
    for k in COUNTERS:
        assert got[2][k] == want[2][k], k


@pytest.mark.parametrize("name", cases.SCENES)
def test_schedules_agree_and_match_oracle(monkeypatch, name):
    base = frame(monkeypatch, name, *SCHEDULES[0])
    rgb, f, st = base
    ref, ref_f, ost = cases.oracle_frame(name)
    print({k: (st[k], ost[k]) for k in oracle_lib.COUNTER_KEYS})
    assert st["transmissive_samples"] > 0 and st["specular_samples"] > 0
    compare_float_ulp(f, ref_f)
    compare_exact(rgb, ref)
    for k in oracle_lib.COUNTER_KEYS:
        assert st[k] == ost[k], k
    for persist, wave in SCHEDULES[1:]:
        assert_identical(frame(monkeypatch, name, persist, wave), base)


def test_camera_rays_replay_under_rounds(monkeypatch):
    r, (aa, w, h) = context(monkeypatch, "all", "0", "3")
    try:
        want = r.RenderImage(aa, w, h, want_float=True)
        rays, ids = r.camera_rays(aa, w, h)
        spp = (aa + 1) ** 2
        assert len(rays) == len(ids) == w * h * spp
        got = r.render_rays(w, h, spp, rays, ids, want_float=True)
    finally:
        r.close()
    assert want[2]["transmissive_samples"] > 0 and want[2]["specular_samples"] > 0
    assert_identical(got, want)
