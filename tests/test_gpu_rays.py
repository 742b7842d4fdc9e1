"""gi_camera_rays and gi_render_rays against the oracle's own entries (oracle_camera_rays,
oracle_render_rays: written from render.cpp and gi.h's text, not from the device code).

- exported camera rays and stream ids equal the oracle's bit for bit: odd frame sizes, a set
  camera, depth of field (the lens draws), and a frame just over gi_camera_rays' 2^22-sample
  chunk;
- ray batches of three sensors that are no pinhole camera (ray_cases.py: orthographic,
  light-field slice, panorama) on three scenes at spp 1, 3 and 5, with 64-bit stream ids and
  with the default ids: 8-bit image and the nine counters equal, float image within one float32
  ulp. Every ray of the orthographic and light-field batches has its own origin, so a hit shaded
  from the camera's eye shows (test_cpu_rays.py measures by how much);
- the same across batches, slot-guard re-runs and the tile shards of a device set.
"""
import numpy as np
import pytest

import gi_amd
import oracle_lib
import ray_cases
from camera_cases import CASES, CORNELL_FLAGS, camera_of, rewrite_scene
from gpu_util import compare_exact, compare_float_ulp, scene

pytestmark = pytest.mark.gpu


def load(renderer, args, maps=True):
    """ParseArgs -> ReadScene (-> MapPhotons) on the shared renderer; returns (aa, w, h)."""
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(args)
    renderer.set_params(p)
    renderer.ReadScene(sc, real)
    if maps and (p.indirect_illum or p.caustic_illum or p.direct_photon_illum):
        renderer.MapPhotons()
    return aa, w, h


def cornell(width, height, aa):
    f = list(CORNELL_FLAGS)
    i = f.index("-resolution")
    f[i + 1], f[i + 2] = str(width), str(height)
    f[f.index("-aa") + 1] = str(aa)
    return f


def assert_same_bits(rays, ids, want_rays, want_ids):
    assert len(rays) == len(want_rays) and len(ids) == len(want_ids)
    np.testing.assert_array_equal(ids, want_ids)
    got = np.ascontiguousarray(rays).view(np.float64).reshape(-1, 6)
    want = np.ascontiguousarray(want_rays).view(np.float64).reshape(-1, 6)
    if not (got.view(np.uint64) == want.view(np.uint64)).all():
        bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        print("rays that differ:", len(np.unique(bad[:, 0])), "of", len(got), "first", bad[:4].tolist(),
              "max abs", float(np.abs(got - want).max()))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))


CAMERA_CASES = {
    "cornell_24x16_aa1": ("cornell.scn", cornell(24, 16, 1), None),
    "cornell_view_37x21_aa2": ("cornell.scn", cornell(37, 21, 2), CASES["cornell"][1]),
    "cornell_5x3_aa0": ("cornell.scn", cornell(5, 3, 0), None),
    "teapot_dof_16x16_aa1": ("teapot.scn", ["-resolution", "16", "16", "-aa", "1", "-dof", "4",
                                            "12.2282", "0.025", "-seed", "6"], None),
    # 4,222,512 samples: the second chunk of gi_camera_rays holds 28,208 of them
    "cornell_531x497_aa2_chunk": ("cornell.scn", cornell(531, 497, 2), None),
}


@pytest.mark.parametrize("case", list(CAMERA_CASES))
def test_camera_rays_equal_the_oracles(renderer, case, tmp_path):
    scn, flags, cam = CAMERA_CASES[case]
    aa, w, h = load(renderer, [scene(scn), "/tmp/x.png"] + flags, maps=False)
    path = scene(scn)
    if cam is not None:
        renderer.set_camera(*camera_of(cam))
        path = rewrite_scene(scene(scn), cam, tmp_path)
    rays, ids = renderer.camera_rays(aa, w, h)
    want_rays, want_ids = oracle_lib.camera_rays([path, "/tmp/x.png"] + flags)
    assert len(rays) == w * h * 4 ** aa * renderer.params.dof_test
    assert_same_bits(rays, ids, want_rays, want_ids)


def check_against_oracle(got, want):
    """(rgb8, rgbf, stats) of the device against the oracle's: 8-bit image and the nine counters
    equal, float image within one float32 ulp. Returns the number of float values that differ."""
    rgb, f, st = got
    ref, ref_f, ost = want
    print({k: (st[k], ost[k]) for k in oracle_lib.COUNTER_KEYS})
    ndiff = compare_float_ulp(f, ref_f)
    compare_exact(rgb, ref)
    for k in oracle_lib.COUNTER_KEYS:
        assert st[k] == ost[k], k
    return ndiff


RENDER_CASES = [b + (True,) for b in ray_cases.BATCHES] + [b + (False,)
                                                           for b in ray_cases.DEFAULT_ID_BATCHES]


@pytest.mark.parametrize("name,sensor,spp,explicit", RENDER_CASES,
                         ids=["-".join([n, s, f"spp{k}", "ids" if e else "default_ids"])
                              for n, s, k, e in RENDER_CASES])
def test_render_rays_matches_oracle(renderer, name, sensor, spp, explicit):
    rays, ids = ray_cases.batch(name, sensor, spp)
    want = ray_cases.oracle_batch(name, sensor, spp, explicit)
    load(renderer, ray_cases.scene_args(name))
    got = renderer.render_rays(ray_cases.W, ray_cases.H, spp, rays, ids if explicit else None,
                               want_float=True)
    ndiff = check_against_oracle(got, want)
    print(f"{name} {sensor} spp {spp} {'explicit' if explicit else 'default'} ids: "
          f"{ndiff} float values differ by one ulp")


def test_render_rays_across_batches_and_shards(monkeypatch):
    """GI_SLOT_LIMIT (path slots per batch) at 60000, and at 9000: this frame's 2331 primaries
    need about 33,000 slots (5 paths and 8 tiled indirect entries each), so that at 9000 the slot
    guard re-runs the batch smaller until it is split. The primary cap of a batch is far above
    2331 samples, so more than one batch can only come from those re-runs; a batch launches its
    own k-NN kernels, which the launch counter shows."""
    name, sensor, spp, w, h = ray_cases.TILED_BATCH
    rays, ids = ray_cases.batch(name, sensor, spp, w, h)
    args = ray_cases.scene_args(name, w, h)
    p, sc, _o, _w, _h, _aa, real = gi_amd.ParseArgs(args)
    floats, launches = {}, {}
    for slot_limit in (60000, 9000):
        monkeypatch.setenv("GI_SLOT_LIMIT", str(slot_limit))
        for devices in (None, [0, 0]):
            r = gi_amd.Renderer(0, p, devices=devices)
            try:
                r.ReadScene(sc, real)
                r.MapPhotons()
                for explicit in (True, False):
                    got = r.render_rays(w, h, spp, rays, ids if explicit else None,
                                        want_float=True)
                    key = (slot_limit, devices is None, explicit)
                    launches[key] = got[2]["knn_kernel_launches"]
                    ndiff = check_against_oracle(
                        got, ray_cases.oracle_batch(name, sensor, spp, explicit, w, h))
                    print(f"limit {slot_limit} devices {devices} explicit ids {explicit}: "
                          f"{launches[key]:.0f} k-NN launches, {ndiff} float values differ by "
                          "one ulp")
                    floats[key] = got[1]
            finally:
                r.close()
    for slot_limit in (60000, 9000):
        for explicit in (True, False):
            np.testing.assert_array_equal(floats[(slot_limit, True, explicit)],
                                          floats[(slot_limit, False, explicit)])
    for one_device in (True, False):
        for explicit in (True, False):
            assert launches[(9000, one_device, explicit)] > launches[(60000, one_device, explicit)]
