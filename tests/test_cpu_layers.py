"""What of the light-path layers needs no GPU: the mirror's names and signatures, the helpers of
tests/layers_ref.py on made-up samples, and the oracle's evidence that the groups are additive
(switching one contribution off does not move another's random streams)."""
import ctypes as C
import re
import os

import numpy as np

import gi_amd
import layers_ref as lr
import oracle_lib
from gpu_util import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mirror_names_follow_the_header():
    txt = open(os.path.join(ROOT, "include", "gi.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"GI_LAYER_([A-Z]+) = (\d+)", txt))
    assert enum == {"SURFACE": 0, "SPECULAR": 1, "INDIRECT": 2, "GLOBAL": 3, "CAUSTIC": 4,
                    "COUNT": 5, "TOTAL": 5}
    for name, v in enum.items():
        assert getattr(gi_amd, "LAYER_" + name) == v
        assert getattr(lr, name) == v
    assert gi_amd.LAYER_NAMES == lr.NAMES == tuple(k.lower() for k in list(enum)[:5])
    L = gi_amd.lib()
    assert L.gi_render_layers.argtypes == L.gi_render_radiance.argtypes
    assert L.gi_render_rays_layers.argtypes == L.gi_render_rays_radiance.argtypes
    assert len(L.gi_accum_add_image_layers.argtypes) == len(L.gi_accum_add_image.argtypes) + 1
    assert len(L.gi_accum_add_rays_layers.argtypes) == len(L.gi_accum_add_rays.argtypes) + 1


def test_layer_list_takes_five_entries():
    class Fake:
        _ctx = C.c_void_p(0x1000)
    arr = gi_amd.Renderer._layer_list([Fake(), None, Fake(), None, None])
    assert [bool(v) for v in arr] == [True, False, True, False, False]
    for n in (4, 6):
        try:
            gi_amd.Renderer._layer_list([None] * n)
        except ValueError:
            continue
        raise AssertionError(n)


def made_up(rng, h=3, w=4, s=2):
    smp = np.zeros((lr.COUNT + 1, h, w, s, 3))
    smp[:lr.COUNT] = rng.random((lr.COUNT, h, w, s, 3)) * (rng.random((lr.COUNT, h, w, s, 1)) < 0.5)
    for l in range(lr.COUNT):      # the total in another order than sum_ratio's
        smp[lr.TOTAL] = smp[lr.COUNT - 1 - l] + smp[lr.TOTAL]
    return smp


def test_helpers_on_made_up_samples():
    smp = made_up(np.random.default_rng(3))
    ratio, zeros = lr.sum_ratio(smp)
    assert zeros and 0.0 <= ratio <= 8 * 2.0 ** -53
    bad = smp.copy()
    bad[lr.TOTAL, 0, 0, 0, 0] = bad[lr.TOTAL, 0, 0, 0, 0] * 1.5 + 1.0
    assert lr.sum_ratio(bad)[0] > 0.3
    lost = smp.copy()
    lost[lr.TOTAL][smp[lr.CAUSTIC] != 0] = 0.0      # a term that never reached the total
    assert not lr.sum_ratio(lost)[1]
    for l in range(lr.COUNT):
        q = lr.alone(smp, l)
        others = np.delete(smp[:lr.COUNT], l, axis=0)
        assert q.shape == smp.shape[1:4]
        assert (others[:, q] == 0).all() and (others[:, ~q] != 0).any(axis=(0, -1)).all()
        # where a layer is alone the total is that layer, whatever the order of the +0 additions
        assert (smp[lr.TOTAL][q] == smp[l][q]).all()
        px = lr.alone_pixels(smp, l)
        assert px.shape == smp.shape[1:3] and px.sum() <= q.any(axis=-1).sum()
    parts = list(np.random.default_rng(5).random((lr.COUNT, 4, 8, 3), dtype=np.float32))
    want = parts[0].astype(np.float64)
    for p in parts[1:]:
        want = want + p.astype(np.float64)
    assert (lr.filtered_sum(parts) == want.astype(np.float32)).all()
    # ... which is not the float32 sum
    f32 = parts[0] + parts[1] + parts[2] + parts[3] + parts[4]
    assert lr.filtered_sum(parts).dtype == np.float32 and (lr.filtered_sum(parts) != f32).any()


def test_accum_state_is_the_restatement_fold():
    import accum_state_ref as asr
    import radiance_ref as rr
    rng = np.random.default_rng(4)
    a, b = rng.random((2, 3, 4, 3)), rng.random((2, 3, 5, 3))
    state, counts = lr.accum_state([(a, 1.0 / 4), (b, 1.0 / 5)])
    assert state.shape == (2, 3, 6) and (counts == 9).all()
    sa = np.concatenate(rr.pass_stats(a, 1.0 / 4), axis=-1)
    sb = np.concatenate(rr.pass_stats(b, 1.0 / 5), axis=-1)
    ref = asr.fold(sa, np.full((2, 3), 4), sb, np.full((2, 3), 5))
    assert (state == ref[0]).all() and (counts == ref[1]).all()


def test_oracle_contributions_are_additive():
    """cornell.scn at 24 x 16, aa 0, -it 4, without direct and ambient light: the caustic
    contribution taken as (all) - (-no_caustic) and as (-no_indirect) - (-no_indirect
    -no_caustic) agrees within float32 rounding of the oracle's output on every pixel that no
    render clamps, so a layer does not depend on which other layers are switched on."""
    base = [scene("cornell.scn"), "/tmp/x.png", "-resolution", "24", "16", "-aa", "0", "-global",
            "20000", "-caustic", "20000", "-it", "4", "-tt", "8", "-st", "8", "-seed", "5",
            "-no_direct", "-no_ambient"]
    f = {k: oracle_lib.render_float(base + list(k), 24, 16)[0].astype(np.float64)
         for k in [(), ("-no_caustic",), ("-no_indirect",), ("-no_indirect", "-no_caustic")]}
    free = np.all([v < 1.0 for v in f.values()], axis=0)
    d1 = f[()] - f[("-no_caustic",)]
    d2 = f[("-no_indirect",)] - f[("-no_indirect", "-no_caustic")]
    err = float(np.abs(d1 - d2)[free].max())
    print(f"{free.mean():.3f} of the values unclamped, caustic contribution up to {d2[free].max():.3f}, "
          f"largest disagreement {err:.2e}")
    assert free.mean() > 0.5 and d2[free].max() > 0.01
    # four float32 roundings of values below 1: 4 * 2^-25
    assert err <= 4 * 2.0 ** -25
