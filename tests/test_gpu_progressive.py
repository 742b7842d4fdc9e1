"""Progressive photon-map passes (gi.h gi_accum_add_progressive): pass p is, bit for bit, the
sequence set_params(Q_p) -> map_photons -> accum_add_image -> set_params(P) with Q_p = P under
seed + p, estimate sizes no map reaches and the radii of tests/progressive_ref.py; its maps and
counters are those of the oracle's render under the same flags."""
import ctypes as C

import pytest

import gi_amd
import oracle_lib
import progressive_ref as pref
from gi_amd import CAUSTIC, GLOBAL
from gpu_util import scene

pytestmark = pytest.mark.gpu

W, H, AA = 24, 16, 1
SEED, R0G, R0C, ALPHA = 5, 0.1, 0.05, 0.7
FLAGS = ["-resolution", str(W), str(H), "-aa", str(AA), "-global", "20000", "-caustic", "20000",
         "-it", "4", "-tt", "2", "-st", "2"]
ARGS = [scene("cornell.scn"), "/tmp/prog.png"] + FLAGS + ["-seed", str(SEED), "-gd", repr(R0G),
                                                         "-cd", repr(R0C)]


def open_renderer(reset=True):
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(ARGS)
    assert (w, h, aa) == (W, H, AA)
    r = gi_amd.Renderer(0, p)
    r.ReadScene(sc, real)
    if reset:
        r.accum_reset(W, H)
    return r


def copy_params(p):
    q = gi_amd.GiParams()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(p))
    return q


def state_bytes(r):
    s, c = r.accum_export()
    return s.tobytes() + c.tobytes()


def test_same_bits_as_the_manual_sequence():
    a, b = open_renderer(), open_renderer()
    try:
        before = bytes(a.params)
        P = copy_params(b.params)
        for p in range(3):
            pst_a, st_a = a.accum_add_progressive(AA, p, alpha=ALPHA)
            Q = copy_params(P)
            Q.seed = P.seed + p
            Q.global_estimate_size = Q.caustic_estimate_size = gi_amd.GI_ESTIMATE_ALL
            Q.global_estimate_dist = pref.radius(R0G, ALPHA, p)
            Q.caustic_estimate_dist = pref.radius(R0C, ALPHA, p)
            b.set_params(Q)
            pst_b = b.MapPhotons()
            st_b = b.accum_add_image(AA)
            b.set_params(copy_params(P))
            assert state_bytes(a) == state_bytes(b), p
            assert st_a["knn_map_kind"] == [10, 10] and st_b["knn_map_kind"] == [10, 10]
            for k in ("global_stored", "caustic_stored", "global_emitted", "caustic_emitted"):
                assert pst_a[k] == pst_b[k], (p, k)
            for k in ("knn_queries", "knn_photons", "screen_rays", "shadow_rays"):
                assert st_a[k] == st_b[k], (p, k)
            assert a.photon_map(GLOBAL).tobytes() == b.photon_map(GLOBAL).tobytes()
        assert bytes(a.params) == before
        # the context's own parameters are back: a plain pass under them (the maps stay pass 2's)
        # equals the one of the context that set them by hand
        a.accum_add_image(AA)
        b.accum_add_image(AA)
        assert state_bytes(a) == state_bytes(b)
        # explicit radii equal the context's, and a pass is not the fixed-map pass
        c = open_renderer()
        try:
            c.accum_add_progressive(AA, 0, alpha=ALPHA, global_radius=R0G, caustic_radius=R0C)
            d = open_renderer()
            try:
                d.accum_add_progressive(AA, 0)   # defaults: alpha 0.7, the context's radii
                assert state_bytes(c) == state_bytes(d)
                d.accum_reset(W, H)
                d.accum_add_image(AA)            # the maps of pass 0, K = 50 / 225 estimates
                assert state_bytes(c) != state_bytes(d)
            finally:
                d.close()
        finally:
            c.close()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("p", [0, 1, 2])
def test_pass_counters_and_maps_match_oracle(p):
    args = ARGS[:2] + FLAGS + pref.pass_args(SEED, p, R0G, R0C, ALPHA)
    r = open_renderer()
    try:
        pst, st = r.accum_add_progressive(AA, p, alpha=ALPHA)
        g, c = r.photon_map(GLOBAL), r.photon_map(CAUSTIC)
    finally:
        r.close()
    _rgb, ost = oracle_lib.render(args, W, H)
    og, oc, _em = oracle_lib.map_photons(args)
    print("pass", p, "queries", st["knn_queries"], "photons", st["knn_photons"], "stored",
          pst["global_stored"], pst["caustic_stored"])
    assert st["knn_queries"] == int(ost["knn_queries"])
    assert st["knn_photons"] == int(ost["knn_photons"])
    assert pst["global_stored"] == int(ost["global_stored"]) == len(og)
    assert pst["caustic_stored"] == int(ost["caustic_stored"]) == len(oc)
    assert g.tobytes() == og.tobytes()
    assert c.tobytes() == oc.tobytes()
    assert st["knn_map_kind"] == [10, 10]


def test_error_codes_leave_the_state_unchanged():
    L = gi_amd.lib()
    ARG, STATE, UNSUP = gi_amd.GI_ERR_ARG, gi_amd.GI_ERR_STATE, gi_amd.GI_ERR_UNSUPPORTED

    def call(r, p=0, aa=AA, **kw):
        pp = gi_amd.progressive_params(**kw)
        return L.gi_accum_add_progressive(r._ctx, aa, p, C.byref(pp), None, None)

    assert L.gi_accum_add_progressive(None, AA, 0, None, None, None) == ARG
    r = gi_amd.Renderer(0)
    try:   # before a scene (with and without an accumulator)
        assert call(r) == STATE
        r.accum_reset(W, H)
        assert call(r) == STATE
    finally:
        r.close()
    r = open_renderer(reset=False)
    try:   # before a reset
        assert call(r) == STATE
        r.accum_reset(W, H)
        r.accum_add_progressive(AA, 0, alpha=ALPHA)
        held = state_bytes(r)
        maps = r.photon_map(GLOBAL).tobytes()
        bad = [dict(alpha=0.0), dict(alpha=1.0), dict(alpha=float("nan")), dict(alpha=-0.5),
               dict(global_radius=-1.0), dict(caustic_radius=float("inf")),
               dict(global_radius=float("nan"))]
        for kw in bad:
            assert call(r, **kw) == ARG, kw
        assert call(r, p=-1) == ARG
        assert call(r, p=1 << 20) == ARG
        assert call(r, aa=-1) == ARG
        # refused calls changed nothing: neither the accumulator nor the maps
        assert state_bytes(r) == held and r.photon_map(GLOBAL).tobytes() == maps
        P = copy_params(r.params)
        P.irradiance_cache = 1
        r.set_params(P)
        assert call(r) == ARG
        P.irradiance_cache = 0
        P.global_estimate_dist = 0.0   # no r_0 anywhere
        r.set_params(P)
        assert call(r) == ARG
        assert state_bytes(r) == held and r.photon_map(GLOBAL).tobytes() == maps
        assert call(r, global_radius=R0G) == gi_amd.GI_OK
        assert state_bytes(r) != held
    finally:
        r.close()
    r = gi_amd.Renderer(devices=[0, 0])
    try:
        assert call(r) == UNSUP
    finally:
        r.close()
