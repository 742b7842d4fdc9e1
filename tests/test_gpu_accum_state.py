"""The accumulator's state out of its context and back (gi.h "accumulator state") on the device,
against tests/accum_state_ref.py bit for bit. Frames: cornell.scn under CORNELL_FLAGS (24 x 16,
aa 1: 4 samples per pixel and pass), maps built under seed 5, passes under seeds 5 .. 8.

1. round trip: export -> reset -> import -> export returns the same bits, and gi_accum_get too;
2. a merged pass is an added pass: a context holding seed 5 and one holding seed 6, merged through
   the host call, the packed pair and gi_accum_merge_from, equal one context that added 5 and 6;
3. accum_fold_states_kernel against the restatement on synthetic states: 851 pixels and 1 pixel,
   1, 3 and 8 states at a padded stride, empty sides, counts of 1 and near 2^40, equal means and
   means of opposite sign;
4. the accumulator works on afterwards: a whole-frame pass and an adaptive pass after an import
   equal the uninterrupted context's;
5. another association of the same four passes changes the bits only within rounding;
6. the error codes, each with the accumulator checked unchanged; a device set;
and tools/progressive_ranks.py under torchrun, two ranks on one GPU.
"""
import ctypes as C

import numpy as np
import pytest

import accum_state_ref as asr
import gi_amd
from camera_cases import CORNELL_FLAGS
from gpu_util import scene

pytestmark = pytest.mark.gpu

W, H, AA, S = 24, 16, 1, 4
CORNELL_ARGS = [scene("cornell.scn"), "/tmp/x.png"] + CORNELL_FLAGS


def same_bits(dev, ref, what=""):
    dev, ref = np.ascontiguousarray(dev), np.ascontiguousarray(ref)
    assert dev.dtype == ref.dtype and dev.shape == ref.shape, (what, dev.dtype, ref.dtype,
                                                                dev.shape, ref.shape)
    u = {4: np.uint32, 8: np.uint64, 1: np.uint8}[dev.dtype.itemsize]
    bad = dev.view(u) != ref.view(u)
    print(f"{what}: {int(bad.sum())} of {dev.size} values differ")
    assert not bad.any(), (what, np.argwhere(bad)[:8].tolist())


def same_state(got, ref, what):
    same_bits(got[0], ref[0], what + " state")
    same_bits(got[1], ref[1], what + " counts")


def load(r):
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(CORNELL_ARGS)
    assert (w, h, aa, p.seed) == (W, H, AA, 5)
    r.set_params(p)
    r.ReadScene(sc, real)
    r.MapPhotons()
    return p


def add_passes(r, p, seeds, reset=True):
    """(state, counts) after each pass of the sequence; the maps stay those of seed 5."""
    out = []
    if reset:
        r.accum_reset(W, H)
    for seed in seeds:
        p.seed = seed
        r.set_params(p)
        r.accum_add_image(AA)
        out.append(r.accum_export())
    p.seed = 5
    r.set_params(p)
    return out


@pytest.fixture(scope="module")
def other():
    """A second context on the same device: the same scene, its maps built under seed 5."""
    r = gi_amd.Renderer(0)
    r.p = load(r)
    yield r
    r.close()


@pytest.fixture(scope="module")
def frames(renderer):
    """States of one context after the passes 5; 5, 6; 5, 6, 7; 5 .. 8 (keys: the seeds) and after
    7, 8 alone. Shared: do not modify."""
    p = load(renderer)
    seeds = (5, 6, 7, 8)
    out = {seeds[:k + 1]: st for k, st in enumerate(add_passes(renderer, p, seeds))}
    out[(7, 8)] = add_passes(renderer, p, (7, 8))[-1]
    for st in out.values():
        for a in st:
            a.setflags(write=False)
    renderer.p = p
    return out


def device_bytes(raw):
    """A device tensor holding the bytes, complete before the library reads it."""
    import torch
    t = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


# ---- 1. round trip -----------------------------------------------------------------------------
def test_export_reset_import_round_trip(renderer, frames):
    add_passes(renderer, renderer.p, (5, 6))
    st = renderer.accum_export()
    same_state(st, frames[(5, 6)], "two passes again")
    got = renderer.accum_get()
    counts, total = renderer.accum_get_counts()
    same_bits(st[1], counts, "exported counts")
    assert total == W * H * 2 * S and (counts == 2 * S).all()
    assert st[0][..., 3:].min() >= 0.0 and st[0][..., 3:].max() > 0.0
    renderer.accum_reset(W, H)
    assert not renderer.accum_export()[0].any() and not renderer.accum_export()[1].any()
    renderer.accum_import(*st)
    same_state(renderer.accum_export(), st, "after the import")
    back = renderer.accum_get()
    same_bits(back[0], got[0], "mean")
    same_bits(back[1], got[1], "variance")
    assert back[2] == got[2] == 2 * S
    assert back[3] == got[3] and got[3] > 0.0
    # each plane alone
    L = gi_amd.lib()
    only = np.zeros((H, W), dtype=np.int64)
    assert L.gi_accum_export(renderer._ctx, None, only.ctypes.data) == gi_amd.GI_OK
    same_bits(only, st[1], "counts alone")
    # an import needs no scene and no reset
    r = gi_amd.Renderer(0)
    try:
        r.accum_import(*st)
        same_state(r.accum_export(), st, "fresh context")
        fresh = r.accum_get()
        same_bits(fresh[0], got[0], "fresh mean")
        assert fresh[2:] == got[2:]
    finally:
        r.close()


# ---- 2. a merged pass is an added pass -----------------------------------------------------------
def test_merged_pass_is_an_added_pass(renderer, other, frames):
    import torch
    ref = frames[(5, 6)]
    a = add_passes(renderer, renderer.p, (5,))[-1]          # context A: seed 5
    same_state(a, frames[(5,)], "A")
    b = add_passes(other, other.p, (6,))[-1]                # context B: seed 6, maps of seed 5
    assert (b[0] != a[0]).any()
    # the host call
    renderer.accum_merge(*b)
    same_state(renderer.accum_export(), ref, "gi_accum_merge")
    assert renderer.accum_get()[2] == 2 * S
    # the packed pair
    nbytes = other.accum_state_bytes()
    assert nbytes == W * H * 56
    buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert other.accum_export_packed(buf.data_ptr(), nbytes) == nbytes
    assert buf.cpu().numpy().tobytes() == asr.pack(*b)
    renderer.accum_import(*a)
    ms = renderer.accum_merge_packed(1, buf.data_ptr(), nbytes)
    assert ms > 0.0
    same_state(renderer.accum_export(), ref, "gi_accum_merge_packed")
    # context to context
    renderer.accum_import(*a)
    ms = renderer.accum_merge_from(other)
    assert ms > 0.0
    same_state(renderer.accum_export(), ref, "gi_accum_merge_from")
    same_state(other.accum_export(), b, "B afterwards")


# ---- 3. the kernel against the restatement -------------------------------------------------------
def synth_state(rng, w, h, k, base=None):
    """State k of a synthetic set: means of both signs, per pixel p (shifted by k) empty, of one
    sample, of about 2^40 samples or of some hundreds, every eleventh pixel empty in every state;
    against `base` (the state folded into) every fifth pixel has base's means and every fifth its
    means negated."""
    npix = w * h
    pix = np.arange(npix) + 3 * k
    state = np.concatenate([rng.normal(0.0, 3.0, (npix, 3)), rng.random((npix, 3)) * 10.0], axis=1)
    counts = rng.integers(2, 1000, npix).astype(np.int64)
    counts[pix % 7 == 0] = 0
    counts[np.arange(npix) % 11 == 5] = 0      # empty in every state of the set
    counts[pix % 7 == 1] = 1
    big = pix % 7 == 2
    counts[big] = (1 << 40) + rng.integers(0, 1000, int(big.sum()))
    if base is not None:
        mu = np.asarray(base[0]).reshape(npix, 6)[:, :3]
        p = np.arange(npix)
        state[p % 5 == 0, :3] = mu[p % 5 == 0]
        state[p % 5 == 1, :3] = -mu[p % 5 == 1]
    return state.reshape(h, w, 6), counts.reshape(h, w)


@pytest.mark.parametrize("nstates", [1, 3, 8])
@pytest.mark.parametrize("w,h", [(37, 23), (1, 1)])
def test_device_fold_equals_restatement(renderer, w, h, nstates):
    npix, pad = w * h, 24
    for shift in range(1 if npix > 1 else 7):      # the single pixel takes every kind in turn
        rng = np.random.default_rng(100 * nstates + shift)
        a = synth_state(rng, w, h, shift)
        bs = [synth_state(rng, w, h, shift + 1 + k, a) for k in range(nstates)]
        ref = asr.fold_many(*a, bs)
        if npix > 1:   # the mix the inputs must hold, first state against a
            na, nb = a[1].ravel(), bs[0][1].ravel()
            d = bs[0][0].reshape(npix, 6)[:, :3] - a[0].reshape(npix, 6)[:, :3]
            both = (na > 0) & (nb > 0)
            assert ((na == 0) & (nb > 0)).any() and ((nb == 0) & (na > 0)).any()
            assert ((na == 0) & (nb == 0)).any() and (na == 1).any() and (nb == 1).any()
            assert (na >= 1 << 40).any() and (nb >= 1 << 40).any()
            assert (both & (d == 0).all(axis=1)).any()
            assert (both & (np.sign(bs[0][0].reshape(npix, 6)[:, 0])
                            == -np.sign(a[0].reshape(npix, 6)[:, 0]))).any()
            assert ref[1].max() > 1 << 40
        # the packed call: the states at a stride padded by 24 bytes (filled with ones)
        stride = npix * 56 + pad
        raw = b"".join(asr.pack(*b) + b"\xff" * pad for b in bs)
        buf = device_bytes(raw)
        renderer.accum_import(*a)
        renderer.accum_merge_packed(nstates, buf.data_ptr(), stride)
        same_state(renderer.accum_export(), ref, f"packed, shift {shift}")
        # the host call, state by state
        renderer.accum_import(*a)
        for b in bs:
            renderer.accum_merge(*b)
        same_state(renderer.accum_export(), ref, f"host, shift {shift}")


# ---- 4. the accumulator works on afterwards --------------------------------------------------------
def test_passes_after_an_import_equal_the_uninterrupted_context(renderer, frames):
    """(Two renders of seed 7 are compared: they have the same bits since the k-NN launch order no
    longer depends on the order in which blocks arrive, DESIGN.md "Accumulator state".)"""
    p = renderer.p
    renderer.accum_import(*frames[(5, 6)])
    st = add_passes(renderer, p, (7,), reset=False)[-1]
    same_state(st, frames[(5, 6, 7)], "whole-frame pass after the import")
    assert renderer.accum_get()[2] == 3 * S
    # an adaptive pass: T between two tile errors, so that the pass is a partial one
    add_passes(renderer, p, (5, 6))
    err = np.sort(renderer.accum_select(tile_px=4)[1])
    assert err[11] < err[12]
    T = 0.5 * (float(err[11]) + float(err[12]))

    def adaptive():
        p.seed = 7
        renderer.set_params(p)
        mask, active, _st = renderer.accum_add_adaptive(AA, tile_px=4, threshold=T)
        p.seed = 5
        renderer.set_params(p)
        return mask, active, renderer.accum_export(), renderer.accum_get()
    mask0, active0, st0, get0 = adaptive()                 # uninterrupted
    assert 0 < active0 < W * H
    renderer.accum_import(*frames[(5, 6)])
    mask1, active1, st1, get1 = adaptive()
    np.testing.assert_array_equal(mask1, mask0)
    assert active1 == active0
    same_state(st1, st0, "adaptive pass after the import")
    assert set(np.unique(st1[1])) == {2 * S, 3 * S}
    same_bits(get1[0], get0[0], "mean")
    same_bits(get1[1], get0[1], "variance")
    assert get1[2:] == get0[2:]


# ---- 5. association ------------------------------------------------------------------------------
def test_other_association_stays_within_rounding(renderer, frames):
    """(5, 6) + (7, 8) against ((5 + 6) + 7) + 8. Each fold step makes at most 4 roundings of 2^-53
    relative to the frame's scale, and its d * d * NS / N1 term carries 2 |d| delta_d * n / 4;
    sixteen such steps stay 50 times below 1e-12 of max|mu| (mu) and of max A + n_max max|mu|^2
    (A)."""
    one = frames[(5, 6, 7, 8)]
    renderer.accum_import(*frames[(5, 6)])
    renderer.accum_merge(*frames[(7, 8)])
    two = renderer.accum_export()
    same_bits(two[1], one[1], "counts")
    assert (two[1] == 4 * S).all()
    mu1, A1, mu2, A2 = one[0][..., :3], one[0][..., 3:], two[0][..., :3], two[0][..., 3:]
    mmax, amax, nmax = float(np.abs(mu1).max()), float(A1.max()), int(one[1].max())
    dmu, dA = float(np.abs(mu2 - mu1).max()), float(np.abs(A2 - A1).max())
    bound_mu, bound_A = 1e-12 * mmax, 1e-12 * (amax + nmax * mmax * mmax)
    print(f"max |dmu| {dmu:.3e} (bound {bound_mu:.3e}), max |dA| {dA:.3e} (bound {bound_A:.3e}), "
          f"{int((one[0] != two[0]).sum())} of {one[0].size} values differ in bits")
    assert dmu <= bound_mu
    assert dA <= bound_A


# ---- pass-parallel ranks -------------------------------------------------------------------------
def test_two_ranks_on_one_gpu_fold_in_rank_order(renderer, frames, tmp_path):
    """tools/progressive_ranks.py under torchrun, two gloo ranks on GPU 0, four passes: rank 0
    holds seeds 5 and 7, rank 1 seeds 6 and 8, and the written mean is the float32 of rank 0's
    state with rank 1's folded in."""
    import json
    import os
    import socket
    import subprocess
    import sys
    import radiance_ref as rr
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pfm = str(tmp_path / "merged.pfm")
    env = dict(os.environ, PROGRESSIVE_BACKEND="gloo", PROGRESSIVE_SAME_GPU="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "tools", "progressive_ranks.py"), scene("cornell.scn"), pfm, "4"]
    out = subprocess.run(cmd + CORNELL_FLAGS, env=env, capture_output=True, text=True, timeout=600,
                         cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and lines[0]["ranks"] == 2 and lines[0]["samples_per_pixel"] == 4 * S
    p = renderer.p
    held = [add_passes(renderer, p, seeds)[-1] for seeds in ((5, 7), (6, 8))]
    ref = asr.fold_many(*held[0], held[1:])
    assert (ref[1] == 4 * S).all()
    _img, raw = rr.read_pfm(pfm)
    assert raw == ref[0][..., :3].astype(np.float32).tobytes()


# ---- 6. errors -------------------------------------------------------------------------------------
def test_error_codes_leave_the_accumulator_unchanged(renderer, frames):
    import torch
    L = gi_amd.lib()
    ARG, STATE, UNSUP = gi_amd.GI_ERR_ARG, gi_amd.GI_ERR_STATE, gi_amd.GI_ERR_UNSUPPORTED
    st = tuple(np.array(a) for a in frames[(5, 6)])
    sp, cp = st[0].ctypes.data, st[1].ctypes.data
    nbytes = W * H * 56
    buf = torch.zeros(2 * nbytes, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    n = C.c_int64(0)
    r = gi_amd.Renderer(0)
    try:   # before a reset
        got = [L.gi_accum_export(r._ctx, sp, cp),
               L.gi_accum_merge(r._ctx, W, H, sp, cp),
               L.gi_accum_export_packed(r._ctx, None, 0, C.byref(n)),
               L.gi_accum_merge_packed(r._ctx, 1, buf.data_ptr(), nbytes, None),
               L.gi_accum_merge_from(r._ctx, renderer._ctx, None),
               L.gi_accum_merge_from(renderer._ctx, r._ctx, None)]
        assert got == [STATE] * len(got)
    finally:
        r.close()
    renderer.accum_import(*st)
    neg = st[1].copy()
    neg[H - 1, W - 1] = -1
    big = np.zeros((H, W + 1, 6)), np.zeros((H, W + 1), dtype=np.int64)
    calls = {
        "import with width 0": lambda: L.gi_accum_import(renderer._ctx, 0, H, sp, cp),
        "import with a negative count": lambda: L.gi_accum_import(renderer._ctx, W, H, sp,
                                                                  neg.ctypes.data),
        "import without counts": lambda: L.gi_accum_import(renderer._ctx, W, H, sp, None),
        "merge of another size": lambda: L.gi_accum_merge(renderer._ctx, W + 1, H,
                                                          big[0].ctypes.data, big[1].ctypes.data),
        "merge with a negative count": lambda: L.gi_accum_merge(renderer._ctx, W, H, sp,
                                                                neg.ctypes.data),
        "export of nothing": lambda: L.gi_accum_export(renderer._ctx, None, None),
        "nstates = 0": lambda: L.gi_accum_merge_packed(renderer._ctx, 0, buf.data_ptr(), nbytes,
                                                       None),
        "short stride": lambda: L.gi_accum_merge_packed(renderer._ctx, 2, buf.data_ptr(),
                                                        nbytes - 8, None),
        "odd stride": lambda: L.gi_accum_merge_packed(renderer._ctx, 1, buf.data_ptr(),
                                                      nbytes + 4, None),
        "misaligned states": lambda: L.gi_accum_merge_packed(renderer._ctx, 1, buf.data_ptr() + 4,
                                                             nbytes, None),
        "null states": lambda: L.gi_accum_merge_packed(renderer._ctx, 1, None, nbytes, None),
        "short export capacity": lambda: L.gi_accum_export_packed(renderer._ctx, buf.data_ptr(),
                                                                  nbytes - 1, C.byref(n)),
        "merge_from itself": lambda: L.gi_accum_merge_from(renderer._ctx, renderer._ctx, None),
    }
    for what, call in calls.items():
        assert call() == ARG, what
        same_state(renderer.accum_export(), st, what)
    assert not buf.cpu().numpy().any()                      # the short export wrote nothing
    assert L.gi_accum_export_packed(renderer._ctx, None, 0, C.byref(n)) == gi_amd.GI_OK
    assert n.value == nbytes
    with pytest.raises(ValueError):
        renderer.accum_merge(st[0][..., :5], st[1])
    # a device set
    r = gi_amd.Renderer(devices=[0, 0])
    try:
        got = [L.gi_accum_export(r._ctx, sp, cp),
               L.gi_accum_import(r._ctx, W, H, sp, cp),
               L.gi_accum_merge(r._ctx, W, H, sp, cp),
               L.gi_accum_export_packed(r._ctx, None, 0, C.byref(n)),
               L.gi_accum_merge_packed(r._ctx, 1, buf.data_ptr(), nbytes, None),
               L.gi_accum_merge_from(r._ctx, renderer._ctx, None),
               L.gi_accum_merge_from(renderer._ctx, r._ctx, None)]
        assert got == [UNSUP] * len(got)
    finally:
        r.close()
    same_state(renderer.accum_export(), st, "after the device set's calls")
