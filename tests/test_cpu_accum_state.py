"""The accumulator state's restatement (tests/accum_state_ref.py) and the pass-parallel ranks
(gi_dist.accumulate_passes), without a GPU.

- the fold: a one-pass state folded in is radiance_ref.Accum adding that pass, bit for bit; an
  empty state is the identity; an empty accumulator takes the state as it is; the -save_accum file
  round trip returns the same bytes;
- gloo worlds of 2 and 3 with a stand-in renderer on host memory and 5 passes (the ranks hold
  unequal numbers of them): rank 0's result is fold_many of the ranks' states in rank order, bit
  for bit, every pixel holds 5 * S samples, and every rank sent one gather of W * H * 56 bytes."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import accum_state_ref as asr
import gi_dist
import radiance_ref as rr

W, H, S = 13, 7, 4


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes()


def one_pass(seed):
    """A pass's {m, M2} [H, W, 6] of S samples per pixel, made from its seed alone."""
    smp = np.random.default_rng(1000 + seed).random((H, W, S, 3)) * 3.0
    m, m2 = rr.pass_stats(smp, rr.box_weight(aa=1))
    return np.concatenate([m, m2], axis=-1)


def pass_state(seed):
    return one_pass(seed), np.full((H, W), S, dtype=np.int64)


def empty_state():
    return np.zeros((H, W, 6)), np.zeros((H, W), dtype=np.int64)


def test_folding_one_pass_states_is_adding_the_passes():
    ref = rr.Accum((H, W))
    s, n = empty_state()
    for seed in (5, 6, 7):
        f = one_pass(seed)
        ref.add(f[..., :3], f[..., 3:], S)
        s, n = asr.fold(s, n, *pass_state(seed))
        same_bits(s[..., :3], ref.mu)
        same_bits(s[..., 3:], ref.A)
        assert (n == ref.N).all()
    # and the three as one fold_many
    s3, n3 = asr.fold_many(*empty_state(), [pass_state(k) for k in (5, 6, 7)])
    same_bits(s3, s)
    same_bits(n3, n)


def test_empty_state_is_the_identity_and_an_empty_accumulator_copies():
    a = asr.fold_many(*empty_state(), [pass_state(5), pass_state(6)])
    s, n = asr.fold(*a, *empty_state())
    same_bits(s, a[0])
    same_bits(n, a[1])
    s, n = asr.fold(*empty_state(), *a)
    same_bits(s, a[0])
    same_bits(n, a[1])
    # per pixel: only some pixels of either side empty; -0.0 and a NaN pass through as bits
    sa, na = (np.array(v) for v in a)
    sb, nb = (np.array(v) for v in pass_state(7))
    na[0, :] = 0
    nb[:, 0] = 0
    sb[1, 1, 0] = -0.0
    sa[2, 0, 3] = np.nan
    s, n = asr.fold(sa, na, sb, nb)
    same_bits(s[0, 1:], sb[0, 1:])      # n_a == 0: b
    same_bits(s[1:, 0], sa[1:, 0])      # n_b == 0: a
    same_bits(s[0, 0], sa[0, 0])        # both empty: a
    assert n[0, 0] == 0 and (n[0, 1:] == S).all() and (n[1:, 0] == 2 * S).all()
    assert (n[1:, 1:] == 3 * S).all()


def test_file_round_trip(tmp_path):
    s, n = asr.fold_many(*empty_state(), [pass_state(5), pass_state(6)])
    p = str(tmp_path / "a.acc")
    asr.write_file(p, s, n, 2)
    raw = open(p, "rb").read()
    assert len(raw) == 32 + W * H * 56
    assert raw[:8] == b"GIACC01\n" and raw[24:32] == b"\0" * 8
    assert np.frombuffer(raw, dtype="<i4", count=2, offset=8).tolist() == [W, H]
    assert int(np.frombuffer(raw, dtype="<i8", count=1, offset=16)[0]) == 2
    s2, n2, done = asr.read_file(p)
    same_bits(s2, s)
    same_bits(n2, n)
    assert done == 2
    q = str(tmp_path / "b.acc")
    asr.write_file(q, s2, n2, done)
    assert open(q, "rb").read() == raw
    same_bits(asr.unpack(asr.pack(s, n), W, H)[0], s)


# ---- pass-parallel ranks over gloo ----------------------------------------------------------
class Params:
    def __init__(self, seed):
        self.seed = seed


class FakeAccum:
    """The accumulator calls accumulate_passes uses, on host memory: a pass is one_pass(seed), the
    packed entry points read and write through raw host pointers."""
    packed_host_memory = True   # opts in with a CPU device

    def __init__(self):
        self.seed = None
        self.state = None

    def set_params(self, p):
        self.seed = p.seed

    def accum_reset(self, w, h):
        assert (w, h) == (W, H)
        self.state = empty_state()

    def accum_add_image(self, aa):
        self.state = asr.fold(*self.state, *pass_state(self.seed))

    def accum_export_packed(self, ptr, cap):
        raw = asr.pack(*self.state)
        assert cap >= len(raw)
        C.memmove(ptr, raw, len(raw))
        return len(raw)

    def accum_merge_packed(self, nstates, ptr, stride):
        states = [asr.unpack(C.string_at(ptr + k * stride, W * H * 56), W, H)
                  for k in range(nstates)]
        self.state = asr.fold_many(*self.state, states)

    def accum_get(self):
        return self.state


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, passes, base_seed, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sent = []
        real_gather = dist.gather

        def spy(t, parts=None, dst=0):
            sent.append(t.numel() * t.element_size())
            return real_gather(t, parts, dst=dst)
        dist.gather = spy
        r, p = FakeAccum(), Params(base_seed)
        got = gi_dist.accumulate_passes(r, 1, W, H, passes, p, rank, world, dist,
                                        torch.device("cpu"))
        q.put((rank, got, sent, p.seed, r.seed))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_fold_in_rank_order(world):
    passes, base_seed = 5, 40
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, passes, base_seed, q))
             for r in range(world)]
    for p in procs:
        p.start()
    out = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    out.sort(key=lambda x: x[0])
    # what each rank holds before the gather: its own passes in order
    held = [asr.fold_many(*empty_state(), [pass_state(base_seed + i)
                                           for i in gi_dist.rank_passes(passes, r, world)])
            for r in range(world)]
    assert sorted(len(gi_dist.rank_passes(passes, r, world)) for r in range(world))[0] \
        < -(-passes // world)                      # unequal numbers of passes
    ref = asr.fold_many(*held[0], held[1:])
    state, counts = out[0][1]
    same_bits(state, ref[0])
    same_bits(counts, ref[1])
    assert (counts == passes * S).all()
    assert all(o[1] is None for o in out[1:])
    for o in out:
        assert o[2] == [W * H * 56]                # one gather of the packed state
        assert o[3] == base_seed and o[4] == base_seed   # the base parameters are back
