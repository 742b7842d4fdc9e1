"""numpy restatement of the accumulator state of gi.h ("accumulator state"): the fold of one
state into another, the K-way left fold, and the CLI's -save_accum / -load_accum file. fp64, each
step one IEEE operation in the order gi.h writes; accum_fold_states_kernel (gi_radiance.hip) is
compared with it bit for bit in tests/test_gpu_accum_state.py.

A state is (state [..., 6] float64 = {mu.rgb, A.rgb}, counts [...] int64) over any pixel shape.
"""
import struct

import numpy as np

MAGIC = b"GIACC01\n"
HEADER = struct.Struct("<8siiq8s")   # magic, width, height, passes_done, 8 zero bytes
assert HEADER.size == 32


def fold(state_a, counts_a, state_b, counts_b):
    """b folded into a: (state, counts), new arrays.
    n_b == 0: a; n_a == 0: b; else Chan's update with (S, m, M2) = (n_b, mu_b, A_b)."""
    sa, sb = np.asarray(state_a, dtype=np.float64), np.asarray(state_b, dtype=np.float64)
    na, nb = np.asarray(counts_a, dtype=np.int64), np.asarray(counts_b, dtype=np.int64)
    assert sa.shape == sb.shape and sa.shape[-1] == 6 and na.shape == nb.shape == sa.shape[:-1]
    Na, Nb = na.astype(np.float64)[..., None], nb.astype(np.float64)[..., None]
    N1 = (na + nb).astype(np.float64)[..., None]
    NS = Na * Nb
    with np.errstate(all="ignore"):   # pixels the two special cases take are computed and dropped
        d = sb[..., :3] - sa[..., :3]
        mu = sa[..., :3] + (d * Nb) / N1
        A = (sa[..., 3:] + sb[..., 3:]) + ((d * d) * NS) / N1
    out = np.concatenate([mu, A], axis=-1)
    out = np.where((na == 0)[..., None], sb, out)
    out = np.where((nb == 0)[..., None], sa, out)
    return out, na + nb


def fold_many(state_a, counts_a, states):
    """The left fold ((a + b_0) + b_1) + ... over states = [(state, counts), ...] in order."""
    s, n = np.array(state_a, dtype=np.float64), np.array(counts_a, dtype=np.int64)
    for sb, nb in states:
        s, n = fold(s, n, sb, nb)
    return s, n


def pack(state, counts):
    """The packed state: the state plane's bytes, then the counts plane's."""
    return (np.ascontiguousarray(state, dtype="<f8").tobytes()
            + np.ascontiguousarray(counts, dtype="<i8").tobytes())


def unpack(buf, width, height):
    npix = width * height
    assert len(buf) == npix * 56, (len(buf), npix * 56)
    state = np.frombuffer(buf, dtype="<f8", count=npix * 6).reshape(height, width, 6)
    counts = np.frombuffer(buf, dtype="<i8", offset=npix * 48).reshape(height, width)
    return state, counts


def write_file(path, state, counts, passes_done):
    """photonmap -save_accum: the 32-byte header, the state plane, the counts plane."""
    h, w = np.shape(counts)
    with open(path, "wb") as f:
        f.write(HEADER.pack(MAGIC, w, h, passes_done, b"\0" * 8))
        f.write(pack(state, counts))


def read_file(path):
    """(state [H, W, 6], counts [H, W], passes_done) of a -save_accum file."""
    with open(path, "rb") as f:
        data = f.read()
    assert len(data) >= 32, len(data)
    magic, w, h, passes_done, zero = HEADER.unpack(data[:32])
    assert magic == MAGIC and zero == b"\0" * 8, (magic, zero)
    assert w > 0 and h > 0 and len(data) == 32 + w * h * 56, (w, h, len(data))
    state, counts = unpack(data[32:], w, h)
    return state, counts, passes_done
