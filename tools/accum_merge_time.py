#!/usr/bin/env python3
"""Measurement of the K-way accumulator merge (DESIGN.md "Accumulator state", Measured) on the
GPU. Prints one JSON line.
usage: python3 tools/accum_merge_time.py [SIZE [STATES [REPS]]]                 (1024 8 20)
           a SIZE x SIZE accumulator and STATES packed states of seeded random values with
           counts of some hundreds (every pixel takes the general branch); HIP events around
           accum_fold_states_kernel (gi_accum_merge_packed's kernel_ms), median of REPS launches
           after 5 warm-ups, next to its compulsory bytes: the accumulator and every state read
           once, 56 B per pixel each, the accumulator written once. gi_radiance_bench in the same
           run gives the yardstick: accum_merge_kernel folding one whole-frame pass (reads the
           pass's 48 B and the accumulator's 56 B per pixel, writes 56 B)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "global-illumination_amd"))
import gi_amd  # noqa: E402

HBM_PEAK = 8.0e12   # bytes per second


def main(a):
    import torch
    size = int(a[0]) if a else 1024
    nstates = int(a[1]) if len(a) > 1 else 8
    reps = int(a[2]) if len(a) > 2 else 20
    npix = size * size
    rng = np.random.default_rng(1)

    def state():
        s = np.concatenate([rng.normal(0.0, 3.0, (npix, 3)), rng.random((npix, 3)) * 10.0], axis=1)
        return s.reshape(size, size, 6), rng.integers(100, 1000, (size, size)).astype(np.int64)

    r = gi_amd.Renderer(0)
    r.accum_import(*state())
    nbytes = r.accum_state_bytes()
    assert nbytes == npix * 56
    host = np.empty((nstates, nbytes), dtype=np.uint8)
    for k in range(nstates):
        s, n = state()
        host[k, :npix * 48] = s.view(np.uint8).ravel()
        host[k, npix * 48:] = n.view(np.uint8).ravel()
    buf = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    ms = [r.accum_merge_packed(nstates, buf.data_ptr(), nbytes) for _ in range(5 + reps)][5:]
    _state, counts = r.accum_export()
    assert counts.min() >= 100 * (1 + (5 + reps) * nstates)
    med = float(np.median(ms))
    moved = npix * (56 * nstates + 56 + 56)
    out = {"width": size, "height": size, "states": nstates, "reps": reps,
           "accum_fold_states_ms": med, "min_ms": min(ms), "max_ms": max(ms),
           "bytes_read": npix * (56 * nstates + 56), "bytes_written": npix * 56,
           "gbps": moved / med / 1e6, "fraction_of_8_TBps": moved / (med * 1e-3) / HBM_PEAK,
           "ms_per_state": med / nstates}
    bench = r.radiance_bench(0, size, size, 5, 50)
    out["accum_merge_ms"] = bench["accum_merge_ms"]
    out["accum_merge_gbps"] = npix * (48 + 56 + 56) / bench["accum_merge_ms"] / 1e6
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
