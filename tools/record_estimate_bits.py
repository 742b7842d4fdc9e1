#!/usr/bin/env python3
"""Records tests/golden/estimate_bits.json (tests/test_gpu_estimate_bits.py) from the built
library, on a GPU. Run it on the commit whose bits are the reference, i.e. before a change to
the estimate; a change that is meant to alter the bits re-records and says so.
usage: tools/record_estimate_bits.py [output file]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "global-illumination_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import synth  # noqa: E402
import test_gpu_estimate_bits as t  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
photons = synth.photon_map(t.N_PHOTONS, seed=41)
rec = {}
for cid, env, fname, k, r in t.CASES:
    rec[cid] = t.case_bits(env, fname, k, r, photons)
    print(cid, {n: v["sum"] for n, v in rec[cid].items()}, flush=True)
rec[t.CACHE_ID] = t.cache_bits()
print(t.CACHE_ID, rec[t.CACHE_ID]["sum"], flush=True)
with open(out, "w") as f:
    json.dump(rec, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", out, len(rec), "entries")
