#!/usr/bin/env python3
"""Cost of the light-path layers: warm gi_render_layers against warm gi_render_radiance in one
process from the same maps, the calls interleaved (host clock around the synchronous calls, mean
and variance asked for, no samples), the median of REPS each; then the HIP-event time of
reduce_prim_layers_kernel alone, summed over a frame's batches (gi_layers_timing), over REPS more
layered frames. On the GPU. Prints one JSON line and writes it to profiles/layers_bench.json.
usage: python3 tools/layers_bench.py [SCENE [RES [AA [PHOTONS [REPS]]]]]
       (default cornell.scn 1024 2 1000000 5: the benchmark's C2 frame)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "global-illumination_amd"))

import gi_amd  # noqa: E402


def summary(ms):
    ms = np.array(ms)
    return {"median": float(np.median(ms)), "min": float(ms.min()), "max": float(ms.max())}


def main():
    a = sys.argv[1:]
    scene = a[0] if len(a) > 0 else "cornell.scn"
    res = int(a[1]) if len(a) > 1 else 1024
    aa = int(a[2]) if len(a) > 2 else 2
    photons = int(a[3]) if len(a) > 3 else 1000000
    reps = max(5, int(a[4])) if len(a) > 4 else 5
    args = [os.path.join(ROOT, "tests", "scenes", scene), "/tmp/l.png", "-resolution", str(res),
            str(res), "-aa", str(aa), "-global", str(photons), "-caustic", str(photons), "-seed", "1"]
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(args)
    r = gi_amd.Renderer(0, p)
    r.ReadScene(sc, real)
    r.MapPhotons()
    for _ in range(2):                   # warm-up: code objects, buffers, batch sizes
        r.render_radiance(aa, w, h)
        r.render_layers(aa, w, h)
    plain, layered = [], []
    for _ in range(reps):
        t = time.perf_counter()
        mean, _var, _st = r.render_radiance(aa, w, h)
        plain.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        lmean, _lvar, _lst = r.render_layers(aa, w, h)
        layered.append((time.perf_counter() - t) * 1e3)
    same_total = bool((lmean[gi_amd.LAYER_TOTAL].view(np.uint32) == mean.view(np.uint32)).all())
    kernel = []
    for _ in range(reps):
        r.layers_timing(True)
        r.render_layers(aa, w, h)
        kernel.append(r.layers_timing(False))
    r.close()
    sp, sl = summary(plain), summary(layered)
    out = {"scene": scene, "width": w, "height": h, "aa": aa, "photons_per_map": photons,
           "reps": reps, "render_radiance_ms": sp, "render_layers_ms": sl,
           "layers_over_radiance_at_median": sl["median"] / sp["median"],
           "reduce_prim_layers_kernel_ms_per_frame": summary(kernel),
           "total_plane_equals_radiance_frame": same_total,
           "layer_mean_of_means": {n: float(lmean[l].mean()) for l, n in enumerate(gi_amd.LAYER_NAMES)}}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "layers_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
