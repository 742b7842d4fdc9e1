#!/usr/bin/env python3
"""Time of the variance-guided denoise pass (gi_denoise_radiance's and gi_accum_denoise's
kernel_ms: HIP events around the level launches) next to the fixed-sigma one (gi_denoise) on the
same frame, in one process, the calls interleaved, on the GPU. Prints one JSON line.
usage: python3 tools/vdenoise_time.py [SCENE [WIDTH HEIGHT [LEVELS [REPS [AA]]]]]
       (default cornell.scn 1024 1024 5 50 2; one radiance pass with small counts gives mean and
       variance: the filters' time depends on the frame's size, not on how it was sampled)"""
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
    w, h = (int(a[1]), int(a[2])) if len(a) > 2 else (1024, 1024)
    levels = int(a[3]) if len(a) > 3 else 5
    reps = int(a[4]) if len(a) > 4 else 50
    aa = int(a[5]) if len(a) > 5 else 2
    args = [os.path.join(ROOT, "tests", "scenes", scene), "/tmp/d.png", "-resolution", str(w),
            str(h), "-aa", str(aa), "-global", "20000", "-caustic", "20000", "-it", "4", "-tt", "4",
            "-st", "4", "-seed", "2"]
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(args)
    r = gi_amd.Renderer(0, p)
    r.ReadScene(sc, real)
    r.MapPhotons()
    r.accum_reset(w, h)
    st = r.accum_add_image(aa)           # one pass: mean and variance of 4^aa samples per pixel
    mean, var, n, _noise = r.accum_get()
    feat = r.camera_features(aa, w, h)
    clamped = np.clip(mean, 0.0, 1.0)    # the fixed-sigma filter's input range
    for _ in range(5):                   # warm-up: code objects, buffers
        r.denoise(clamped, feat, levels=levels)
        r.denoise_radiance(mean, var, feat, levels=levels)
        r.accum_denoise(feat, levels=levels)
    fixed, guided, accum, wall = [], [], [], []
    for _ in range(reps):
        fixed.append(r.denoise(clamped, feat, levels=levels)[1])
        t = time.perf_counter()
        guided.append(r.denoise_radiance(mean, var, feat, levels=levels)[2])
        wall.append((time.perf_counter() - t) * 1e3)
        accum.append(r.accum_denoise(feat, levels=levels)[2])
    r.close()
    traffic = (16 + 32 + 16) * w * h * levels  # compulsory bytes: colour + planes read, colour written
    out = {"scene": scene, "width": w, "height": h, "aa": aa, "samples_per_pixel": n,
           "levels": levels, "reps": reps, "compulsory_bytes": traffic,
           "coverage_mean": float(feat["coverage"].mean()),
           "variance_zero_share": float((var.max(axis=-1) == 0).mean()),
           "render_s": st["render_s"], "call_wall_ms_median": float(np.median(wall))}
    for name, ms in (("denoise", fixed), ("denoise_radiance", guided), ("accum_denoise", accum)):
        s = summary(ms)
        out[name + "_kernel_ms"] = s
        out[name + "_compulsory_gbps_at_median"] = traffic / s["median"] / 1e6
    print(json.dumps(out))


if __name__ == "__main__":
    main()
