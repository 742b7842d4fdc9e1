#!/usr/bin/env python3
"""Time of the denoise pass (gi_denoise's kernel_ms: HIP events around its level launches) and of
the feature planes on one rendered frame, on the GPU. Prints one JSON line.
usage: python3 tools/denoise_time.py [SCENE [WIDTH HEIGHT [LEVELS [REPS]]]]
       (default cornell.scn 1024 1024 5 50; the frame is rendered at aa 0 with small counts:
       the filter's time depends on the frame's size, not on how it was sampled)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "global-illumination_amd"))

import gi_amd  # noqa: E402


def main():
    a = sys.argv[1:]
    scene = a[0] if len(a) > 0 else "cornell.scn"
    w, h = (int(a[1]), int(a[2])) if len(a) > 2 else (1024, 1024)
    levels = int(a[3]) if len(a) > 3 else 5
    reps = int(a[4]) if len(a) > 4 else 50
    args = [os.path.join(ROOT, "tests", "scenes", scene), "/tmp/d.png", "-resolution", str(w),
            str(h), "-aa", "0", "-global", "20000", "-caustic", "20000", "-it", "4", "-tt", "4",
            "-st", "4", "-seed", "2"]
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(args)
    r = gi_amd.Renderer(0, p)
    r.ReadScene(sc, real)
    r.MapPhotons()
    _rgb, f, st = r.RenderImage(aa, w, h, want_float=True)
    t0 = time.perf_counter()
    feat = r.camera_features(aa, w, h)
    t1 = time.perf_counter()
    feat = r.camera_features(aa, w, h)
    feat_s = time.perf_counter() - t1
    for _ in range(5):  # warm-up: code objects, buffers
        r.denoise(f, feat, levels=levels)
    ms, wall = [], []
    for _ in range(reps):
        t = time.perf_counter()
        _rgb8, k = r.denoise(f, feat, levels=levels)
        wall.append((time.perf_counter() - t) * 1e3)
        ms.append(k)
    r.close()
    ms, wall = np.array(ms), np.array(wall)
    traffic = (16 + 32 + 16) * w * h * levels  # compulsory bytes: colour + planes read, colour written
    print(json.dumps({
        "scene": scene, "width": w, "height": h, "levels": levels, "reps": reps,
        "kernel_ms_median": float(np.median(ms)), "kernel_ms_min": float(ms.min()),
        "kernel_ms_max": float(ms.max()), "call_wall_ms_median": float(np.median(wall)),
        "compulsory_bytes": traffic, "compulsory_gbps_at_median": traffic / np.median(ms) / 1e6,
        "features_first_call_s": t1 - t0, "features_call_s": feat_s,
        "coverage_mean": float(feat["coverage"].mean()), "render_s": st["render_s"]}))


if __name__ == "__main__":
    main()
