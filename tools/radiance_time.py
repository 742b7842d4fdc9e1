#!/usr/bin/env python3
"""Time of the three radiance kernels (gi_radiance_bench: HIP events around each launch, median of
REPS after 5 warm-ups, on a synthetic frame) next to their compulsory traffic, and of one
gi_render_radiance frame next to gi_render_image's, on the GPU. Prints one JSON line.
usage: python3 tools/radiance_time.py [WIDTH HEIGHT [AA [REPS [FRAMES]]]]
       (default 1024 1024 2 50 3; FRAMES = 0 skips the two renders; the frame is bench.py's C2:
       cornell.scn, 1M + 1M photons, seed 1)"""
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
    w, h = (int(a[0]), int(a[1])) if len(a) > 1 else (1024, 1024)
    aa = int(a[2]) if len(a) > 2 else 2
    reps = int(a[3]) if len(a) > 3 else 50
    frames = int(a[4]) if len(a) > 4 else 3
    args = [os.path.join(ROOT, "tests", "scenes", "cornell.scn"), "/tmp/r.png", "-resolution",
            str(w), str(h), "-aa", str(aa), "-global", "1000000", "-caustic", "1000000", "-seed", "1"]
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(args)
    r = gi_amd.Renderer(0, p)
    out = {"width": w, "height": h, "aa": aa, "reps": reps}
    out.update(r.radiance_bench(aa, w, h, 5, reps))
    npix, S = w * h, 4 ** aa
    # compulsory bytes: primaries read once + pixel list + {m, M2} written; pass read + accumulator
    # read and written; accumulator read + one partial per 256 pixels
    traffic = {"reduce_radiance": npix * S * 24 + npix * 8 + npix * 48,
               "accum_merge": npix * 48 * 3,
               "accum_noise": npix * 48 + (npix + 255) // 256 * 8}
    for k, b in traffic.items():
        out[k + "_bytes"] = b
        out[k + "_gbps"] = b / out[k + "_ms"] / 1e6
    if frames > 0:
        r.ReadScene(sc, real)
        r.MapPhotons()
        mean = np.zeros((h, w, 3), dtype=np.float32)
        L = gi_amd.lib()
        r.RenderImage(aa, w, h)  # warm-up: buffers, batch size
        img, rad = [], []
        for _ in range(frames):
            t = time.perf_counter()
            r.RenderImage(aa, w, h)
            img.append(time.perf_counter() - t)
            t = time.perf_counter()
            r._check(L.gi_render_radiance(r._ctx, aa, w, h, mean.ctypes.data, None, None, None))
            rad.append(time.perf_counter() - t)
        out.update({"render_image_s": img, "render_radiance_s": rad,
                    "render_image_s_median": float(np.median(img)),
                    "render_radiance_s_median": float(np.median(rad))})
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
