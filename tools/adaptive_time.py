#!/usr/bin/env python3
"""Measurements of the adaptive passes (DESIGN.md "Adaptive passes", Measured) on the GPU. Each
mode prints one JSON line.
usage: python3 tools/adaptive_time.py kernels [WIDTH HEIGHT [TILE [REPS]]]    (1024 1024 8 50)
           gi_adaptive_bench: the tile error + selection kernels, the masked fold at half the
           tiles and the whole-frame fold (HIP events, median of REPS after 5 warm-ups, synthetic
           frame), next to their compulsory traffic
       python3 tools/adaptive_time.py frames [FRAMES [PACKAGE_DIR]]             (3)
           wall time of FRAMES gi_accum_add_image passes of bench.py's C2 frame (cornell.scn,
           1024 x 1024, aa 2, 1M + 1M photons) after one warm-up pass; PACKAGE_DIR: the
           global-illumination_amd directory of another build (a checkout of another commit), to
           compare the whole-frame pass across commits
       python3 tools/adaptive_time.py purpose [SIZE [PASSES [TILE [MAX_PASSES]]]]   (256 16 8 256)
           cornell.scn at SIZE x SIZE, -it 4, aa 1: PASSES uniform passes give the noise T; then
           the uniform loop to T (the CLI's -noise T) and the adaptive loop (-noise T -adaptive
           TILE, at most MAX_PASSES passes): primary samples, wall time, final noise and largest
           tile error of both; and of uniform passes continued until no tile's error is above T"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNELL = os.path.join(ROOT, "tests", "scenes", "cornell.scn")


def load_package(path=None):
    sys.path.insert(0, path or os.path.join(ROOT, "global-illumination_amd"))
    import gi_amd
    return gi_amd


def kernels(a):
    gi_amd = load_package()
    w, h = (int(a[0]), int(a[1])) if len(a) > 1 else (1024, 1024)
    tile = int(a[2]) if len(a) > 2 else 8
    reps = int(a[3]) if len(a) > 3 else 50
    r = gi_amd.Renderer(0)
    out = {"width": w, "height": h, "tile_px": tile, "reps": reps}
    out.update(r.adaptive_bench(w, h, tile, 5, reps))
    out.update({k: v for k, v in r.radiance_bench(0, w, h, 5, reps).items() if k == "accum_noise_ms"})
    r.close()
    npix = w * h
    ntiles = ((w + tile - 1) // tile) * ((h + tile - 1) // tile)
    # compulsory bytes: accumulator record + count read per pixel, error + smallest count written
    # and read again per tile, one mask byte; pass read, accumulator and count read and written
    # (+ the list's 8 B per pixel)
    traffic = {"select": npix * 56 + ntiles * (16 + 16 + 1),
               "masked_merge": (npix // 2) * (48 * 3 + 16 + 8),
               "accum_merge": npix * (48 * 3 + 16)}
    for k, b in traffic.items():
        out[k + "_bytes"] = b
        out[k + "_gbps"] = b / out[k + "_ms"] / 1e6
    print(json.dumps(out))


def frames(a):
    n = int(a[0]) if a else 3
    gi_amd = load_package(a[1] if len(a) > 1 else None)
    args = [CORNELL, "/tmp/r.png", "-resolution", "1024", "1024", "-aa", "2", "-global", "1000000",
            "-caustic", "1000000", "-seed", "1"]
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(args)
    r = gi_amd.Renderer(0, p)
    r.ReadScene(sc, real)
    r.MapPhotons()
    r.accum_reset(w, h)
    r.accum_add_image(aa)   # warm-up: buffers, batch size
    t = []
    for i in range(n):
        p.seed = 2 + i
        r.set_params(p)
        t0 = time.perf_counter()
        r.accum_add_image(aa)
        t.append(time.perf_counter() - t0)
    _m, _v, ns, noise = r.accum_get()
    r.close()
    print(json.dumps({"package": os.path.dirname(gi_amd.__file__), "accum_add_image_s": t,
                      "median_s": float(np.median(t)), "spread_s": max(t) - min(t),
                      "nsamples": ns, "noise": noise}))


def purpose(a):
    gi_amd = load_package()
    size = int(a[0]) if a else 256
    passes = int(a[1]) if len(a) > 1 else 16
    tile = int(a[2]) if len(a) > 2 else 8
    max_passes = int(a[3]) if len(a) > 3 else 256
    args = [CORNELL, "/tmp/r.png", "-resolution", str(size), str(size), "-aa", "1", "-it", "4"]
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(args)
    seed0 = p.seed
    r = gi_amd.Renderer(0, p)
    r.ReadScene(sc, real)
    r.MapPhotons()

    def loop(threshold, limit, adaptive, every_tile=False):
        """photonmap's pass loop (host/photonmap.cpp) under -noise threshold [-adaptive tile];
        every_tile: uniform passes until no tile's error is above the threshold"""
        r.accum_reset(w, h)
        least, done, partial = 0, 0, []
        t0 = time.perf_counter()
        for i in range(limit):
            p.seed = seed0 + i
            r.set_params(p)
            if adaptive and least >= 8:
                _mask, ap, _st = r.accum_add_adaptive(aa, tile_px=tile, threshold=threshold)
                if ap == 0:
                    break
                partial.append(ap)
            else:
                r.accum_add_image(aa)
            done += 1
            _m, _v, least, noise = r.accum_get()
            if every_tile:
                if least >= 8 and r.accum_select(tile_px=tile, threshold=threshold, dilate=0)[2] == 0:
                    break
            elif not adaptive and threshold is not None and least >= 2 and noise <= threshold:
                break
        wall = time.perf_counter() - t0
        _m, _v, least, noise = r.accum_get()
        counts, total = r.accum_get_counts()
        err = r.accum_select(tile_px=tile)[1]
        return {"passes": done, "primary_samples": total, "wall_s": wall, "noise": noise,
                "largest_tile_error": float(err.max()), "tiles_above_T": None,
                "count_min": int(counts.min()), "count_max": int(counts.max()),
                "partial_pass_pixels": partial}, err

    r.accum_reset(w, h)
    r.accum_add_image(aa)   # warm-up: buffers, batch size
    probe, _e = loop(None, passes, False)
    T = probe["noise"]
    uniform, eu = loop(T, passes, False)
    adaptive, ea = loop(T, max_passes, True)
    every, ee = loop(T, max_passes, False, True)
    uniform["tiles_above_T"] = int((eu > T).sum())
    adaptive["tiles_above_T"] = int((ea > T).sum())
    every["tiles_above_T"] = int((ee > T).sum())
    r.close()
    print(json.dumps({"size": size, "tile_px": tile, "T": T, "tiles": int(len(eu)),
                      "uniform": uniform, "adaptive": adaptive, "uniform_every_tile": every}))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    {"kernels": kernels, "frames": frames, "purpose": purpose}[mode](sys.argv[2:])
