#!/usr/bin/env python3
"""What filtering the light-path layers apart buys: cornell.scn at -it 4, PASSES passes, the
variance-guided filter (LEVELS levels) of the undivided accumulator against the sum of the
separately filtered layers (specular left unfiltered: photonmap -layers -vdenoise), both as RMSE
of unclamped radiance against the mean of REF passes under other seeds; separately over the pixels
whose primary hit is the glass sphere or the mirror (albedo 0, coverage > 0) and over the rest. On
the GPU. Prints one JSON line and writes it to profiles/layers_benefit.json.
usage: python3 tools/layers_benefit.py [WIDTH HEIGHT [PASSES [REF [LEVELS]]]]  (96 64 8 512 5)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "global-illumination_amd"))

import gi_amd  # noqa: E402


def rmse(a, b, mask):
    d = (a.astype(np.float64) - b.astype(np.float64))[mask]
    return float(np.sqrt((d * d).mean()))


def main():
    a = sys.argv[1:]
    w, h = (int(a[0]), int(a[1])) if len(a) > 1 else (96, 64)
    passes = int(a[2]) if len(a) > 2 else 8
    nref = int(a[3]) if len(a) > 3 else 512
    levels = int(a[4]) if len(a) > 4 else 5
    aa = 1
    args = [os.path.join(ROOT, "tests", "scenes", "cornell.scn"), "/tmp/l.png", "-resolution",
            str(w), str(h), "-aa", str(aa), "-global", "20000", "-caustic", "20000", "-it", "4",
            "-tt", "8", "-st", "8", "-seed", "5"]
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(args)
    r = gi_amd.Renderer(0, p)
    r.ReadScene(sc, real)
    r.MapPhotons()
    feat = r.camera_features(aa, w, h)
    r.accum_reset(w, h)
    for i in range(nref):
        p.seed = 100000 + i
        r.set_params(p)
        r.accum_add_image(aa)
    ref = r.accum_get()[0]
    layers = [gi_amd.Renderer(0) for _ in range(gi_amd.LAYER_COUNT)]
    r.accum_reset(w, h)
    for x in layers:
        x.accum_reset(w, h)
    for i in range(passes):
        p.seed = 5 + i
        r.set_params(p)
        r.accum_add_image_layers(aa, layers)
    noisy = r.accum_get()[0]
    whole = r.accum_denoise(feat, levels=levels)[0]
    total = np.zeros(whole.shape, dtype=np.float64)
    for l, x in enumerate(layers):
        part = (x.accum_get()[0] if l == gi_amd.LAYER_SPECULAR
                else x.accum_denoise(feat, levels=levels)[0])
        total = total + part.astype(np.float64)
    apart = total.astype(np.float32)
    for x in layers + [r]:
        x.close()
    shiny = (feat["albedo"].max(axis=-1) == 0) & (feat["coverage"] > 0)
    out = {"scene": "cornell.scn", "width": w, "height": h, "aa": aa, "indirect_test": 4,
           "passes": passes, "reference_passes": nref, "levels": levels,
           "glass_and_mirror_pixels": int(shiny.sum()), "other_pixels": int((~shiny).sum())}
    for name, mask in (("glass_and_mirror", shiny), ("rest", ~shiny)):
        out["rmse_" + name] = {"unfiltered": rmse(noisy, ref, mask),
                               "vdenoise": rmse(whole, ref, mask),
                               "layers_vdenoise": rmse(apart, ref, mask)}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "layers_benefit.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
