#!/usr/bin/env python3
"""Measurements of the reprojection across views (DESIGN.md "Reprojection across views",
Measured) on the GPU. Each mode prints one JSON line.
usage: python3 tools/reproject_time.py kernel [SIZE [REPS]]                     (1024 50)
           cornell.scn at SIZE x SIZE, aa 0, two passes in view A; then gi_accum_reproject to a
           camera moved sideways by a few pixels and back, in turn (the accumulator stays a
           rendered one): HIP events around accum_reproject_kernel, median of REPS after 5
           warm-ups, next to its compulsory bytes; gi_adaptive_bench in the same run for the
           yardsticks (accum_merge_kernel, tile_error_kernel + tile_select_kernel)
       python3 tools/reproject_time.py purpose [SIZE [VIEWS [STEP [T [MAX_PASSES]]]]]
                                                               (256 8 0.03 0.037831 128)
           cornell.scn at SIZE x SIZE, aa 1, -it 4, a path of VIEWS cameras whose eye moves by
           STEP scene radii per view; the CLI's loop -views F -noise T -adaptive 8 through the API
           with and without -history 32: primary samples, wall time, kept and reset pixels, final
           noise and largest tile error per view"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNELL = os.path.join(ROOT, "tests", "scenes", "cornell.scn")
sys.path.insert(0, os.path.join(ROOT, "global-illumination_amd"))
import gi_amd  # noqa: E402


def context(size, aa, extra):
    args = [CORNELL, "/tmp/r.png", "-resolution", str(size), str(size), "-aa", str(aa)] + extra
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs(args)
    r = gi_amd.Renderer(0, p)
    info = r.ReadScene(sc, real)
    r.MapPhotons()
    return r, p, w, h, aa, info["radius"]


def kernel(a):
    size = int(a[0]) if a else 1024
    reps = int(a[1]) if len(a) > 1 else 50
    r, p, w, h, aa, _radius = context(size, 0, [])
    eye, towards, up, xfov = r.get_camera()
    # a sideways move of five pixel footprints at the frame's median depth
    covered = r.camera_features(aa, w, h)
    depth = float(np.median(covered["depth"][covered["coverage"] > 0]))
    step = 5 * 2.0 * float(np.tan(xfov)) * depth / w
    cams = [(eye, towards, up, xfov), ((eye[0] + step, eye[1], eye[2]), towards, up, xfov)]
    feat, views = [], []
    for c in cams:
        r.set_camera(*c)
        feat.append(r.camera_features(aa, w, h))
        views.append(r.get_view())
    r.set_camera(*cams[0])
    r.accum_reset(w, h)
    for s in (1, 2):
        p.seed = s
        r.set_params(p)
        r.accum_add_image(aa)
    ms, kept = [], []
    for i in range(5 + reps):
        src, dst = i % 2, 1 - i % 2
        r.set_camera(*cams[dst])
        st, t = r.accum_reproject(views[src], feat[src], feat[dst])
        ms.append(t)
        kept.append(st["kept_pixels"])
    ms = ms[5:]
    npix = w * h
    out = {"width": w, "height": h, "reps": reps, "eye_step": step,
           "accum_reproject_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms),
           "kept_pixels_first": kept[0], "kept_pixels_last": kept[-1], "pixels": npix}
    # compulsory bytes: the old record and count read once, two plane sets read, the new record
    # and count written
    out["accum_reproject_bytes"] = npix * (56 + 64 + 56)
    out["accum_reproject_gbps"] = out["accum_reproject_bytes"] / out["accum_reproject_ms"] / 1e6
    out.update(r.adaptive_bench(w, h, 8, 5, reps))
    r.close()
    print(json.dumps(out))


def purpose(a):
    size = int(a[0]) if a else 256
    nviews = int(a[1]) if len(a) > 1 else 8
    step = float(a[2]) if len(a) > 2 else 0.03
    T = float(a[3]) if len(a) > 3 else 0.037831
    max_passes = int(a[4]) if len(a) > 4 else 128
    r, p, w, h, aa, radius = context(size, 1, ["-it", "4"])
    seed0 = p.seed
    eye, towards, up, xfov = r.get_camera()
    cams = [((eye[0] + k * step * radius, eye[1], eye[2]), towards, up, xfov) for k in range(nviews)]
    r.accum_reset(w, h)
    r.accum_add_image(aa)   # warm-up: buffers, batch size

    def walk(history):
        """photonmap's loop under -views F -noise T -adaptive 8 [-history H]"""
        rows, prev = [], None
        t_all = time.perf_counter()
        for k, cam in enumerate(cams):
            t0 = time.perf_counter()
            r.set_camera(*cam)
            st, least = None, 0
            if history:
                feat = r.camera_features(aa, w, h)
            if history and k >= 1:
                st, _ms = r.accum_reproject(prev[0], prev[1], feat, max_history=history)
                least = r.accum_get()[2]
            else:
                r.accum_reset(w, h)
            samples, done = 0, 0
            for i in range(max_passes):
                p.seed = seed0 + i
                r.set_params(p)
                if st is not None or least >= 8:
                    _mask, ap, _st = r.accum_add_adaptive(aa, tile_px=8, threshold=T)
                    if ap == 0:
                        break
                    samples += ap * 4 ** aa
                else:
                    r.accum_add_image(aa)
                    samples += w * h * 4 ** aa
                done += 1
                least = r.accum_get()[2]
            if history:
                prev = (r.get_view(), feat)
            wall = time.perf_counter() - t0
            _m, _v, least, noise = r.accum_get()
            err = r.accum_select(tile_px=8)[1]
            rows.append({"view": k, "passes": done, "primary_samples": samples, "wall_s": wall,
                         "noise": noise, "largest_tile_error": float(err.max()),
                         "kept_pixels": None if st is None else st["kept_pixels"],
                         "reset_pixels": None if st is None else st["reset_pixels"],
                         "kept_samples": None if st is None else st["kept_samples"]})
        return {"views": rows, "primary_samples": sum(v["primary_samples"] for v in rows),
                "wall_s": time.perf_counter() - t_all}

    out = {"size": size, "views": nviews, "eye_step_radii": step, "T": T,
           "without_history": walk(0), "history_32": walk(32)}
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    {"kernel": kernel, "purpose": purpose}[mode](sys.argv[2:])
