#!/usr/bin/env python3
"""The progressive pipeline on several GPUs, cut by passes (gi_dist.accumulate_passes): every
rank builds the same photon maps, rank r renders the passes i % world == r under seed + i, and
rank 0 folds the ranks' accumulator states in rank order and writes the merged mean.

usage: torchrun --nproc_per_node N tools/progressive_ranks.py SCENE OUT.pfm PASSES [FLAGS ...]
           SCENE, FLAGS: as for photonmap (-resolution, -aa, -global, -caustic, -seed, ...);
           OUT: .pfm or .hdr, the unclamped mean of all PASSES passes (written by rank 0)
       PROGRESSIVE_SAME_GPU=1 maps every rank onto GPU 0 and PROGRESSIVE_BACKEND=gloo carries the
       gather through host memory (a one-GPU machine; RCCL needs distinct GPUs).
Rank 0 prints one JSON line: passes, ranks, samples per pixel, noise, seconds."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "global-illumination_amd"))


def main(argv):
    if len(argv) < 3:
        raise SystemExit(__doc__)
    import torch
    import torch.distributed as dist
    import gi_amd
    import gi_dist
    scene, out, passes = argv[0], argv[1], int(argv[2])
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = 0 if os.environ.get("PROGRESSIVE_SAME_GPU") == "1" else int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dist.init_process_group(backend=os.environ.get("PROGRESSIVE_BACKEND") or "nccl",
                            rank=rank, world_size=world)
    try:
        p, sc, _o, w, h, aa, real = gi_amd.ParseArgs([scene, "/tmp/unused.png"] + argv[3:])
        r = gi_amd.Renderer(local, p)
        r.ReadScene(sc, real)
        if p.indirect_illum or p.caustic_illum or p.direct_photon_illum:
            r.MapPhotons()
        t0 = time.perf_counter()
        got = gi_dist.accumulate_passes(r, aa, w, h, passes, p, rank, world, dist,
                                        torch.device("cuda", local))
        if got is not None:
            mean, _var, n, noise = got
            gi_amd.write_image_float(out, mean)
            print(json.dumps({"passes": passes, "ranks": world, "samples_per_pixel": n,
                              "noise": noise, "seconds": time.perf_counter() - t0}))
        r.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1:])
