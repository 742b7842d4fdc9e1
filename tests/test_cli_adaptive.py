"""The drop-in CLI's extension flag -adaptive [TILE] (only together with -noise T): whole-frame
passes until every pixel has the default min_samples, then gi_accum_add_adaptive passes with
threshold T over TILE x TILE tiles until no tile is active or -passes is used up. Like the other
extension flags it is taken out of argv before gi_parse_args; a malformed one is the reference's
"Invalid program argument" line and exit 1, before any device is opened.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import gi_amd
import radiance_ref as rr
from camera_cases import CORNELL_FLAGS
from gpu_util import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "global-illumination_amd", "photonmap")
W, H = 24, 16


def run(args, timeout=300):
    assert os.path.exists(CLI), f"{CLI} not built (run __graft_entry__.build())"
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("tail", [
    ["-adaptive"],                                     # without -noise
    ["-adaptive", "8"],
    ["-passes", "4", "-adaptive", "8", "-exposure", "2"],
    ["-noise", "0.02", "-adaptive", "3"],              # TILE out of range
    ["-noise", "0.02", "-adaptive", "65"],
    ["-adaptive", "-1", "-noise", "0.02"],
    ["-adaptive", "8", "-noise", "0.02", "-adaptive", "2"],   # the last one counts too
])
def test_malformed_adaptive_is_an_argument_error(tail, tmp_path):
    out = tmp_path / "o.png"
    # the scene does not exist: reaching ReadScene would print its message and exit -1
    r = run([str(tmp_path / "missing.scn"), str(out)] + tail)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert r.stderr == "Invalid program argument: -adaptive"
    assert r.stdout == ""
    assert not out.exists()


def test_adaptive_is_removed_before_parse_args(tmp_path):
    """With -noise the flag passes the argument stage, with or without TILE and wherever it
    stands: the next failure is the missing scene file (or, without a GPU, the device)."""
    for flags in (["-adaptive", "-noise", "0.02"], ["-noise", "0.02", "-aa", "0", "-adaptive"],
                  ["-adaptive", "16", "-noise", "0.02", "-no_shadow"],
                  ["-noise", "0.02", "-adaptive", "-no_shadow"]):
        r = run([str(tmp_path / "missing.scn"), str(tmp_path / "o.png")] + flags)
        assert r.returncode == 255, (flags, r.returncode, r.stderr)
        assert "Invalid program argument" not in r.stderr
    r = run([str(tmp_path / "missing.scn"), str(tmp_path / "o.png"), "-noise", "0.02", "-adaptive",
             "-gpus", "2"])
    assert r.returncode == 255 and "one device" in r.stderr
    with pytest.raises(ValueError, match=r"^Invalid program argument: -adaptive$"):
        gi_amd.ParseArgs(["a.scn", "b.png", "-adaptive"])


@pytest.mark.gpu
def test_adaptive_run_equals_the_same_sequence_through_the_api(renderer, tmp_path):
    passes = 6
    p, sc, _o, w, h, aa, real = gi_amd.ParseArgs([scene("cornell.scn"), "/tmp/x.png"] + CORNELL_FLAGS)
    assert (w, h, aa) == (W, H, 1)
    renderer.set_params(p)
    renderer.ReadScene(sc, real)
    renderer.MapPhotons()
    # T: between two tile errors at the median after the two whole-frame passes, so that the
    # third pass is a partial one (repr() round-trips through the CLI's strtod)
    renderer.accum_reset(w, h)
    for s in (5, 6):
        p.seed = s
        renderer.set_params(p)
        renderer.accum_add_image(aa)
    err = np.sort(renderer.accum_select(tile_px=4)[1])
    assert err[11] < err[12]
    T = 0.5 * (float(err[11]) + float(err[12]))
    renderer.accum_reset(w, h)
    done, least, kinds, rays = 0, 0, [], 0
    for i in range(passes):
        p.seed = 5 + i
        renderer.set_params(p)
        if least >= 8:
            _mask, ap, st = renderer.accum_add_adaptive(aa, tile_px=4, threshold=T)
            if ap == 0:
                break
            kinds.append(ap)
        else:
            st = renderer.accum_add_image(aa)
            kinds.append(w * h)
        rays += st["screen_rays"]
        done += 1
        least = renderer.accum_get()[2]
    p.seed = 5
    renderer.set_params(p)
    mean, _var, n, noise = renderer.accum_get()
    counts, total = renderer.accum_get_counts()
    print("pixels per pass:", kinds, "counts", counts.min(), counts.max(), "noise", noise)
    # the fixture condition: at least one pass of the run was a partial one
    assert kinds[:2] == [w * h, w * h] and any(0 < k < w * h for k in kinds[2:])
    png, pfm = str(tmp_path / "out.png"), str(tmp_path / "f.pfm")
    r = run([scene("cornell.scn"), png] + CORNELL_FLAGS + ["-passes", str(passes), "-noise", repr(T),
                                                          "-adaptive", "4", "-radiance", pfm, "-v"])
    assert r.returncode == 0, r.stderr
    _back, raw = rr.read_pfm(pfm)
    assert raw == mean.tobytes()
    m = re.search(r"^Accumulated image: (\d+) passes, (\d+) samples, (\d+) to (\d+) per pixel, "
                  r"noise = (\S+)$", r.stdout, re.M)
    assert m, r.stdout
    assert [int(m.group(k)) for k in (1, 2, 3, 4)] == [done, total, n, int(counts.max())]
    assert n == int(counts.min()) and total == 4 * sum(kinds)
    assert float(m.group(5)) == pytest.approx(noise, rel=1e-5)
    assert f"# Screen Rays = {rays}\n" in r.stdout
