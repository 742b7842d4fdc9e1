"""The drop-in CLI's extension flag -progressive A (a radiance flag): every pass traces fresh
photon maps and estimates with the pass's fixed radii (gi_accum_add_progressive), with the pass
index counted across -save_accum / -load_accum, so a run that is saved after two passes and
resumed for two more ends with the bytes of the uninterrupted four-pass run."""
import os
import re
import subprocess

import pytest

import progressive_ref as pref
from gpu_util import scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "global-illumination_amd", "photonmap")
FLAGS = ["-resolution", "24", "16", "-aa", "1", "-global", "20000", "-caustic", "20000",
         "-it", "4", "-tt", "2", "-st", "2", "-seed", "5", "-gd", "0.1", "-cd", "0.05",
         "-progressive", "0.7"]


def run(args, timeout=300):
    assert os.path.exists(CLI), f"{CLI} not built (run __graft_entry__.build())"
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=timeout)


def test_resumed_run_equals_the_uninterrupted_run(tmp_path):
    base = [scene("cornell.scn")]
    t = {k: str(tmp_path / k) for k in ("a.png", "b.png", "c.png", "d.png", "a.pfm", "b.pfm",
                                        "c.pfm", "d.pfm", "a.acc", "b.acc", "c.acc")}
    r = run(base + [t["a.png"]] + FLAGS + ["-v", "-passes", "2", "-radiance", t["a.pfm"],
                                           "-save_accum", t["a.acc"]])
    assert r.returncode == 0, r.stderr
    # -v names each pass's radii as -gd / -cd, and the stored photon counts
    lines = [l for l in r.stdout.splitlines() if l.startswith("Progressive pass")]
    assert len(lines) == 2, r.stdout
    for p, line in enumerate(lines):
        m = re.match(r"Progressive pass (\d+): -gd (\S+) -cd (\S+), (\d+) global and (\d+) caustic "
                     r"photons stored$", line)
        assert m, line
        assert int(m.group(1)) == p
        assert float(m.group(2)) == pref.radius(0.1, 0.7, p)
        assert float(m.group(3)) == pref.radius(0.05, 0.7, p)
        assert int(m.group(4)) >= 20000 and int(m.group(5)) >= 20000
    assert "Built photon map" not in r.stdout    # no up-front map build
    r = run(base + [t["b.png"]] + FLAGS + ["-v", "-load_accum", t["a.acc"], "-passes", "2",
                                           "-radiance", t["b.pfm"], "-save_accum", t["b.acc"]])
    assert r.returncode == 0, r.stderr
    assert "Progressive pass 2:" in r.stdout and "Progressive pass 3:" in r.stdout
    r = run(base + [t["c.png"]] + FLAGS + ["-passes", "4", "-radiance", t["c.pfm"],
                                           "-save_accum", t["c.acc"]])
    assert r.returncode == 0, r.stderr

    def raw(k):
        with open(t[k], "rb") as f:
            return f.read()
    assert raw("b.acc") == raw("c.acc")
    assert raw("b.pfm") == raw("c.pfm")
    assert raw("b.png") == raw("c.png")
    assert raw("a.acc")[32:] != raw("c.acc")[32:]
    # and the flag does something: four fixed-map passes give another image
    fixed = [f for f in FLAGS[:-2]]
    r = run(base + [t["d.png"]] + fixed + ["-passes", "4", "-radiance", t["d.pfm"]])
    assert r.returncode == 0, r.stderr
    assert raw("d.pfm") != raw("c.pfm")
