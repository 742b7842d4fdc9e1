"""bench.py's command line and its --dump-outputs writer (no GPU: nothing is rendered)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_outputs_writes_float32_arrays(tmp_path):
    rgb = (np.arange(5 * 7 * 3) % 256).astype(np.uint8).reshape(5, 7, 3)
    bench.dump_outputs(str(tmp_path / "d"), {"rgb": rgb})
    got = np.load(tmp_path / "d" / "rgb.npy")
    assert got.dtype == np.float32 and got.shape == rgb.shape
    np.testing.assert_array_equal(got, rgb.astype(np.float32))


def test_dump_outputs_samples_past_the_limit(tmp_path, monkeypatch):
    """Two outputs share the limit; the one larger than its share is cut to the same seeded
    sample of its elements on every run, the smaller one is written whole."""
    monkeypatch.setattr(bench, "DUMP_LIMIT", 800)  # 100 float32 elements per file
    big = np.arange(1000, dtype=np.float64).reshape(10, 100)
    small = np.arange(30, dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (100,)
    np.testing.assert_array_equal(a, b)
    assert len(set(a.tolist())) == 100 and np.all(np.diff(a) > 0)  # distinct elements, in order
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "small.npy"), small)
    total = sum(np.load(tmp_path / "a" / f).nbytes for f in os.listdir(tmp_path / "a"))
    assert total <= 800


def test_command_line_has_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in out.stdout
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                         capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--steps" in bad.stderr
