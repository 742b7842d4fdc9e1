"""The kd leaves' photon ranges (csrc/gi_layout.h kd_leaf_start, kd_leaf_range) on the host.

The kernels and the host build compute start(j) = (j * n) >> levels where they used to divide by
nleaves. tests/leaf_range_check.cpp includes the header as the library does and compares the two
for every j in [0, L] over a grid of (n, levels): n = 1, n = L - 1 (empty leaves), the leaf sizes
in use, products that cross 2^32 inside the map, n = 10^7 at L = 2^17 and n = 2^31 - 1; the starts
must be monotone and end at n. A plain host program: the header needs no device compiler."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_leaf_start_equals_the_division(tmp_path):
    exe = str(tmp_path / "leaf_range_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "global-illumination_amd", "csrc"),
                           os.path.join(ROOT, "tests", "leaf_range_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stderr
    assert p.stdout.startswith("ok ")
