"""The drop-in CLI's argument stage against tests/cli_cases.py, the table of what it answered
before its source was split into stages, and its `-v` report against tests/cli_reports/.

No row of the table reaches a device: the stage ends before gi_create_devices, so these run on
CPU. A row that passes the stage fails next at the device (no GPU) or at the scene file, which
does not exist.

The reports are the CLI's stdout of four cornell.scn runs (24 x 16, aa 1) that between them print
every line of the report, recorded from the same earlier CLI over this library on an MI355X and
masked: the seconds after `Time =` (and after `Photon Tracing =` and `KdTree Construction =`, which
are gi_photon_stats' wall-clock times too), the `ms` figures, the scene's and the temporary
directory, and every redraw of a progress bar but each view's final 100 % one. Everything else in
them is counters of deterministic renders and repeats from run to run.
"""
import os
import re
import subprocess

import pytest

import cli_cases
from camera_cases import CORNELL_FLAGS
from gpu_util import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "global-illumination_amd", "photonmap")
REPORTS = os.path.join(ROOT, "tests", "cli_reports")


def case_id(c):
    return " ".join([f"{k}={v}" for k, v in c.env.items()] + (c.head or []) + c.tail) or "no arguments"


@pytest.mark.parametrize("case", cli_cases.CASES, ids=case_id)
def test_argument_stage_answers_as_recorded(case, tmp_path):
    assert os.path.exists(CLI), f"{CLI} not built (run __graft_entry__.build())"
    cli_cases.make_files(tmp_path)
    r = cli_cases.run_case(CLI, tmp_path, case.tail, case.env, case.head)
    err = r.stderr.replace(str(tmp_path), "{tmp}")
    if case.want is cli_cases.PASSES:
        assert r.returncode == 255, (r.returncode, err)
        assert not [t for t in cli_cases.REFUSAL_TEXTS if t in err], err
    else:
        assert (r.returncode, err) == case.want
    assert r.stdout == ""
    assert sorted(os.listdir(tmp_path)) == sorted(cli_cases.FILE_NAMES)


def test_table_is_well_formed():
    assert len(cli_cases.CASES) == len({(tuple(c.head or ()), tuple(c.tail), tuple(c.env.items()))
                                        for c in cli_cases.CASES})
    assert sum(c.want is cli_cases.PASSES for c in cli_cases.CASES) >= 20
    assert {c.want[0] for c in cli_cases.CASES if c.want} == {1, 255}


# ---- the -v report ------------------------------------------------------------------------------
REPORT_RUNS = {
    "plain": ["-v"],
    "views_history_adaptive_vdenoise": ["-it", "4", "-passes", "3", "-noise", "0", "-adaptive", "8", "-views",
                                        "{tmp}/views.txt", "-history", "8", "-vdenoise", "2", "-v"],
    "layers_vdenoise": ["-it", "4", "-passes", "2", "-layers", "{tmp}/p", "-vdenoise", "2", "-v"],
    "progressive_save_accum": ["-it", "4", "-passes", "2", "-progressive", "0.7", "-save_accum",
                               "{tmp}/s.acc", "-v"],
}
BAR_100 = "[" + "=" * 50 + "] 100%"
# test_cli_reproject.py's two cameras
_A = " ".join(cli_cases.CAM)
VIEWS = "\n".join(["# two cameras", _A, "", "  " + " ".join([repr(0.95 + 0.15)] + cli_cases.CAM[1:])]) + "\n"


def mask_report(stdout, tmp):
    """stdout (decoded without newline translation) with what differs between runs taken out: the
    redrawn bars (each ends in \\r; a line's text is what follows the last) but a line's final
    100 % one, the times, and the two directories."""
    out = []
    text = stdout.replace(str(tmp), "{tmp}").replace(scene("cornell.scn"), "{scene}")
    for line in text.split("\n"):
        bars = line.split("\r")
        line = BAR_100 if bars[-1] == "" and bars[-2:-1] == [BAR_100] else bars[-1]
        line = re.sub(r"((?:Time|Photon Tracing|KdTree Construction) = )[0-9.]+( seconds)$", r"\1T\2", line)
        line = re.sub(r"[0-9.]+ ms$", "T ms", line)
        out.append(line)
    return "\n".join(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REPORT_RUNS))
def test_verbose_report_is_the_recorded_text(name, tmp_path):
    (tmp_path / "views.txt").write_text(VIEWS)
    argv = [CLI, scene("cornell.scn"), str(tmp_path / "out.png")] + CORNELL_FLAGS + \
           [a.replace("{tmp}", str(tmp_path)) for a in REPORT_RUNS[name]]
    r = subprocess.run(argv, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = mask_report(r.stdout.decode(), tmp_path)
    print(got)
    with open(os.path.join(REPORTS, name + ".txt")) as f:
        assert got == f.read()
