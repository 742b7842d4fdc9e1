"""The fixture conditions tests/test_gpu_path_classes.py rests on, checked through the oracle on
the CPU (path_class_cases.path_stats: derived from the oracle's counters).

The GPU test compares the Monte Carlo schedules on scenes with boxes and with cylinders, under
a point light and under an area light. For the schedules to have something to disagree on,
every frame needs transmissive and specular sample paths, and paths that go past their first
bounce: GI_MC_WAVE=1 runs bounce 1 in the begin kernel and every later bounce in the tail
launch, GI_MC_WAVE=3 runs bounces 2 and 3 in the single-bounce rounds. A second bounce is
therefore enough to reach each kernel; `poly` also has a third, so that the second round of
GI_MC_WAVE=3 and the tail of a list that the first round shortened run on it.
"""
import pytest

import path_class_cases as cases


@pytest.mark.parametrize("name", cases.SCENES)
def test_scenes_have_the_paths_the_gpu_test_needs(name):
    st = cases.oracle_frame(name)[2]
    ps = cases.path_stats(name)
    print(name, ps, {k: st[k] for k in ("transmissive_samples", "specular_samples")})
    assert st["transmissive_samples"] > 0 and st["specular_samples"] > 0
    monte = ps["monte"]
    assert ps["paths"] > 0
    # monte[2] - monte[1] paths run a second bounce that hits something
    assert monte[2] - monte[1] >= 10
    assert monte[3] >= monte[2]
    if name.startswith("poly"):
        assert monte[3] > monte[2]


def test_scene_texts_differ_in_solids_and_light_only():
    lines = {n: set(cases.scene_text(n).splitlines()) for n in cases.SCENES}
    assert lines["poly"] ^ lines["all"] == set(cases.SOLIDS["poly"] + cases.SOLIDS["all"])
    for kind in ("poly", "all"):
        diff = lines[kind] ^ lines[kind + "_soft"]
        assert len(diff) == 2 and cases.AREA_LIGHT in diff
        assert any(ln.startswith("point_light") for ln in diff)
        assert "-lt" in cases.args(kind + "_soft") and "-lt" not in cases.args(kind)
