"""The fixture conditions tests/test_gpu_mc_wave.py rests on, checked through the oracle on the
CPU. The oracle exposes no per-path bounce counts: the conditions are derived from its counters
(mc_wave_cases.path_stats, whose docstring says how).

With GI_MC_WAVE = R the begin kernel runs bounce 1, R - 1 launches run bounces 2 .. R and the
tail launch runs the rest. For the GPU test's R = 1, 3 and 200 to exercise what they name, both
frames need: transmissive and specular paths; a path that ends at its first bounce (the begin
kernel writes a base and stores no state) and one that goes on (it stores one); a path with
more than 3 bounces (R = 3 leaves work for the tail); no path as long as 200 bounces (the
tail of R = 200 finds an empty list; -md caps a path at 128).
"""
import pytest

import mc_wave_cases as cases


@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_paths_have_the_lengths_the_gpu_test_needs(name):
    ps = cases.path_stats(name)
    print(name, ps)
    paths = ps["transmissive_paths"] + ps["specular_paths"]
    monte = ps["monte"]
    assert ps["transmissive_paths"] > 0 and ps["specular_paths"] > 0
    # some paths end at their first bounce, some continue
    assert 0 < ps["continued1"] < paths
    # bounces 2, 3 and 4 are run by some path: the rounds of R = 3 and its tail have work
    assert monte[1] < monte[2] < monte[3] < monte[4] <= monte[cases.MD_DEFAULT]
    # mean bounces per path above 1 and below the -md cap, which itself is below R = 200
    mean = monte[cases.MD_DEFAULT] / paths
    assert 1.0 < mean < cases.MD_DEFAULT < 200


def test_plain_room_has_no_monte_carlo_paths():
    import oracle_lib
    _rgb, st = oracle_lib.render(cases.plain_args(), 16, 12)
    assert st["transmissive_samples"] == 0 and st["specular_samples"] == 0
    assert st["indirect_samples"] > 0 and st["knn_queries"] > 0
