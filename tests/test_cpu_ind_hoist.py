"""The fixture of tests/test_gpu_ind_hoist.py (ind_hoist_cases.py) checked on the oracle alone for
its power to show an error in the values the indirect paths share. No GPU.

Of the oracle's primary hits (its camera rays, its intersections) at least 10 % are back-facing
and at least 10 % fall in each branch of the diffuse sampler's tangent; none is on the glass
sphere, so every global-map query of the frame comes from an indirect sample, and at least 25 %
of the indirect samples issue one; at least 60 % of the float values lie strictly inside (0, 1).
The same for the frame with depth of field, and the (0, 1) share for the ray batch.
"""
import pytest

import ind_hoist_cases as cases
import ray_cases


@pytest.mark.parametrize("dof", [False, True], ids=["pinhole", "dof2"])
def test_frame_can_show_an_error(dof):
    back, first, second, glass = cases.primary_classes(dof)
    _rgb, f, st = cases.oracle_frame(dof)
    queries = st["knn_queries"] - st["caustic_samples"]  # one caustic query per caustic sample
    share = queries / st["indirect_samples"]
    inside = ray_cases.inside_fraction(f)
    print(f"back-facing {back:.3f}, tangent branches {first:.3f} / {second:.3f}, glass primary "
          f"hits {glass}, indirect samples {st['indirect_samples']:.0f} of which {share:.3f} "
          f"query, values inside (0, 1) {inside:.3f}")
    assert back >= 0.10
    assert first >= 0.10 and second >= 0.10
    assert glass == 0
    assert st["caustic_samples"] == st["screen_rays"]
    assert share >= 0.25
    assert inside >= 0.60
    assert st["caustic_stored"] > 0 and st["transmissive_samples"] > 0  # the sphere is reached


@pytest.mark.parametrize("explicit", [True, False], ids=["ids", "default_ids"])
def test_ray_batch_can_show_an_error(explicit):
    cases.register_ray_scene()
    rays, _ids = ray_cases.batch(cases.RAY_SCENE, cases.RAY_SENSOR, cases.RAY_SPP)
    _rgb, f, st = ray_cases.oracle_batch(cases.RAY_SCENE, cases.RAY_SENSOR, cases.RAY_SPP, explicit)
    hits = ray_cases.hit_fraction(cases.RAY_SCENE, rays)
    inside = ray_cases.inside_fraction(f)
    print(f"rays that hit {hits:.3f}, values inside (0, 1) {inside:.3f}, indirect samples "
          f"{st['indirect_samples']:.0f}")
    assert hits >= 0.60 and inside >= 0.60
    assert st["indirect_samples"] > 0
