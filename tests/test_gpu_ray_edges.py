"""The scene walk (scene_intersect_b, gi_device.h) and the shadow test (illum_test) on the
edge-case rays of ray_edge_cases.py, against the oracle: gi_intersect_probe / gi_illum_probe run
the device's own functions through every instance a scene can take. Nothing is excused: hit
flags, materials and shadow verdicts are equal, points and normals bit-equal (the device is built
without contraction and restates the oracle's fp64 sequence)."""
import numpy as np
import pytest

import gi_amd
import oracle_lib
import ray_edge_cases as rc

pytestmark = pytest.mark.gpu

# scenes with a scale under a scale, and their nesting levels (test_walk_matches_oracle)
NESTED_SCALE = {"nested.scn": 2}


def ulps(a, b):
    return np.abs(a.view(np.int64) - b.view(np.int64))


def check_walk(name, got, want, planes):
    gh, gt, gp, gn, gm, gtri = got
    oh, ot, op, on, om = want
    bad = np.flatnonzero(gh != oh)
    print(f"  hit flags differ: {len(bad)}; materials differ: {int((gm != om).sum())}; "
          f"points differ: {int((gp != op).any(1).sum())}; normals differ: "
          f"{int((gn != on).any(1).sum())}; t differ: {int((gt != ot).sum())}, "
          f"max {int(ulps(gt, ot).max())} ulp")
    np.testing.assert_array_equal(gh, oh)
    np.testing.assert_array_equal(gm, om)
    np.testing.assert_array_equal(gp, op)
    np.testing.assert_array_equal(gn, on)
    if name in NESTED_SCALE:
        assert ulps(gt, ot).max() <= 2 * NESTED_SCALE[name]
    else:
        np.testing.assert_array_equal(gt, ot)
    # tri names a triangle whose plane holds the point
    k = np.flatnonzero((gh != 0) & (gtri >= 0))
    assert (gtri[gh == 0] == -1).all() and (gtri < len(planes)).all()
    if len(k):
        pl = planes[gtri[k]]
        dist = np.abs((pl[:, :3] * gp[k]).sum(1) + pl[:, 3])
        assert dist.max() <= 1e-6, float(dist.max())
    return len(k)


@pytest.mark.parametrize("cls,name", rc.WALK_CASES)
def test_walk_matches_oracle(renderer, cls, name):
    """Hit flag, material, point and normal equal the oracle's in every scene; t too, except
    under a scale below a scale (NESTED_SCALE): the device multiplies the scales of a node's
    chain and divides the world t by the product once, where the reference divides level by
    level on the way down and multiplies level by level on the way up (R3SceneNode.cpp:454-458,
    499). The two orders round differently, so t is compared at 2 ulp per nesting level there.
    Within a node the device carries the node's own closest t from element to element as the
    reference does, so a tie between two elements of one node falls the same way (the coplanar
    pair of nested.scn, test_cpu_ray_edges.py::test_rays_reach_the_coplanar_pair). A tie between
    elements of two nodes with different scale chains is not made exact: there the reference's
    own rounding of the conversion decides, no fixture holds such a pair, and following it would
    take a per-level stack of closest values in the walk."""
    rays = rc.walk_rays(cls, name)
    want = rc.oracle_walk(cls, name)
    renderer.ReadScene(rc.scene_path(name))
    planes = renderer.triangle_planes()
    out = []
    for instance in (0, 1):
        print(f"{cls} {name} instance {instance}: {len(rays['org'])} rays")
        got = renderer.IntersectProbe(rays["org"], rays["dir"], None, instance)
        ntri = check_walk(name, got, want, planes)
        out.append(got)
    if cls == "edges" and len(rc.geometry(name).tris):
        assert ntri > 0
    for a, b in zip(out[0], out[1]):
        np.testing.assert_array_equal(a, b)
    if cls == "leaving":
        # the first cast gives the triangle each ray leaves from; its hit point is the origin
        sh, _t, sp, _n, _m, stri = renderer.IntersectProbe(rays["seed_org"], rays["seed_dir"])
        assert sh.all()
        np.testing.assert_array_equal(sp, rays["org"])
        print(f"  hinted: {int((stri >= 0).sum())} of {len(stri)} rays leave a triangle")
        for instance in (0, 1):
            hinted = renderer.IntersectProbe(rays["org"], rays["dir"], stri, instance)
            for a, b in zip(hinted, out[instance]):
                np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", rc.AXIS_SCENES)
def test_axis_rays_with_and_without_the_element_pretest(name, monkeypatch):
    """The axis class again with GI_ELEM_PRETEST 0 and 1 in fresh contexts (the default turns the
    pre-test off wherever every light is hard): its slab third starts on the faces of the grown
    boxes elem_maybe_hit and bvh_box read, where (face - o) * (1 / 0) is 0 * inf."""
    rays = rc.walk_rays("axis", name)
    want = rc.oracle_walk("axis", name)
    for pretest in ("0", "1"):
        monkeypatch.setenv("GI_ELEM_PRETEST", pretest)
        r = gi_amd.Renderer(0)
        try:
            r.ReadScene(rc.scene_path(name))
            planes = r.triangle_planes()
            for instance in (0, 1):
                print(f"axis {name} pretest {pretest} instance {instance}:")
                got = r.IntersectProbe(rays["org"], rays["dir"], None, instance)
                check_walk(name, got, want, planes)
        finally:
            r.close()


def test_probe_refuses_an_instance_that_does_not_hold_the_scene(renderer):
    renderer.ReadScene(rc.scene_path("stilllife.scn"))  # meshes and a box
    org, d = np.zeros((1, 3)), np.array([[0.0, -1.0, 0.0]])
    with pytest.raises(gi_amd.GiError):
        renderer.IntersectProbe(org, d, None, 2)
    renderer.IntersectProbe(org, d, None, 3)
    renderer.ReadScene(rc.scene_path("cylinder.scn"))
    with pytest.raises(gi_amd.GiError):
        renderer.IntersectProbe(org, d, None, 3)
    with pytest.raises(gi_amd.GiError):
        renderer.IllumProbe(org, -1, p_light=d, instance=3)
    with pytest.raises(gi_amd.GiError):  # the mask needs an area or rect light
        renderer.IllumProbe(org, 0, r12=np.zeros((1, 2)), mask=True)
    with pytest.raises(gi_amd.GiError):
        renderer.IllumProbe(org, -1, p_light=d, mask=True)


@pytest.mark.parametrize("cls,key", rc.ILLUM_CASES)
def test_shadow_verdicts_match_oracle(cls, key, monkeypatch):
    """Every case with the occluder mask on and off (area and rect lights), under
    GI_ELEM_PRETEST 0 and 1 in fresh contexts, through instance 0 and 1: all equal the oracle's
    RayIlluminationTest on the device's own point on the light."""
    rays = rc.illum_rays(cls, key)
    path = rc.scene_path(rc.illum_scene(key))
    soft = rays["light"][0] >= 0
    want = None
    for pretest in ("0", "1"):
        monkeypatch.setenv("GI_ELEM_PRETEST", pretest)
        r = gi_amd.Renderer(0)
        try:
            r.ReadScene(path)
            for mask in ((False, True) if soft else (False,)):
                for instance in (0, 1):
                    if soft:
                        lit, pl = r.IllumProbe(rays["p_scene"], rays["light"], r12=rays["r12"],
                                               mask=mask, instance=instance)
                    else:
                        lit, pl = r.IllumProbe(rays["p_scene"], -1, p_light=rays["p_light"],
                                               instance=instance)
                    if want is None:
                        # the generator's numpy point is the same expression: equal to rounding
                        np.testing.assert_allclose(pl, rays["p_light"], rtol=0, atol=1e-13)
                        if not soft:
                            np.testing.assert_array_equal(pl, rays["p_light"])
                        want = (oracle_lib.illum_test(path, rays["p_scene"], pl), pl)
                    np.testing.assert_array_equal(pl, want[1])
                    nbad = int((lit != want[0]).sum())
                    print(f"{cls} {key} pretest {pretest} mask {int(mask)} instance {instance}: "
                          f"{len(lit)} rays, lit {lit.mean():.3f}, differ {nbad}")
                    np.testing.assert_array_equal(lit, want[0])
        finally:
            r.close()
