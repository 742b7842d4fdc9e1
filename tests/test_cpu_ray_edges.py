"""The edge-case ray classes of ray_edge_cases.py through the oracle alone: each class must be
what test_gpu_ray_edges.py takes it for, or the device could pass that file without having met
the cases. No GPU."""
import numpy as np
import pytest

import oracle_lib
import ray_edge_cases as rc


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("cls,name", rc.WALK_CASES)
def test_walk_class(cls, name):
    fn = rc.WALK_CLASSES[cls][0]
    rays = rc.walk_rays(cls, name)
    _same(rays, fn.__wrapped__(name))  # deterministic under its seed
    n = len(rays["org"])
    assert 2000 <= n <= 12000
    np.testing.assert_allclose(np.linalg.norm(rays["dir"], axis=1), 1.0, rtol=0, atol=1e-12)
    hit, t, p, nr, _m = rc.oracle_walk(cls, name)
    assert np.isfinite(t).all() and np.isfinite(p).all() and np.isfinite(nr).all()
    on = rc.on_target(rays, hit, t)
    print(f"{cls} {name}: {n} rays, hit {np.mean(hit != 0):.3f}, on target {on.mean():.3f}")
    assert on.mean() >= 0.10
    if (cls, name) not in rc.FEW_MISSES:
        assert (~on).mean() >= 0.10
    if cls == "axis":
        d = rays["dir"]
        zeros = (d == 0.0).sum(1)
        assert set(np.unique(zeros)) == {1, 2}
        assert (np.signbit(d) & (d == 0.0)).any() and (~np.signbit(d) & (d == 0.0)).any()
        assert rays["face"].mean() == pytest.approx(1.0 / 3.0, abs=0.01)
        assert rays["slab"].mean() == pytest.approx(1.0 / 3.0, abs=0.01)
        # the slab third starts on faces of the boxes the device's division-free tests read: in
        # the node's frame (the device's own expression) the origin's coordinate on a zero axis
        # of the direction is the face, or the double next to it, so (face - o) * (1 / 0) is
        # 0 * inf there; both kinds of box, every offset and every axis occur
        sb = rc.slab_boxes(name)
        org, meta = rays["org"][rays["slab"]], rays["slab_meta"]
        dd = d[rays["slab"]]
        for o, di, (bi, a, side, ulp) in zip(org, dd, meta):
            row = sb[bi]
            f = row[2 + 3 * side + a]
            want = f if ulp == 0 else np.nextafter(f, np.inf * ulp)
            assert rc.to_node(row, o)[a] == want and di[a] == 0.0
        assert set(meta[:, 3]) == {-1, 0, 1} and set(meta[:, 1]) == {0, 1, 2}
        assert (meta[:, 3] == 0).sum() >= 200
        kinds = set(sb[meta[:, 0], 0])
        assert 0.0 in kinds and (1.0 in kinds) == bool((sb[:, 0] == 1.0).any())
    if cls == "leaving":
        rehit = (hit != 0) & (t < 1e-5)
        print(f"  re-hit at t < 1e-5: {rehit.mean():.3f}")
        assert rehit.mean() >= 0.30
        # the origins are the oracle's hit points of the seed rays, bit for bit
        sh, _t, sp, _n, _m = oracle_lib.intersect(rc.scene_path(name), rays["seed_org"],
                                                  rays["seed_dir"])
        assert sh.all()
        np.testing.assert_array_equal(sp, rays["org"])
    if cls == "edges" and len(rc.geometry(name).tris):
        # (box.scn has corners and edges but no triangle: nothing to tie there)
        ex = rays["exact"]
        ties = oracle_lib.tri_ties(rc.scene_path(name), rays["org"][ex], rays["dir"][ex])
        print(f"  exact-target rays with two triangles at equal t: {(ties >= 2).mean():.3f}")
        assert (ties >= 2).mean() >= 0.25


@pytest.mark.parametrize("cls,key", rc.ILLUM_CASES)
def test_illum_class(cls, key):
    rays = rc.illum_rays(cls, key)
    _same(rays, rc.ILLUM_CLASSES[cls].__wrapped__(key))
    n = len(rays["p_scene"])
    assert 2000 <= n <= 10000
    lit = oracle_lib.illum_test(rc.scene_path(rc.illum_scene(key)), rays["p_scene"],
                                rays["p_light"])
    print(f"{cls} {key}: {n} rays, lit {lit.mean():.3f}")
    _g, li, L = rc._light(key)
    if L is not None:
        r = rays["r12"]
        if L["kind"] == "area":
            assert (np.hypot(r[:, 0], r[:, 1]) <= 1.0 + 1e-12).mean() > 0.8
        else:
            assert np.abs(r).max() <= 0.5
        if cls != "offsets":  # corners and edges of the range
            assert (np.abs(r) == (1.0 if L["kind"] == "area" else 0.5)).any(0).all()
    if cls == "offsets":
        s = rays["s"]
        base = lit[s == 0.0]
        assert 0.1 <= base.mean() <= 0.95  # both verdicts at s = 0, in every scene
        for v in rc.OFFSETS:
            f = lit[s == v]
            if abs(v) < 1.0:
                assert f.sum() == base.sum(), v
            elif abs(v) >= 1.01:
                assert f.sum() == 0, v


def test_illum_classes_give_both_verdicts():
    for cls in rc.ILLUM_CLASSES:
        lit = np.concatenate([
            oracle_lib.illum_test(rc.scene_path(rc.illum_scene(k)), rc.illum_rays(c, k)["p_scene"],
                                  rc.illum_rays(c, k)["p_light"])
            for c, k in rc.ILLUM_CASES if c == cls])
        assert 0.05 <= lit.mean() <= 0.95, (cls, lit.mean())


def test_nested_fixture_is_what_it_claims():
    """nested.scn: more than 64 elements (one per node and material), a scale of 3 over a scale
    of 0.7 under a rotation, two coplanar triangles in the innermost node; nested_rigid.scn: no
    scale, a rect light and an area light."""
    text = open(rc.scene_path("nested.scn")).read()
    assert text.count("\nsphere ") + text.count("\n  ") > 64
    mats = {ln.split()[1] for ln in text.splitlines() if ln.split() and ln.split()[0] in
            ("sphere", "tri", "box", "mesh")}
    assert len(mats) > 64
    g = rc.geometry("nested.scn")
    a, b = g.tris[-2], g.tris[-1]  # the coplanar pair comes last in its node
    na = np.cross(a[1] - a[0], a[2] - a[0])
    assert np.abs((b - a[0]) @ na).max() < 1e-12 * np.linalg.norm(na)
    kinds = [L["kind"] for L in rc.geometry("nested_rigid.scn").lights]
    assert kinds == ["rect", "area"]


def _in_tri(tri, p):
    n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    n /= np.linalg.norm(n)
    ok = np.abs((p - tri[0]) @ n) < 1e-6
    for i in range(3):
        e = tri[(i + 1) % 3] - tri[i]
        ok &= np.cross(e, p - tri[i]) @ n > 1e-6 * np.linalg.norm(e)
    return ok


def test_rays_reach_the_coplanar_pair():
    """The overlap of nested.scn's two coplanar triangles (two elements of one node under the
    scales) is hit, strictly inside both, by at least 100 rays of the walk classes, and every one
    of them takes the first triangle's material: the tie at equal t that the device's walk has to
    give to the earlier element."""
    name = "nested.scn"
    g = rc.geometry(name)
    a, b = g.tris[-2], g.tris[-1]
    only_a = a[0] * 0.8 + a[1] * 0.05 + a[2] * 0.15  # in the first triangle, outside the second
    assert _in_tri(a, only_a[None])[0] and not _in_tri(b, only_a[None])[0]
    org = only_a + np.array([0.3, 0.4, 5.0])
    h, _t, p, _n, m = oracle_lib.intersect(rc.scene_path(name), org[None], rc.unit(only_a - org)[None])
    assert h[0] and np.abs(p[0] - only_a).max() < 1e-9
    first = m[0]
    total = 0
    for cls, scenes in rc.WALK_CLASSES.items():
        if name not in scenes[1]:
            continue
        h, _t, p, _n, m = rc.oracle_walk(cls, name)
        k = (h != 0) & _in_tri(a, p) & _in_tri(b, p)
        total += int(k.sum())
        assert (m[k] == first).all()
    print(f"rays in the overlap: {total}")
    assert total >= 100
