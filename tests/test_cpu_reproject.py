"""The numpy restatement of the reprojection across views (tests/reproject_ref.py): its
properties on synthetic frames whose answer is known by construction, and its purpose on
accumulated oracle frames of two cameras. No GPU: the device kernel is compared with the same
restatement in tests/test_gpu_reproject.py.

Synthetic frames: a camera at `eye` looking along +z with far_right = (0.5, 0, 0) and far_up =
(0, 0.5, 0) at focus 1, 16 x 8 pixels. A plane z = 4 then has a pixel footprint of exactly 0.25 in
x, so a sideways move of k * 0.25 shifts the frame by k pixels.
"""
import functools
import os

import numpy as np
import pytest

import adaptive_ref as ar
import camera_cases
import denoise_ref
import feature_cases as fc
import oracle_lib
import reproject_ref as rp
from gpu_util import scene

W, H = 16, 8
FOOT = 0.25


def front_view(eye=(0.0, 0.0, 0.0), towards_z=1.0):
    e = np.array(eye, dtype=np.float64)
    return rp.View(e, e + np.array([0.0, 0.0, towards_z]), np.array([0.5, 0.0, 0.0]),
                   np.array([0.0, 0.5, 0.0]))


def plane_planes(view, z_of, normal=(0.0, 0.0, -1.0), albedo=(0.5, 0.5, 0.5), w=W, h=H):
    """Planes of a frame whose pixel (x, y) sees the surface z = z_of(direction) along its centre
    ray: depth = distance from the eye; normal and albedo constant."""
    d = rp.pixel_rays(view, w, h)
    z = z_of(d)
    f = np.zeros((h, w), dtype=rp.FEATURE_DTYPE)
    f["depth"] = (z - view.eye[2]) / d[2]
    f["normal"] = normal
    f["albedo"] = albedo
    f["coverage"] = 1.0
    return f


def flat(z):
    return lambda d: np.full(d[2].shape, z)


def random_accum(seed=3, lo=2, hi=20, w=W, h=H):
    rng = np.random.default_rng(seed)
    acc = ar.Accum((h, w))
    acc.mu = 3.0 * rng.random((h, w, 3))
    acc.A = rng.random((h, w, 3))
    acc.n = rng.integers(lo, hi, (h, w)).astype(np.int64)
    return acc


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def test_defaults_are_the_documented_ones():
    assert rp.DEFAULTS == dict(max_history=32, depth_tol=0.02, normal_min=0.9, albedo_tol=0.05)
    assert rp.MIN_WEIGHT == 1.0 / 1024.0


@pytest.mark.parametrize("k", [1, 3])
def test_sideways_move_by_k_pixels_shifts_the_history(k):
    acc = random_accum()
    a, b = front_view(), front_view((k * FOOT, 0.0, 0.0))
    pa, pb = plane_planes(a, flat(4.0)), plane_planes(b, flat(4.0))
    out, st, taps = rp.reproject(acc, a, pa, b, pb)
    assert (taps[:, :W - k] == 1).all() and (taps[:, W - k:] == 0).all()
    np.testing.assert_array_equal(out.n[:, :W - k], np.minimum(acc.n[:, k:], 32))
    assert (out.n[:, W - k:] == 0).all() and not out.mu[:, W - k:].any() and not out.A[:, W - k:].any()
    assert rel(out.mu[:, :W - k], acc.mu[:, k:]) <= 1e-12
    assert st == dict(kept_pixels=(W - k) * H, reset_pixels=k * H, kept_samples=int(out.n.sum()))


def test_identity_keeps_every_covered_pixel_through_one_tap():
    acc = random_accum(lo=2, hi=60)
    a = front_view()
    pa = plane_planes(a, flat(4.0))
    pa["coverage"][2:4, 5:9] = 0.0
    covered = pa["coverage"] > 0
    out, st, taps = rp.reproject(acc, a, pa, a, pa)
    # u is the pixel's own index within rounding: the neighbour's weight is ~1e-16, below 2^-10
    assert (taps[covered] == 1).all() and (taps[~covered] == 0).all()
    np.testing.assert_array_equal(out.n[covered], np.minimum(acc.n[covered], 32))
    assert (acc.n[covered] > 32).any() and (acc.n[covered] < 32).any()
    assert rel(out.mu[covered], acc.mu[covered]) <= 1e-12
    assert not out.n[~covered].any() and not out.mu[~covered].any()
    assert st["kept_pixels"] == int(covered.sum()) and st["reset_pixels"] == int((~covered).sum())


def step_scene(view):
    """A near plane z = 2 over world x < 0.3 in front of a far plane z = 4."""
    def z_of(d):
        x_near = view.eye[0] + d[0] * ((2.0 - view.eye[2]) / d[2])
        return np.where(x_near < 0.3, 2.0, 4.0)
    return z_of


def test_depth_step_resets_what_the_previous_view_did_not_see():
    """The camera moves right by two far-plane pixels: each far pixel of the new frame lands on the
    centre of a previous pixel, which saw either the same point (kept) or the near plane in front
    of it (reset: the depth stop)."""
    acc = random_accum()
    a, b = front_view(), front_view((2 * FOOT, 0.0, 0.0))
    pa, pb = plane_planes(a, step_scene(a)), plane_planes(b, step_scene(b))
    out, _st, _taps = rp.reproject(acc, a, pa, b, pb)
    far = pb["depth"] > 3.0
    d = rp.pixel_rays(b, W, H)
    X = [b.eye[k] + d[k] * pb["depth"].astype(np.float64) for k in range(3)]
    # the previous eye's segment to X crosses z = 2 at this x: occluded when left of the edge
    x_cross = a.eye[0] + (X[0] - a.eye[0]) * ((2.0 - a.eye[2]) / (X[2] - a.eye[2]))
    _a, u, _t, _r = rp.project(a, X, W, H)
    outside = np.rint(u) > W - 1
    occluded = far & (x_cross < 0.3)
    assert occluded.any() and (far & ~occluded & ~outside).any() and (~far).any()
    np.testing.assert_array_equal(out.n[far] == 0, (occluded | outside)[far])
    assert (out.n[~far] >= 2).all()                    # the near plane was seen before


def tilted(planes, deg):
    out = planes.copy()
    t = np.radians(deg)
    out["normal"] = (np.sin(t), 0.0, -np.cos(t))
    return out


def test_each_stop_resets_a_pixel_the_defaults_keep():
    """depth_tol, normal_min and albedo_tol tightened; max_history, the fourth parameter, cannot
    reset a pixel: tightened it lowers the carried count."""
    acc = random_accum(lo=8, hi=20)
    a = front_view()
    pa = plane_planes(a, flat(4.0))
    cur = tilted(pa, 10.0)                              # cos 10 deg = 0.985
    cur["albedo"] = (0.5, 0.53, 0.5)
    kept = rp.reproject(acc, a, pa, a, cur)[0].n
    assert (kept >= 8).all()
    assert not rp.reproject(acc, a, pa, a, cur, normal_min=0.99)[0].n.any()
    assert not rp.reproject(acc, a, pa, a, cur, albedo_tol=0.01)[0].n.any()
    # the reprojected distance and the float32 depth plane differ in their last bits
    n0 = rp.reproject(acc, a, pa, a, cur, depth_tol=0.0)[0].n
    assert (n0 == 0).any()
    n4 = rp.reproject(acc, a, pa, a, cur, max_history=4)[0].n
    assert (n4 == 4).all()


def test_point_behind_the_previous_camera_has_no_history():
    acc = random_accum()
    b = front_view()
    back = front_view(towards_z=-1.0)                   # the previous camera looked the other way
    pb = plane_planes(b, flat(4.0))
    out, st, _taps = rp.reproject(acc, back, pb, b, pb)
    assert not out.n.any() and st["kept_pixels"] == 0


def test_point_outside_the_previous_frame_has_no_history():
    acc = random_accum()
    a, b = front_view(), front_view((W * FOOT + 1.0, 0.0, 0.0))
    out, _st, _taps = rp.reproject(acc, a, plane_planes(a, flat(4.0)), b, plane_planes(b, flat(4.0)))
    assert not out.n.any()


def test_single_sample_source_gives_no_history():
    acc = random_accum()
    acc.n[3, 7] = 1
    a = front_view()
    pa = plane_planes(a, flat(4.0))
    out, _st, _taps = rp.reproject(acc, a, pa, a, pa)
    assert out.n[3, 7] == 0 and (np.delete(out.n.ravel(), 3 * W + 7) >= 2).all()


def test_capped_count_keeps_the_variance_of_a_single_sample():
    acc = random_accum(lo=10, hi=40)
    a = front_view()
    pa = plane_planes(a, flat(4.0))
    out, st, _taps = rp.reproject(acc, a, pa, a, pa, max_history=6)
    assert (out.n == 6).all()
    s2_old = acc.A / (acc.n - 1).astype(np.float64)[..., None]
    assert rel(out.A / 5.0, s2_old) <= 1e-12
    assert st["kept_samples"] == 6 * W * H


def test_kept_samples_is_the_sum_of_the_new_counts():
    acc = random_accum()
    a, b = front_view(), front_view((3 * FOOT, FOOT, 0.0))
    out, st, _taps = rp.reproject(acc, a, plane_planes(a, flat(4.0)), b, plane_planes(b, flat(4.0)))
    assert 0 < st["kept_pixels"] < W * H
    assert st["kept_samples"] == int(out.n.sum()) and st["kept_pixels"] == int((out.n > 0).sum())
    assert st["kept_pixels"] + st["reset_pixels"] == W * H


def test_view_of_is_the_frame_the_rays_come_from():
    """The oracle's camera rays at aa 0 (through the cell corners: camera_ray's dx = 2 (i - W / 2) /
    W) from view_of's frame."""
    args = [camera_cases.dimmed_cornell(), "/tmp/x.png", "-resolution", "7", "5", "-aa", "0"]
    rays, _ids = oracle_lib.camera_rays(args)
    v = rp.view_of(camera_cases.CORNELL_FILE_CAMERA, oracle_lib.parse_args(args)[1].focus_depth)
    ys, xs = np.mgrid[0:5, 0:7]
    dx = 2.0 * (xs - 7 // 2) / 7.0
    dy = 2.0 * (ys - 5 // 2) / 5.0
    D = np.stack([((v.far_org[k] + v.far_right[k] * dx) + v.far_up[k] * dy) - v.eye[k]
                  for k in range(3)], axis=-1)
    D /= np.sqrt((D * D).sum(-1))[..., None]
    assert np.abs(D.reshape(-1, 3) - rays["dir"]).max() <= 1e-12


# ---- quality on accumulated oracle frames: the purpose ----------------------------------------
CAMERA_A = camera_cases.CASES["cornell_dim"][1]
OFFSET_X = 0.15


def camera_b_line():
    v = CAMERA_A.split()
    v[0] = repr(float(v[0]) + OFFSET_X)
    return " ".join(v)


def view_args(line, sub, tail):
    d = os.path.join(camera_cases.tmp_dir(), sub)
    os.makedirs(d, exist_ok=True)
    path = camera_cases.rewrite_scene(camera_cases.dimmed_cornell(), line, d)
    return [path, "/tmp/x.png"] + fc.QUALITY_FLAGS + tail


def oracle_planes(args):
    w, h = fc.QUALITY_W, fc.QUALITY_H
    rays, _ids = oracle_lib.camera_rays(args)
    hit, _t, p, n, m = oracle_lib.intersect(args[0], rays["org"], rays["dir"])
    depth = oracle_lib.math("sqrt", denoise_ref.sample_depth(rays["org"], p))
    with open(scene("cornell.scn")) as f:
        table = np.array([[float(x) for x in ln.split()[4:7]] for ln in f
                          if ln.lstrip().startswith("material")])
    assert m[hit != 0].max() < len(table)
    return fc.planes((hit != 0, n, depth, m), w, h, 1, table)


@functools.lru_cache(maxsize=None)
def quality_fixture():
    """Dimmed cornell, 48 x 32, aa 0. View A: the cornell_dim camera, eight -it 4 passes under
    seeds 1..8; view B: the eye moved by +0.15 in x, two -it 4 passes under seeds 11, 12 and the
    converged -it 256 -seed 99 frame; both views' planes from the oracle's own intersections and
    their pinhole frames from view_of."""
    w, h = fc.QUALITY_W, fc.QUALITY_H
    line_b = camera_b_line()
    a_passes = [oracle_lib.render_float(view_args(CAMERA_A, "reproject_a", ["-it", "4", "-seed", str(s)]), w, h)[0]
                for s in range(1, 9)]
    b_passes = [oracle_lib.render_float(view_args(line_b, "reproject_b", ["-it", "4", "-seed", str(s)]), w, h)[0]
                for s in (11, 12)]
    conv = oracle_lib.render_float(view_args(line_b, "reproject_b", ["-it", "256", "-seed", "99"]), w, h)[0]
    args_a = view_args(CAMERA_A, "reproject_a", ["-it", "4", "-seed", "1"])
    args_b = view_args(line_b, "reproject_b", ["-it", "4", "-seed", "1"])
    focus = oracle_lib.parse_args(args_a)[1].focus_depth
    view_a = rp.view_of(camera_cases.camera_of(CAMERA_A), focus)
    view_b = rp.view_of(camera_cases.camera_of(line_b), focus)
    return a_passes, b_passes, conv, oracle_planes(args_a), oracle_planes(args_b), view_a, view_b


def fold(acc, frames):
    for f in frames:
        acc.add(f.astype(np.float64), np.zeros(f.shape), 1)
    return acc


def test_quality_history_from_another_view_beats_starting_over():
    """One sample per pixel and pass (S = 1, M2 = 0); RMSE to the converged frame of view B of (a)
    two passes of B alone and (b) eight passes of A reprojected with the defaults plus the same
    two passes of B. The offset is the issue's first choice, +0.15 in x; it meets the three fixture
    conditions (89.6 % of B's covered pixels kept, 10.4 % reset, 1.8 % of the converged values >= 1).
    Recorded (DESIGN.md "Reprojection across views"), (a) / (b): all pixels 0.0774 / 0.0359, kept
    pixels 0.0896 / 0.0380, reset pixels 0.0299 / 0.0299."""
    a_passes, b_passes, conv, feat_a, feat_b, view_a, view_b = quality_fixture()
    shape = (fc.QUALITY_H, fc.QUALITY_W)
    alone = fold(ar.Accum(shape), b_passes)
    carried, st, _taps = rp.reproject(fold(ar.Accum(shape), a_passes), view_a, feat_a, view_b, feat_b)
    kept = carried.n > 0
    covered = feat_b["coverage"] > 0
    fold(carried, b_passes)
    share_kept = float(kept[covered].mean())
    share_reset = float((~kept)[covered].mean())
    share_clamped = float((conv >= 1.0).mean())
    e_a, e_b = fc.rmse(alone.mu, conv), fc.rmse(carried.mu, conv)
    k_a, k_b = fc.rmse(alone.mu[kept], conv[kept]), fc.rmse(carried.mu[kept], conv[kept])
    r_a, r_b = fc.rmse(alone.mu[~kept], conv[~kept]), fc.rmse(carried.mu[~kept], conv[~kept])
    print(f"kept {100 * share_kept:.1f} %, reset {100 * share_reset:.1f} % of B's covered pixels; "
          f"values >= 1 in the converged frame {100 * share_clamped:.1f} %; stats {st}")
    print(f"rmse to the converged frame, B alone / with A's history: all pixels {e_a:.4f} / "
          f"{e_b:.4f}, kept pixels {k_a:.4f} / {k_b:.4f}, reset pixels {r_a:.4f} / {r_b:.4f}")
    # the fixture conditions, on the oracle and the restatement alone
    assert share_kept >= 0.60
    assert share_reset >= 0.03
    assert share_clamped <= 0.10
    assert e_b < e_a
    assert k_b < k_a
