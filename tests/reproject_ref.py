"""numpy restatement of the reprojection across views of gi.h ("reprojection across views"): the
accumulator carried from one pinhole camera into another. fp64 on the given values, one IEEE
operation per step in the order gi.h writes, sums and dot products left to right. Builds on the
accumulator restatements (adaptive_ref.Accum: radiance_ref.Accum with one count per pixel, which
a reprojected accumulator needs). The device kernel (gi_radiance.hip accum_reproject_kernel) is
compared with it bit for bit in tests/test_gpu_reproject.py. Also view_of: the pinhole frame of a
camera in numpy (gi_get_view returns the host's own bits; this one agrees within rounding).
"""
import collections

import numpy as np

import adaptive_ref as ar
from denoise_ref import FEATURE_DTYPE

DEFAULTS = dict(max_history=32, depth_tol=0.02, normal_min=0.9, albedo_tol=0.05)
MIN_WEIGHT = 2.0 ** -10

View = collections.namedtuple("View", "eye far_org far_right far_up")


def as_view(v):
    """A View of float64 [3] arrays from a View, a gi_amd.View or anything with the four fields."""
    return View(*(np.array([float(x) for x in getattr(v, f)]) for f in View._fields))


def view_of(camera, focus_depth):
    """The pinhole frame of camera = (eye, towards, up, xfov) as the host builds it (R3Triad axes:
    z = -towards / |towards|, right = up x z normalised, up = z x right; yfov = xfov):
    far_org = eye + towards * focus_depth, far_right = right * tan(xfov) * focus_depth, far_up
    likewise."""
    eye, towards, up, xfov = camera
    eye, towards, up = (np.asarray(a, dtype=np.float64) for a in (eye, towards, up))
    z = -towards / np.sqrt(towards @ towards)
    x = np.cross(up, z)
    x = x / np.sqrt(x @ x)
    y = np.cross(z, x)
    t = np.tan(xfov)
    return View(eye, eye + (-z) * focus_depth, x * t * focus_depth, y * t * focus_depth)


def dot(a, b):
    """(a0 b0 + a1 b1) + a2 b2 of two triples of arrays or scalars."""
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def pixel_rays(view, w, h):
    """Unit directions through the pixel centres [3][H, W]: steps 2 of the definition."""
    v = as_view(view)
    ys, xs = np.mgrid[0:h, 0:w]
    dx = (2 * xs + 1 - w).astype(np.float64) / float(w)
    dy = (2 * ys + 1 - h).astype(np.float64) / float(h)
    D = [((v.far_org[k] + v.far_right[k] * dx) + v.far_up[k] * dy) - v.eye[k] for k in range(3)]
    ln = np.sqrt(dot(D, D))
    safe = np.where(ln == 0.0, 1.0, ln)
    return [np.where(ln == 0.0, D[k], D[k] / safe) for k in range(3)]


def project(prev_view, X, w, h):
    """Steps 4: points X [3][...] into the previous camera: (a, u, t, r)."""
    v0 = as_view(prev_view)
    v = [X[k] - v0.eye[k] for k in range(3)]
    G = [v0.far_org[k] - v0.eye[k] for k in range(3)]
    with np.errstate(all="ignore"):
        a = dot(v, G) / dot(G, G)
        sx = (dot(v, v0.far_right) / dot(v0.far_right, v0.far_right)) / a
        sy = (dot(v, v0.far_up) / dot(v0.far_up, v0.far_up)) / a
        u = ((sx + 1.0) * float(w)) * 0.5 - 0.5
        t = ((sy + 1.0) * float(h)) * 0.5 - 0.5
    return a, u, t, np.sqrt(dot(v, v))


def reproject(acc, prev_view, prev_feat, cur_view, cur_feat, **params):
    """gi_accum_reproject of an adaptive_ref.Accum seen from prev_view (planes prev_feat) into
    cur_view (planes cur_feat). Returns (the new Accum, stats dict kept_pixels / reset_pixels /
    kept_samples, taps [H, W]: how many taps counted at each pixel)."""
    P = dict(DEFAULTS)
    for k, val in params.items():
        assert k in DEFAULTS, k
        P[k] = val
    h, w = acc.n.shape
    prev_feat = np.ascontiguousarray(prev_feat, dtype=FEATURE_DTYPE)
    cur_feat = np.ascontiguousarray(cur_feat, dtype=FEATURE_DTYPE)
    assert prev_feat.shape == (h, w) and cur_feat.shape == (h, w)
    v1 = as_view(cur_view)
    d = pixel_rays(v1, w, h)
    z = cur_feat["depth"].astype(np.float64)
    X = [v1.eye[k] + d[k] * z for k in range(3)]
    a, u, t, r = project(prev_view, X, w, h)
    with np.errstate(all="ignore"):
        ok = (cur_feat["coverage"] != 0) & (a > 0.0)
        x0, y0 = np.floor(u), np.floor(t)
        fx, fy = u - x0, t - y0
    n_p = [cur_feat["normal"][..., k].astype(np.float64) for k in range(3)]
    a_p = [cur_feat["albedo"][..., k].astype(np.float64) for k in range(3)]
    npp = dot(n_p, n_p)
    nm2 = P["normal_min"] * P["normal_min"]
    at2 = P["albedo_tol"] * P["albedo_tol"]
    hs = np.zeros((h, w))
    sm = np.zeros((h, w, 3))
    sv = np.zeros((h, w, 3))
    nmin = np.full((h, w), np.iinfo(np.int64).max, dtype=np.int64)
    taps = np.zeros((h, w), dtype=np.int64)
    for j in (0, 1):
        for i in (0, 1):
            with np.errstate(all="ignore"):
                tx, ty = x0 + float(i), y0 + float(j)
                cnt = ok & (tx >= 0.0) & (tx <= float(w) - 1.0) & (ty >= 0.0) & (ty <= float(h) - 1.0)
                hh = (fx if i else 1.0 - fx) * (fy if j else 1.0 - fy)
                cnt &= hh >= MIN_WEIGHT
            qx = np.where(cnt, tx, 0.0).astype(np.int64)
            qy = np.where(cnt, ty, 0.0).astype(np.int64)
            nq = acc.n[qy, qx]
            cnt &= nq >= 2
            pf = prev_feat[qy, qx]
            cnt &= pf["coverage"] > 0
            with np.errstate(all="ignore"):
                cnt &= np.abs(r - pf["depth"].astype(np.float64)) <= P["depth_tol"] * r
                n_q = [pf["normal"][..., k].astype(np.float64) for k in range(3)]
                c = dot(n_p, n_q)
                cnt &= (c > 0.0) & (c * c >= ((nm2 * npp) * dot(n_q, n_q)))
                e = [a_p[k] - pf["albedo"][..., k].astype(np.float64) for k in range(3)]
                cnt &= dot(e, e) <= at2
                q1 = (np.where(nq >= 2, nq, 2) - 1).astype(np.float64)
                hh = np.where(cnt, hh, 0.0)
                hs = np.where(cnt, hs + hh, hs)
                sm = np.where(cnt[..., None], sm + hh[..., None] * acc.mu[qy, qx], sm)
                sv = np.where(cnt[..., None], sv + hh[..., None] * (acc.A[qy, qx] / q1[..., None]), sv)
            nmin = np.where(cnt, np.minimum(nmin, nq), nmin)
            taps += cnt
    kept = taps > 0
    out = ar.Accum((h, w))
    out.n = np.where(kept, np.minimum(nmin, np.int64(P["max_history"])), 0).astype(np.int64)
    hs1 = np.where(kept, hs, 1.0)[..., None]
    n1 = (out.n - 1).astype(np.float64)[..., None]
    out.mu = np.where(kept[..., None], sm / hs1, 0.0)
    out.A = np.where(kept[..., None], (sv / hs1) * n1, 0.0)
    stats = dict(kept_pixels=int(kept.sum()), reset_pixels=int((~kept).sum()),
                 kept_samples=int(out.n.sum()))
    return out, stats, taps
