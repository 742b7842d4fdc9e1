"""Edge-case rays for the scene walk and the shadow test, shared by tests/test_cpu_ray_edges.py
(the oracle alone: are the classes what they claim to be?) and tests/test_gpu_ray_edges.py (the
device against the oracle). Seeded and pure numpy; geometry comes from a small .scn / .off parser
below, hit points ("seeds") from random rays cast through the oracle.

Classes for the scene walk (gi_intersect_probe), each a dict of arrays with "org" and "dir":
  axis      one or two direction components zero (+0.0 and -0.0): a third aimed at seeds, a
            third with the origin's zero-axis coordinate copied from a shape's or triangle's box
            face, a third with it on a face of a box the division-free slab tests read (the
            loader's grown element boxes and mesh hierarchy boxes), exactly or one ulp to either
            side: 0 * inf there
  edges     rays aimed at mesh vertices, edge midpoints and face diagonals, box corners and edges,
            exactly and +-1e-7, 1e-6, 1e-5 across
  leaving   origin = a seed hit point bit for bit; direction random, mirrored or tangent
  tangent   rays passing a sphere / cylinder axis at r (1 +- {0, 1e-9, 1e-7, 1e-6, 1e-5}) and at
            r +- about 1e-6; rays nearly in a triangle's or circle's plane, n . d on both sides of
            1e-6
Classes for the shadow test (gi_illum_probe), dicts with "p_scene", "light", "r12", "p_light":
  offsets   a seed moved along the light ray by s * 1e-6, s in OFFSETS
  coeffs    sample coefficients uniform, and on the corners and edges of their range
  thin      points where an occluder ends within 1e-5 of the shaded point
"""
import functools
import os

import numpy as np

import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-6  # RN_EPSILON


def scene_path(name):
    for d in ("scenes", "scenes_extra"):
        p = os.path.join(ROOT, "tests", d, name)
        if os.path.exists(p):
            return p
    raise FileNotFoundError(name)


# ---------------------------------------------------------------------------------------------
# a small .scn / .off parser: world-space geometry only
# ---------------------------------------------------------------------------------------------
def read_off(path):
    """(vertices [nv, 3], faces: list of vertex-index lists)."""
    tok = open(path).read().split()
    assert tok[0] == "OFF", path
    nv, nf = int(tok[1]), int(tok[2])
    v = np.array(tok[4:4 + 3 * nv], dtype=np.float64).reshape(nv, 3)
    faces, k = [], 4 + 3 * nv
    for _ in range(nf):
        m = int(tok[k])
        faces.append([int(x) for x in tok[k + 1:k + 1 + m]])
        k += 1 + m
    return v, faces


class Geometry:
    """World-space shapes of a scene file. tris [n, 3, 3]; edges [n, 2, 3] (every polygon edge and
    fan diagonal of meshes, every edge of `tri` shapes, the 12 edges of boxes); verts [n, 3];
    edge_c / vert_c: the centre of the edge's / vertex's mesh, box or triangle;
    boxes [n, 2, 3] (world corners lo / hi of untransformed-axis boxes: shapes' and triangles'
    boxes under identity or translation nodes); spheres [(c, r)]; cyls [(p1, p2, r)]; circles
    [(c, n, r)]; lights [dict]."""

    def __init__(self):
        self.tris, self.edges, self.verts, self.boxes = [], [], [], []
        self.edge_c, self.vert_c = [], []  # per edge / vertex: the centre of its object
        self.spheres, self.cyls, self.circles, self.lights = [], [], [], []


def _apply(M, p):
    p = np.asarray(p, dtype=np.float64)
    return p @ M[:3, :3].T + M[:3, 3]


@functools.lru_cache(maxsize=None)
def geometry(name):
    path = scene_path(name)
    g = Geometry()
    tok = []
    for ln in open(path):
        tok += ln.split("#")[0].split()
    stack = [np.eye(4)]
    k = 0

    def take(n):
        nonlocal k
        out = tok[k:k + n]
        k += n
        return out

    def fl(n):
        return np.array(take(n), dtype=np.float64)

    def add_box(lo, hi, M):
        # only where the node's axes are the world's (identity or translation)
        if np.array_equal(M[:3, :3], np.eye(3)):
            g.boxes.append(np.stack([lo + M[:3, 3], hi + M[:3, 3]]))

    def add_tri(p, M):
        w = _apply(M, p)
        g.tris.append(w)
        add_box(p.min(0), p.max(0), M)

    while k < len(tok):
        cmd = take(1)[0]
        M = stack[-1]
        if cmd == "tri":
            take(1)
            p = fl(9).reshape(3, 3)
            add_tri(p, M)
            w = _apply(M, p)
            g.verts += list(w)
            g.edges += [np.stack([w[i], w[(i + 1) % 3]]) for i in range(3)]
            g.vert_c += [w.mean(0)] * 3
            g.edge_c += [w.mean(0)] * 3
        elif cmd == "box":
            take(1)
            v = fl(6)
            lo, hi = np.minimum(v[:3], v[3:]), np.maximum(v[:3], v[3:])
            add_box(lo, hi, M)
            c = np.array([[(lo, hi)[(i >> a) & 1][a] for a in range(3)] for i in range(8)])
            w = _apply(M, c)
            g.verts += list(w)
            g.vert_c += [w.mean(0)] * 8
            for i in range(8):
                for a in range(3):
                    if not (i >> a) & 1:
                        g.edges.append(np.stack([w[i], w[i | (1 << a)]]))
                        g.edge_c.append(w.mean(0))
        elif cmd == "sphere":
            take(1)
            v = fl(4)
            s = np.linalg.norm(M[:3, 0])
            g.spheres.append((_apply(M, v[:3]), v[3] * s))
            add_box(v[:3] - v[3], v[:3] + v[3], M)
        elif cmd == "circle":
            take(1)
            v = fl(7)
            n = M[:3, :3] @ v[3:6]
            g.circles.append((_apply(M, v[:3]), n / np.linalg.norm(n), v[6] * np.linalg.norm(M[:3, 0])))
        elif cmd in ("cylinder", "cone"):
            take(1)
            v = fl(5)  # centre, radius, height: axis y (R3Scene.cpp:1590-1640)
            c, r, h = v[:3], v[3], v[4]
            g.cyls.append((_apply(M, c - [0, h / 2, 0]), _apply(M, c + [0, h / 2, 0]), r))
        elif cmd == "line":
            take(1)
            v = fl(6)
            g.cyls.append((_apply(M, v[:3]), _apply(M, v[3:]), 1e-3))
        elif cmd == "mesh":
            take(1)
            verts, faces = read_off(os.path.join(os.path.dirname(path), take(1)[0]))
            w = _apply(M, verts)
            g.verts += list(w)
            g.vert_c += [w.mean(0)] * len(w)
            for f in faces:
                for i in range(len(f)):
                    g.edges.append(np.stack([w[f[i]], w[f[(i + 1) % len(f)]]]))
                    g.edge_c.append(w.mean(0))
                for i in range(1, len(f) - 1):
                    add_tri(verts[[f[0], f[i], f[i + 1]]], M)
                    if i > 1:
                        g.edges.append(np.stack([w[f[0]], w[f[i]]]))
                        g.edge_c.append(w.mean(0))
        elif cmd == "begin":
            take(1)
            stack.append(M @ fl(16).reshape(4, 4))
        elif cmd == "end":
            stack.pop()
        elif cmd == "material":
            take(18)
        elif cmd == "camera":
            take(12)
        elif cmd == "dir_light":
            take(6)
            g.lights.append({"kind": "dir"})  # keeps the file's light numbering
        elif cmd == "point_light":
            v = fl(9)
            g.lights.append({"kind": "point", "pos": v[3:6]})
        elif cmd == "spot_light":
            v = fl(14)
            g.lights.append({"kind": "spot", "pos": v[3:6]})
        elif cmd == "area_light":
            v = fl(13)
            n = v[6:9] / np.linalg.norm(v[6:9])
            u = np.array([n[1], -n[0], 0.0])
            if 1.0 - abs(n[2]) < 0.1:
                u = np.array([n[2], 0.0, -n[0]])
            vv = np.cross(u, n)
            g.lights.append({"kind": "area", "pos": v[3:6], "n": n, "su": u / np.linalg.norm(u) * v[9],
                             "sv": vv / np.linalg.norm(vv) * v[9]})
        elif cmd == "rect_light":
            v = fl(17)
            a1, a2 = v[6:9] / np.linalg.norm(v[6:9]), v[9:12] / np.linalg.norm(v[9:12])
            n = np.cross(a1, a2)
            g.lights.append({"kind": "rect", "pos": v[3:6], "n": n / np.linalg.norm(n),
                             "su": a1 * v[12], "sv": a2 * v[13]})
        elif cmd in ("background", "ambient"):
            take(3)
        else:
            raise ValueError(f"{path}: command {cmd}")
    for a in ("tris", "edges", "verts", "boxes", "edge_c", "vert_c"):
        v = getattr(g, a)
        setattr(g, a, np.array(v) if v else np.zeros((0,)))
    pts = [g.verts] if len(g.verts) else []
    pts += [np.stack([c - r, c + r]) for c, r in g.spheres]
    pts += [np.stack([p1 - r, p1 + r, p2 - r, p2 + r]) for p1, p2, r in g.cyls]
    pts = np.concatenate(pts)
    g.lo, g.hi = pts.min(0), pts.max(0)
    g.centre = (g.lo + g.hi) / 2
    g.radius = np.linalg.norm(g.hi - g.lo) / 2
    return g


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def perp(d, rng):
    """A random unit vector perpendicular to each row of d."""
    r = rng.normal(size=d.shape)
    r -= (r * d).sum(-1, keepdims=True) * d
    return unit(r)


def _rays(org, d):
    org = np.ascontiguousarray(org, dtype=np.float64)
    d = np.ascontiguousarray(d, dtype=np.float64)
    return {"org": org, "dir": d}


# ---------------------------------------------------------------------------------------------
# seeds
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seeds(name, n=1500, seed=1, spread=0.5):
    """Random rays that hit: (org, dir, point, normal), the oracle's hit points. Origins normal
    around the scene's centre with deviation spread * radius. Read-only."""
    g = geometry(name)
    rng = np.random.default_rng(seed)
    parts, got = [], 0
    for _ in range(60):
        org = g.centre + rng.normal(size=(4 * n, 3)) * g.radius * spread
        d = unit(rng.normal(size=(4 * n, 3)))
        h, _t, p, nr, _m = oracle_lib.intersect(scene_path(name), org, d)
        k = np.flatnonzero(h)
        parts.append((org[k], d[k], p[k], nr[k]))
        got += len(k)
        if got >= n:
            break
    out = tuple(np.concatenate([q[i] for q in parts])[:n] for i in range(4))
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------
# classes for the scene walk
# ---------------------------------------------------------------------------------------------
AXIS_SCENES = ("cornell.scn", "jensen.scn", "box.scn", "stilllife.scn", "teapot.scn",
               "cylinder.scn", "transform.scn", "nested.scn")
# (transform.scn holds spheres only: no vertex or edge to aim at, so the edges class leaves it out)
EDGE_SCENES = ("box.scn", "ico.scn", "teapot.scn", "stilllife.scn", "cornell.scn", "nested.scn")
LEAVING_SCENES = ("cornell.scn", "jensen.scn", "stilllife.scn", "teapot.scn", "cylinder.scn",
                  "transform.scn", "nested.scn")
TANGENT_SCENES = ("cornell.scn", "transform.scn", "fourspheres.scn", "cylinder.scn", "lines.scn",
                  "circles.scn", "nested.scn")
EDGE_OFFSETS = (0.0, 1e-7, -1e-7, 1e-6, -1e-6, 1e-5, -1e-5)
# distance of the ray from a sphere's centre / a cylinder's axis: r (1 + rel) + add. The relative
# steps straddle the surface; the absolute ones straddle the RN_EPSILON the reference allows
# beyond it (all of a radius-1e-3 `line`'s relative steps lie within that)
RADIAL = [(e, 0.0) for e in (0.0, 1e-9, -1e-9, 1e-7, -1e-7, 1e-6, -1e-6, 1e-5, -1e-5)] + [
    (0.0, a) for a in (0.9e-6, 1.1e-6, -0.9e-6, -1.1e-6, 2e-6, 1e-5, 1e-4)]
DENOMS = (0.0, 0.5e-6, -0.5e-6, 0.99e-6, -0.99e-6, 1.01e-6, -1.01e-6, 2e-6, -2e-6, 1e-4, -1e-4)


def _axis_dirs(n, rng):
    """Unit directions with one or two zero components, the zeros signed at random."""
    d = np.zeros((n, 3))
    ax = rng.integers(0, 3, n)
    two = rng.random(n) < 0.5           # two zero components: +-e_ax
    ang = rng.random(n) * 2 * np.pi
    sgn = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    for i in range(n):
        if two[i]:
            d[i, ax[i]] = sgn[i]
        else:                            # zero component ax, the other two on the unit circle
            d[i, (ax[i] + 1) % 3] = np.cos(ang[i])
            d[i, (ax[i] + 2) % 3] = np.sin(ang[i])
    zero = d == 0.0
    d[zero & (rng.random((n, 3)) < 0.5)] = -0.0
    return d


@functools.lru_cache(maxsize=None)
def slab_boxes(name):
    """The loader's own slab-test boxes (gi_amd.slab_boxes: elements' grown boxes and mesh
    hierarchy boxes, node frame) that lie under at most one transform, and that one without
    rotation: there a world coordinate can be found whose image in the node's frame is a box face
    bit for bit. Read-only."""
    import gi_amd
    b = gi_amd.slab_boxes(scene_path(name))
    T = b[:, 8:20].reshape(-1, 3, 4)
    off = np.abs(T[:, :, :3] * (1 - np.eye(3))).sum((1, 2))
    keep = (b[:, 1] == 1) & (off == 0) & (b[:, 2:5] <= b[:, 5:8]).all(1)
    b = b[keep]
    b.setflags(write=False)
    return b


def to_node(row, w):
    """xf_point(Tinv, w) of gi_device.h for a slab_boxes row: the device's expression, in order."""
    m = row[8:20].reshape(3, 4)
    return ((m[:, 0] * w[0] + m[:, 1] * w[1]) + m[:, 2] * w[2]) + m[:, 3]


def _preimage(row, a, f):
    """A world coordinate on axis a whose image in the row's node frame is f exactly, or None."""
    m = row[8:20].reshape(3, 4)
    x = (f - m[a, 3]) / m[a, a]
    cand = [x]
    for k in range(1, 5):
        lo, hi = cand[0], cand[-1]
        cand = [np.nextafter(lo, -np.inf)] + cand + [np.nextafter(hi, np.inf)]
    w = np.zeros(3)
    for c in sorted(cand, key=lambda c: abs(c - x)):
        w[a] = c
        if to_node(row, w)[a] == f:
            return c
    return None


@functools.lru_cache(maxsize=None)
def axis(name, n=3000, seed=2):
    g = geometry(name)
    rng = np.random.default_rng(seed)
    sb = slab_boxes(name)
    n_slab = n // 3 if len(sb) else 0
    n -= n_slab
    h = n // 2
    # aimed at seeds
    sp = seeds(name)[2]
    tgt = sp[rng.integers(0, len(sp), h)]
    d1 = _axis_dirs(h, rng)
    o1 = tgt - d1 * (g.radius * (0.5 + rng.random((h, 1))))
    # origin on a box face plane of a zero axis
    d2 = _axis_dirs(n - h, rng)
    boxes = g.boxes if len(g.boxes) else np.stack([[g.lo, g.hi]])
    b = boxes[rng.integers(0, len(boxes), n - h)]
    inside = b[:, 0] + rng.random((n - h, 3)) * (b[:, 1] - b[:, 0])
    o2 = inside - d2 * (g.radius * (0.5 + rng.random((n - h, 1))))
    side = rng.integers(0, 2, n - h)
    ulp = rng.integers(-1, 2, n - h)
    for i in range(n - h):
        za = np.flatnonzero(d2[i] == 0.0)
        a = za[rng.integers(0, len(za))]
        c = b[i, side[i], a]
        if ulp[i]:
            c = np.nextafter(c, np.inf * ulp[i])
        o2[i, a] = c
    # origin on a face of a box that a division-free slab test reads (elem_maybe_hit, bvh_box:
    # the grown boxes, not the shapes' own): there (face - o) is 0 and 1 / d is inf, 0 * inf
    d3 = _axis_dirs(n_slab, rng)
    o3 = np.zeros((n_slab, 3))
    meta = np.zeros((n_slab, 4), dtype=np.int64)  # box row, axis, side, ulps off the face
    for i in range(n_slab):
        while True:
            bi = rng.integers(0, len(sb))
            row = sb[bi]
            m = row[8:20].reshape(3, 4)
            lo, hi = row[2:5], row[5:8]
            za = np.flatnonzero(d3[i] == 0.0)
            a = za[rng.integers(0, len(za))]
            side, ulp = rng.integers(0, 2), rng.integers(-1, 2)
            f = (lo, hi)[side][a]
            if ulp:
                f = np.nextafter(f, np.inf * ulp)
            x = _preimage(row, a, f)
            if x is not None:
                break
        inside = lo + rng.random(3) * (hi - lo)
        w = (inside - m[:, 3]) / np.diag(m[:, :3])
        o3[i] = w - d3[i] * np.sign(np.diag(m[:, :3])) * (g.radius * (0.5 + rng.random()))
        o3[i, a] = x
        meta[i] = (bi, a, side, ulp)
    org, d = np.concatenate([o1, o2, o3]), np.concatenate([d1, d2, d3])
    away = rng.random(len(org)) < 0.2   # a fifth of them start there and leave the scene
    d[away] = -d[away]
    out = _rays(org, d)
    out["face"] = (np.arange(len(org)) >= h) & (np.arange(len(org)) < n)
    out["slab"] = np.arange(len(org)) >= n
    out["slab_meta"] = meta
    return out


@functools.lru_cache(maxsize=None)
def edges(name, n_targets=450, seed=3):
    """Targets: vertices, edge midpoints (face diagonals of polygons included). Every target with
    every offset of EDGE_OFFSETS across the edge (for a vertex: across a random direction).
    out["exact"] marks the offset-0 rays."""
    g = geometry(name)
    rng = np.random.default_rng(seed)
    ne = n_targets // 2
    ie, iv = rng.integers(0, len(g.edges), ne), rng.integers(0, len(g.verts), n_targets - ne)
    e, v = g.edges[ie], g.verts[iv]
    tgt = np.concatenate([(e[:, 0] + e[:, 1]) * 0.5, v])
    along = np.concatenate([unit(e[:, 1] - e[:, 0]), unit(rng.normal(size=v.shape))])
    # from the target's side of its object, at a random angle; a third of the rays graze: they
    # pass the target at a right angle to the line from the object's centre
    outward = tgt - np.concatenate([g.edge_c[ie], g.vert_c[iv]])
    size = np.linalg.norm(outward, axis=1, keepdims=True)
    outward = unit(np.where(size > 0, outward, rng.normal(size=tgt.shape)))
    out_dir = unit(outward + rng.normal(size=tgt.shape) * 0.5)
    graze = rng.random(len(tgt)) < 1.0 / 3.0
    out_dir[graze] = perp(outward[graze], rng)
    org = tgt + out_dir * g.radius * (1.0 + rng.random((len(tgt), 1)))
    # two triangles that share the target accept the exact ray at the same t only where their
    # two roundings agree: of three distances of the origin, take the first at which they do
    if len(g.tris):
        for _ in range(2):
            tied = oracle_lib.tri_ties(scene_path(name), org, unit(tgt - org)) >= 2
            retry = tgt + out_dir * g.radius * (1.0 + rng.random((len(tgt), 1)))
            org = np.where(tied[:, None], org, retry)
    d0 = unit(tgt - org)
    across = unit(np.cross(along, d0))
    orgs, dirs, exact = [], [], []
    for off in EDGE_OFFSETS:
        orgs.append(org)
        dirs.append(unit(tgt + across * off - org))
        exact.append(np.full(len(tgt), off == 0.0))
    out = _rays(np.concatenate(orgs), np.concatenate(dirs))
    out["exact"] = np.concatenate(exact)
    out["aim_t"] = np.tile(np.linalg.norm(tgt - org, axis=1), len(EDGE_OFFSETS))
    out["aim_tol"] = np.full(len(out["aim_t"]), 1e-3)
    return out


@functools.lru_cache(maxsize=None)
def leaving(name, seed=4):
    """out["seed_org"], out["seed_dir"]: the ray whose hit point is the origin (the GPU test casts
    it first for the hint triangle)."""
    # seeds seen from far outside as well as from inside: a room's walls are hit on their outer
    # faces too, and a ray that leaves one of those can miss everything
    so, sd, sp, sn = seeds(name, 2500, seed, 3.0)
    rng = np.random.default_rng(seed)
    n = len(sp)
    kind = rng.integers(0, 3, n)
    rnd = unit(rng.normal(size=(n, 3)))
    # (a random direction on the side of the surface the seed ray came from, as a bounce has it)
    back = np.sign((rnd * sn).sum(-1, keepdims=True)) == np.sign((sd * sn).sum(-1, keepdims=True))
    rnd = np.where(back, -rnd, rnd)
    mir = unit(sd - 2.0 * (sd * sn).sum(-1, keepdims=True) * sn)
    tan = perp(sn, rng)
    d = np.where((kind == 0)[:, None], rnd, np.where((kind == 1)[:, None], mir, tan))
    out = _rays(sp.copy(), d)
    out["seed_org"], out["seed_dir"] = so, sd
    return out


@functools.lru_cache(maxsize=None)
def tangent(name, n=100, seed=5):
    g = geometry(name)
    rng = np.random.default_rng(seed)
    orgs, dirs, aim, tol = [], [], [], []
    round_shapes = [(c, None, r) for c, r in g.spheres] + [(p1, p2, r) for p1, p2, r in g.cyls]
    if len(round_shapes) > 6:  # the file's first three (nested.scn: the ones under its nodes)
        rest = rng.choice(np.arange(3, len(round_shapes)), 3, replace=False)
        round_shapes = round_shapes[:3] + [round_shapes[i] for i in rest]
    for c, p2, r in round_shapes:
        d = unit(rng.normal(size=(n, 3)))
        if p2 is None:
            u = perp(d, rng)
            base = np.broadcast_to(c, (n, 3))
        else:
            u = unit(np.cross(unit(p2 - c), d))
            base = c + rng.random((n, 1)) * (p2 - c)
        L = (r + g.radius) * (0.5 + rng.random((n, 1)))
        for e, add in RADIAL:
            q = base + u * (r * (1.0 + e) + add)
            orgs.append(q - d * L)
            dirs.append(d)
            aim.append(L[:, 0])
            tol.append(np.full(n, 0.01 * r))  # the chord at r (1 - 1e-5) is 0.0045 r deep
    flat = [(t.mean(0) * 0.5 + t[0] * 0.5, unit(np.cross(t[1] - t[0], t[2] - t[0]))) for t in
            (g.tris[rng.integers(0, len(g.tris), 12)] if len(g.tris) else [])]
    flat += [(c, nn) for c, nn, _r in g.circles]
    for c, nn in flat:
        m = max(16, n // 6)
        tdir = perp(np.broadcast_to(nn, (m, 3)), rng)
        for dn in DENOMS:
            d = unit(tdir + nn * dn)
            L = g.radius * (0.2 + rng.random((m, 1)))
            orgs.append(c - d * L)
            dirs.append(d)
            aim.append(L[:, 0])
            tol.append(np.full(m, 1e-3))
    if sum(len(o) for o in orgs) < 2200 and n < 3200:  # few shapes: more rays for each
        return tangent.__wrapped__(name, n * 2, seed)
    out = _rays(np.concatenate(orgs), np.concatenate(dirs))
    # the distance to the point the ray is aimed at, and how near it a hit of the target lies
    out["aim_t"], out["aim_tol"] = np.concatenate(aim), np.concatenate(tol)
    return out


WALK_CLASSES = {"axis": (axis, AXIS_SCENES), "edges": (edges, EDGE_SCENES),
                "leaving": (leaving, LEAVING_SCENES), "tangent": (tangent, TANGENT_SCENES)}
WALK_CASES = [(c, s) for c, (_f, scenes) in WALK_CLASSES.items() for s in scenes]


# cylinder.scn holds cylinders and `line` cylinders only, and a ray that starts on a cylinder
# meets it again at t = 0 whatever its direction (R3Isect.cpp:1025-1200 clamps the near root to
# 0 and accepts it): the leaving class cannot miss there, and is only asked for its hits
# stilllife.scn is a box and meshes: a ray that starts on a box face starts "inside" it by
# R3Contains' tolerance and meets the face at t = 0 or the far face (R3Isect.cpp:883-942), and one
# that starts on a mesh triangle meets the mesh's box the same way and then a triangle; 4 % miss.
FEW_MISSES = {("leaving", "cylinder.scn"), ("leaving", "stilllife.scn")}


def on_target(rays, hit, t):
    """Which rays hit what they were aimed at: a hit within aim_tol of aim_t where the class gives
    them (edges, tangent: something else usually lies behind the target), else any hit."""
    hit = np.asarray(hit) != 0
    if "aim_t" not in rays:
        return hit
    return hit & (np.abs(t - rays["aim_t"]) <= rays["aim_tol"])


def walk_rays(cls, name):
    return WALK_CLASSES[cls][0](name)


@functools.lru_cache(maxsize=None)
def oracle_walk(cls, name):
    """oracle_lib.intersect of the class's rays: (hit, t, point, normal, material). Shared by the
    tests: do not modify."""
    r = walk_rays(cls, name)
    out = oracle_lib.intersect(scene_path(name), r["org"], r["dir"])
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------
# classes for the shadow test
# ---------------------------------------------------------------------------------------------
OFFSETS = (0.0, 0.5, -0.5, 0.99, -0.99, 0.999999, -0.999999, 1.000001, -1.000001, 1.01, -1.01,
           1.04, -1.04, 1.06, -1.06, 2.0, -2.0, 10.0, -10.0)
# scene -> the light every class uses: an index into the file's lights (area / rect: the device
# forms the sample point) or None (light -1: the caller's point, here the first point light's
# position, for transform.scn the camera's)
ILLUM_SCENES = {"jensen.scn": 0, "softshadow.scn": 0, "cornell.scn": None, "stilllife.scn": None,
                "transform.scn": None, "nested_rigid.scn": 0, "nested_rigid.scn#area": 1, "nested_many.scn": 0}


def illum_scene(key):
    return key.split("#")[0]


def _light(key):
    g = geometry(illum_scene(key))
    li = ILLUM_SCENES[key]
    return g, li, (g.lights[li] if li is not None else None)


def _coeffs(L, n, rng, special=True):
    """Sample coefficients of light L: uniform in its range, and (special) a share of them on the
    range's corners and edges."""
    if L["kind"] == "area":
        ang = rng.random(n) * 2 * np.pi
        rad = np.sqrt(rng.random(n))
        if special:
            rad[rng.random(n) < 0.4] = 1.0
        r = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
        if special:  # the corners of the mask's hull (outside the disk the render samples)
            k = rng.random(n) < 0.15
            r[k] = np.where(rng.random((k.sum(), 2)) < 0.5, 1.0, -1.0)
        return r
    r = rng.random((n, 2)) - 0.5
    if special:
        k = rng.random((n, 2)) < 0.35
        r[k] = np.where(rng.random(k.sum()) < 0.5, 0.5, -0.5)
    return r


def sample_point(L, r12):
    """light_sample_point's expression in numpy (the GPU test takes the device's own bits)."""
    return ((r12[:, :1] * L["su"] + r12[:, 1:] * L["sv"]) + L["pos"]) + L["n"] * EPS


def _pack(key, p_scene, r12, p_light):
    _g, li, _L = _light(key)
    n = len(p_scene)
    return {"p_scene": np.ascontiguousarray(p_scene),
            "light": np.full(n, -1 if li is None else li, dtype=np.int32),
            "r12": np.ascontiguousarray(r12), "p_light": np.ascontiguousarray(p_light)}


def _light_points(key, n, rng, special):
    g, li, L = _light(key)
    if L is not None:
        r12 = _coeffs(L, n, rng, special)
        return r12, sample_point(L, r12)
    # light -1: the first positional light's place (the camera's side of transform.scn, which has
    # none), and for every other ray a point outside the scene, from where other surfaces hide
    # many of the seeds: both verdicts occur in every scene
    pos = next((L["pos"] for L in g.lights if "pos" in L), np.array([0.0, 0.0, 20.0]))
    pl = np.broadcast_to(pos, (n, 3)).copy()
    pl[1::2] = g.centre + g.radius * 1.2 * unit(np.array([0.6, 0.5, 0.62]))
    return np.zeros((n, 2)), pl


@functools.lru_cache(maxsize=None)
def light_seeds(key, n=300, seed=6):
    """Surface points the light's rays reach first, and some they do not: the oracle's hits of
    rays from light points towards random scene seeds (first hits) and the seeds themselves."""
    name = illum_scene(key)
    rng = np.random.default_rng(seed)
    sp = seeds(name)[2]
    tgt = sp[rng.integers(0, len(sp), n)]
    _r, pl = _light_points(key, n, rng, False)
    h, _t, p, _n, _m = oracle_lib.intersect(scene_path(name), pl, unit(tgt - pl))
    first = p[h != 0]
    out = np.concatenate([first[:(2 * n) // 3], tgt[:n - min(len(first), (2 * n) // 3)]])
    out.setflags(write=False)
    return out


def _steep(key, sp, pl, min_cos=0.1):
    """Which of the points sp the light rays from pl meet at |cos| >= min_cos to the surface
    normal there (the oracle's, of a ray along the light ray from just in front of the point)."""
    d = unit(sp - pl)
    h, _t, _p, nr, _m = oracle_lib.intersect(scene_path(illum_scene(key)), sp - d * 1e-3, d)
    return (h != 0) & (np.abs((nr * d).sum(-1)) >= min_cos)


@functools.lru_cache(maxsize=None)
def offsets(key, seed=7):
    """Every seed with every s of OFFSETS, the same light point for all of a seed's offsets.
    out["s"]: the offset of each ray."""
    rng = np.random.default_rng(seed)
    sp = light_seeds(key)
    r12, pl = _light_points(key, len(sp), rng, False)
    # a surface nearly parallel to the light ray (jensen's light triangles seen from the light in
    # their plane) multiplies the rounding of the hit's t past the 1e-12 between s = 0.999999 and
    # 1: such points are the thin class's, not this one's
    keep = _steep(key, sp, pl)
    sp, r12, pl = sp[keep], r12[keep], pl[keep]
    n = len(sp)
    along = unit(sp - pl)
    ps = np.concatenate([sp + along * (s * EPS) for s in OFFSETS])
    out = _pack(key, ps, np.tile(r12, (len(OFFSETS), 1)), np.tile(pl, (len(OFFSETS), 1)))
    out["s"] = np.repeat(np.array(OFFSETS), n)
    return out


@functools.lru_cache(maxsize=None)
def coeffs(key, n=3000, seed=8):
    rng = np.random.default_rng(seed)
    sp = light_seeds(key)
    ps = sp[rng.integers(0, len(sp), n)]
    r12, pl = _light_points(key, n, rng, True)
    return _pack(key, ps, r12, pl)


# scene key -> (foot points: [(centre of contact, normal of the floor, reach)]): points on the
# floor plane within `reach` of where an occluder touches it or ends
THIN = {
    "softshadow.scn": [((-1.0, 0.0, 0.0), (0, 1, 0), 0.02), ((1.0, 0.0, 0.0), (0, 1, 0), 0.02)],
    # the ceiling over and next to the light triangles, the triangles' own plane (that of the
    # light, one RN_EPSILON above its sample points) and the floor under the glass sphere
    "jensen.scn": [((2.75, 5.0, 1.8), (0, 1, 0), 1.3), ((2.75, 4.99, 1.8), (0, 1, 0), 1.3),
                   ((1.45, 0.001, 1.8), (0, 1, 0), 0.05)],
    # the rim of the table top: a corner and an edge
    "stilllife.scn": [((3.0, 0.0, 3.0), (0, 1, 0), 0.02), ((3.0, 0.0, 0.0), (0, 1, 0), 0.02)],
    "nested_rigid.scn": [((-6.25 * 0.8660254037844387 + 1 * 0.5, -1.0, 6.25 * 0.5 + 1 * 0.8660254037844387),
                          (0, 1, 0), 0.02)],
}
THIN["nested_rigid.scn#area"] = THIN["nested_rigid.scn"]


@functools.lru_cache(maxsize=None)
def thin(key, n=2000, seed=9):
    rng = np.random.default_rng(seed)
    spots = THIN[key]
    ps = []
    for c, nn, reach in spots:
        c, nn = np.array(c, float), np.array(nn, float)
        m = -(-n // len(spots))
        # distances from the contact log-uniform in [1e-7, reach]
        rad = np.exp(rng.uniform(np.log(1e-7), np.log(reach), m))[:, None]
        ps.append(c + perp(np.broadcast_to(nn, (m, 3)), rng) * rad)
    ps = np.concatenate(ps)
    r12, pl = _light_points(key, len(ps), rng, True)
    return _pack(key, ps, r12, pl)


ILLUM_CLASSES = {"offsets": offsets, "coeffs": coeffs, "thin": thin}
ILLUM_CASES = [(c, k) for c in ("offsets", "coeffs") for k in ILLUM_SCENES] + [("thin", k) for k in THIN]


def illum_rays(cls, key):
    return ILLUM_CLASSES[cls](key)
