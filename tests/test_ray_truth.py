"""Closest-hit ray queries against a float64 truth (tests/ray_truth.py) on rays chosen to be hostile to a BVH walk: axis-parallel and denormal
directions, boxes of zero thickness, origins far along an axis the ray barely moves on, geometry at 1e-3 .. 1e3, shared edges and vertices,
transformed instances, self-hits and coplanar duplicates.

dev_trace.h claims that "a triangle accepted by the exact test is never culled by rounding": the slab test (safe_inv, noi = -(o * inv), the relaxed
comparison), the builders' box padding, the thinner padding of the instances' world boxes and the cull on pop all have to hold for it. The truth
walks no tree, so an error in any of them shows as an answer it rejects.

CPU tests: the truth on hand-made cases; the oracle's float32 brute force (no tree either) passes the acceptor on every family, which shows the
bounds are sound, and the decisive shares show they are not vacuous; mutated answers are rejected.
GPU tests: per family and builder, the exact flavour is bit-identical to the oracle's brute force, both flavours pass the acceptor, and on decisive
rays the fast flavour returns the exact flavour's triangle.
"""
import functools

import numpy as np
import pytest

import oracle_lib
import ray_truth
from luminary_amd import Host, scenes

NONE = 0xFFFFFFFF
INTERIOR, GRAZING, OTHER = 0, 1, 2
TAG_NAMES = {INTERIOR: "interior-aimed", GRAZING: "grazing", OTHER: "other"}
SHARE = {INTERIOR: 0.95, GRAZING: 0.5}  # decisive shares the families must reach (conditions on the families' inputs, not tuned to results)


# ---- scenes ----
def _scene(meshes, instances):
    """meshes: list of [n, 3, 3] arrays; instances: list of (mesh, position, rotation, scale). Returns (host, view)."""
    host = Host()
    scenes.apply_benchmark_settings(host, 16, 16, 2, sky=(0.5, 0.5, 0.5))
    mat = host.add_material(scenes._material((0.6, 0.6, 0.6), 0.6))
    ids = [host.add_mesh(np.asarray(t, dtype=np.float32).reshape(len(t), 9), np.full(len(t), mat, dtype=np.uint16)) for t in meshes]
    for (m, pos, rot, scale) in instances:
        host.new_instance(ids[m], pos, rot, scale)
    scenes.set_camera(host, (0.0, 0.0, 30.0), (0.0, 0.0, 0.0))
    return host, oracle_lib.with_luts(host.device_scene())


def _box(lo, hi, n=1):
    """A closed box of 12 n^2 triangles."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    tris = []
    for axis in range(3):
        b, c = (axis + 1) % 3, (axis + 2) % 3
        for side in (lo, hi):
            for i in range(n):
                for j in range(n):
                    def p(u, v):
                        q = np.zeros(3)
                        q[axis] = side[axis]
                        q[b] = lo[b] + (hi[b] - lo[b]) * u / n
                        q[c] = lo[c] + (hi[c] - lo[c]) * v / n
                        return q
                    tris.append([p(i, j), p(i + 1, j), p(i + 1, j + 1)])
                    tris.append([p(i, j), p(i + 1, j + 1), p(i, j + 1)])
    return np.array(tris, dtype=np.float32)


def _icosphere(level, radius=1.0):
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6),
         (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    tris = np.array([[v[a], v[b], v[c]] for (a, b, c) in f], dtype=np.float64)
    for _ in range(level):
        a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
        ab, bc, ca = (a + b) / 2, (b + c) / 2, (c + a) / 2
        tris = np.concatenate([np.stack(x, axis=1) for x in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))])
    tris /= np.linalg.norm(tris, axis=2, keepdims=True)
    # float32 first, so that a vertex shared by several triangles is the same float32 point in all of them
    return (tris * radius).astype(np.float32)


def _grid(n, size):
    xs = np.linspace(-size, size, n + 1)
    tris = []
    for i in range(n):
        for j in range(n):
            def p(a, b):
                return [xs[a], 0.25 * np.sin(1.3 * xs[a]) * np.cos(0.9 * xs[b]), xs[b]]
            tris.append([p(i, j), p(i + 1, j), p(i + 1, j + 1)])
            tris.append([p(i, j), p(i + 1, j + 1), p(i, j + 1)])
    return np.array(tris, dtype=np.float32)


def _soup(rng, n, spread=10.0):
    """The soup of test_gpu_builders_on_triangle_soups."""
    c = rng.uniform(-1.0, 1.0, (n, 1, 3)) * spread
    return c + rng.normal(size=(n, 3, 3)) * rng.choice([0.05, 0.5, 4.0], size=(n, 1, 1))


def _normalise32(d):
    d = np.asarray(d, dtype=np.float64)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return (d / np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)).astype(np.float32)  # normalised in float32


def _targets(rng, tris, idx, lo=0.1, hi=0.8):
    """Interior points of triangles `idx` (float32 positions as stored): barycentrics u, v >= lo, u + v <= hi."""
    t = np.asarray(tris, dtype=np.float32).astype(np.float64)[idx]
    u = rng.uniform(lo, hi - lo, len(idx))
    v = rng.uniform(lo, hi - u)
    return t[:, 0] + u[:, None] * (t[:, 1] - t[:, 0]) + v[:, None] * (t[:, 2] - t[:, 0])


def _no_ignore(n):
    return np.full((n, 2), NONE, dtype=np.uint32)


class Family:
    def __init__(self, meshes, instances, o, d, tags, ignore=None, never_sky=False):
        self.meshes, self.instances = meshes, instances
        self.o = np.ascontiguousarray(o, dtype=np.float32)
        self.d = np.ascontiguousarray(d, dtype=np.float32)
        self.tags = np.asarray(tags)
        self.ignore = _no_ignore(len(self.o)) if ignore is None else np.ascontiguousarray(ignore, dtype=np.uint32)
        self.never_sky = never_sky
        assert self.o.shape == self.d.shape and len(self.tags) == len(self.o) <= 20000
        assert sum(len(m) for m in meshes) <= 4000
        assert np.all(np.isfinite(self.o)) and np.all(np.isfinite(self.d)) and np.all(np.linalg.norm(self.d.astype(np.float64), axis=1) > 0.5)


IDENTITY = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
DEAD = [0.0, -0.0, 1e-31, -1e-31, 9e-31, -9e-31, 1.1e-30, -1.1e-30, 1e-29, -1e-29]  # safe_inv's threshold is 1e-30


def _axis_parallel_rays(rng, tris_world, n, lo=0.1, hi=0.8):
    """Rays with one or two dead direction components aimed at triangles given in world space ([m, 3, 3] float32 positions). A third of them at an
    interior point, a third with the dead coordinate exactly on the face of the target's box, a third just outside it (inside the box padding)."""
    tw = np.asarray(tris_world, dtype=np.float32)
    idx = rng.randint(0, len(tw), n)
    tgt = _targets(rng, tw, idx, lo, hi)
    mode = rng.randint(0, 3, n)  # 0 inside, 1 on, 2 outside the target's box along the dead axes
    two = rng.randint(0, 2, n).astype(bool)
    axis = rng.randint(0, 3, n)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[np.abs(d) < 0.2] = 0.3
    dead = np.zeros((n, 3), dtype=bool)
    dead[np.arange(n), axis] = True
    dead[np.arange(n), (axis + 1) % 3] |= two
    box_lo, box_hi = tw[idx].min(axis=1).astype(np.float64), tw[idx].max(axis=1).astype(np.float64)
    side = rng.randint(0, 2, (n, 3)).astype(bool)
    face = np.where(side, box_hi, box_lo)
    out = face + np.where(side, 1.0, -1.0) * (4e-6 * np.abs(face) + 1e-30)
    tgt = np.where(dead & (mode == 1)[:, None], face, tgt)
    tgt = np.where(dead & (mode == 2)[:, None], out, tgt)
    d = _normalise32(np.where(dead, 0.0, d))
    d[dead] = np.asarray(DEAD, dtype=np.float32)[rng.randint(0, len(DEAD), int(dead.sum()))]
    t = rng.uniform(1.0, 20.0, (n, 1))
    o = (tgt - t * d.astype(np.float64)).astype(np.float32)
    o[dead] = tgt.astype(np.float32)[dead]  # the ray's constant coordinates, exactly
    return o, d, np.where(mode == 0, INTERIOR, OTHER)


def family_axis_parallel():
    rng = np.random.RandomState(101)
    soup = (_soup(rng, 300, 5.0)).astype(np.float32)
    back = _box((-60.0,) * 3, (60.0,) * 3)
    o, d, tags = _axis_parallel_rays(rng, soup, 3000)
    return Family([soup, back], [(0,) + IDENTITY, (1,) + IDENTITY], o, d, tags)


def family_flat_boxes():
    rng = np.random.RandomState(102)
    tris, plane = [], []
    for axis in range(3):
        for c in (0.0, 1e-3, 1.0, 100.00001, 1e4):
            for cell in range(6):  # one triangle per 5 x 5 cell: triangles of one plane do not overlap
                p = np.zeros((3, 3))
                centre = np.array([5.0 * (cell % 3) - 5.0, 5.0 * (cell // 3) - 2.5])
                corners = rng.uniform(-2.2, 2.2, (3, 2))
                e1, e2 = corners[1] - corners[0], corners[2] - corners[0]
                if abs(e1[0] * e2[1] - e1[1] * e2[0]) < 2.0:  # no slivers: the family is about the boxes, not the triangle test
                    corners = np.array([[-2.0, -2.0], [2.0, -1.5], [-1.0, 2.0]]) + rng.uniform(-0.2, 0.2, (3, 2))
                p[:, (axis + 1) % 3] = centre[0] + corners[:, 0]
                p[:, (axis + 2) % 3] = centre[1] + corners[:, 1]
                p[:, axis] = np.float32(c)
                tris.append(p)
                plane.append((axis, np.float64(np.float32(c))))
    tris = np.array(tris, dtype=np.float32)
    back = _box((-3e4,) * 3, (3e4,) * 3)
    n = 3000
    idx = rng.randint(0, len(tris), n)
    tgt = _targets(rng, tris, idx)
    angles = np.array([np.pi / 2, 0.5, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5])
    ang = angles[rng.randint(0, len(angles), n)]
    axis = np.array([plane[i][0] for i in idx])
    c = np.array([plane[i][1] for i in idx])
    inplane = rng.normal(size=(n, 3))
    inplane[np.arange(n), axis] = 0.0
    inplane /= np.linalg.norm(inplane, axis=1, keepdims=True)
    normal = np.zeros((n, 3))
    normal[np.arange(n), axis] = rng.choice([-1.0, 1.0], n)
    d64 = np.cos(ang)[:, None] * inplane + np.sin(ang)[:, None] * normal
    d = _normalise32(d64)
    # far enough back that the origin leaves the plane by several float32 steps of its coordinate there
    t = np.maximum(rng.uniform(0.5, 3.0, n), 64.0 * np.spacing(np.float32(np.maximum(np.abs(c), 1e-3))).astype(np.float64) / np.sin(ang))
    o = (tgt - t[:, None] * d.astype(np.float64)).astype(np.float32)
    tags = np.where(ang >= 0.5, INTERIOR, GRAZING)
    # rays inside the plane's slab, parallel to it, past the triangles: they miss them all and must reach the backdrop
    m = 1000
    idx2 = rng.randint(0, len(tris), m)
    tgt2 = _targets(rng, tris, idx2)
    axis2 = np.array([plane[i][0] for i in idx2])
    c2 = np.array([plane[i][1] for i in idx2])
    d2 = rng.normal(size=(m, 3))
    d2[np.arange(m), axis2] = 0.0
    d2 = _normalise32(d2)
    d2[np.arange(m), axis2] = rng.choice(np.float32([0.0, -0.0]), m)
    o2 = (tgt2 - rng.uniform(0.5, 3.0, (m, 1)) * d2.astype(np.float64)).astype(np.float32)
    c32 = c2.astype(np.float32)
    off = rng.randint(0, 5, m)  # in the plane, one float32 step off it, or halfway into the box padding
    pad = (4e-6 * np.abs(c2)).astype(np.float32)
    o2[np.arange(m), axis2] = np.select([off == 0, off == 1, off == 2, off == 3], [c32, np.nextafter(c32, np.float32(np.inf)), np.nextafter(c32, np.float32(-np.inf)), c32 + pad],
                                        c32 - pad)
    return Family([tris, back], [(0,) + IDENTITY, (1,) + IDENTITY], np.concatenate([o, o2]), np.concatenate([d, d2]),
                  np.concatenate([tags, np.full(m, INTERIOR)]))


def family_far_shallow():
    rng = np.random.RandomState(103)
    # clusters of triangles whose coordinate on one axis is about B; a small sphere for the far rays
    tris, where = [], []
    for axis in range(3):
        for B in (1.0, 100.0, 1e4):
            for _ in range(12):
                c = rng.uniform(-3.0, 3.0, 3)
                c[axis] = B
                tris.append(c + rng.normal(size=(3, 3)) * 0.7)
                where.append((axis, B))
    near = np.array(tris, dtype=np.float32)
    centre = np.float32([-40.0, -40.0, -40.0])
    ball = _icosphere(1) + centre  # diameter 2, away from the clusters; seen from outside its front is one layer of 0.6-wide triangles
    n = 3000
    idx = rng.randint(0, len(near), n)
    tgt = _targets(rng, near, idx, 0.2, 0.7)
    axis = np.array([where[i][0] for i in idx])
    K = 10.0 ** rng.choice([2, 4, 6, 8], n)
    t = rng.uniform(1.0, 10.0, n)
    d64 = rng.normal(size=(n, 3))
    d64[np.arange(n), axis] = 0.0
    d64 /= np.linalg.norm(d64, axis=1, keepdims=True)
    d64[np.arange(n), axis] = rng.choice([-1.0, 1.0], n) * np.abs(tgt[np.arange(n), axis]) / (K * t)  # |o_a / d_a| = K * t
    d = _normalise32(d64)
    o = (tgt - t[:, None] * d.astype(np.float64)).astype(np.float32)
    m = 1500
    idx2 = rng.randint(0, len(ball), m)
    tgt2 = _targets(rng, ball, idx2, 0.3, 0.7)
    dist = 2.0 * 10.0 ** rng.choice([3, 4, 5], m)  # 1e3 .. 1e5 diameters
    out = tgt2 - centre.astype(np.float64)  # from the side the target faces, up to about 40 degrees off its normal
    out = out / np.linalg.norm(out, axis=1, keepdims=True) + rng.uniform(-0.45, 0.45, (m, 3))
    o2 = (tgt2 + dist[:, None] * out / np.linalg.norm(out, axis=1, keepdims=True)).astype(np.float32)
    d2 = _normalise32(tgt2 - o2.astype(np.float64))
    return Family([near, ball], [(0,) + IDENTITY, (1,) + IDENTITY], np.concatenate([o, o2]), np.concatenate([d, d2]), np.full(n + m, INTERIOR))


def family_scale(scale):
    rng = np.random.RandomState(11)
    soup = _soup(rng, 300)
    # long thin triangles, aspect 1e4
    thin = []
    for _ in range(40):
        c = rng.uniform(-10.0, 10.0, 3)
        along = rng.normal(size=3)
        along /= np.linalg.norm(along)
        across = np.cross(along, rng.normal(size=3))
        across /= np.linalg.norm(across)
        thin.append([c, c + 10.0 * along, c + 5.0 * along + 1e-3 * across])
    tris = (np.concatenate([soup, np.array(thin)]) * scale).astype(np.float32)
    back = _box((-80.0 * scale,) * 3, (80.0 * scale,) * 3)
    n = 2500
    idx = rng.randint(0, len(tris), n)
    tgt = _targets(rng, tris, idx, 0.2, 0.7)
    span = float(np.abs(tris).max())
    o = rng.uniform(-1.5 * span, 1.5 * span, (n, 3)).astype(np.float32)
    d = _normalise32(tgt - o.astype(np.float64))
    return Family([tris, back], [(0,) + IDENTITY, (1,) + IDENTITY], o, d, np.full(n, INTERIOR))


def _shared_features(rng, tris, n):
    """float32 targets on the vertices and the edges of a mesh."""
    t = np.asarray(tris, dtype=np.float32)
    idx = rng.randint(0, len(t), n)
    k = rng.randint(0, 3, n)
    a, b = t[idx, k], t[idx, (k + 1) % 3]
    s = np.where(rng.randint(0, 2, n) == 0, 0.0, rng.uniform(0.05, 0.95, n)).astype(np.float32)  # 0: the vertex itself
    return (a + s[:, None] * (b - a)).astype(np.float32)


def family_edges():
    rng = np.random.RandomState(105)
    box, ico, grid = _box((-1.0,) * 3, (1.0,) * 3, 4), _icosphere(2), _grid(16, 2.0)
    places = [np.float32([-6.0, 0.0, 0.0]), np.float32([0.0, 0.0, 0.0]), np.float32([6.0, 0.0, 0.0])]
    meshes = [box + places[0], ico + places[1], grid + places[2]]  # float32 sums: the stored positions
    back = _box((-100.0,) * 3, (100.0,) * 3)
    os_, ds = [], []
    for mesh, centre, closed in zip(meshes, places, (True, True, False)):
        n = 1000
        tgt = _shared_features(rng, mesh, n).astype(np.float64)
        dirs = rng.normal(size=(n, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        inside = rng.randint(0, 2, n).astype(bool) & closed
        o = np.where(inside[:, None], centre + rng.uniform(-0.3, 0.3, (n, 3)), centre + 8.0 * dirs).astype(np.float32)
        os_.append(o)
        ds.append(_normalise32(tgt - o.astype(np.float64)))
    o, d = np.concatenate(os_), np.concatenate(ds)
    return Family(meshes + [back], [(i,) + IDENTITY for i in range(4)], o, d, np.full(len(o), OTHER), never_sky=True)


def _instance_world(words, pts):
    """Object -> world of dev_math.h xf_point (S * R * v + T) in float64, for aiming only."""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    p = w.view(np.float32).astype(np.float64)
    q = np.array([(int(w[6]) & 0xFFFF), (int(w[6]) >> 16), (int(w[7]) & 0xFFFF), (int(w[7]) >> 16)], dtype=np.float64) / 0x7FFF - 1.0
    u, s = q[0:3], q[3]
    v = np.asarray(pts, dtype=np.float64)
    r = 2.0 * (v @ u)[..., None] * u + (s * s - u @ u) * v + 2.0 * s * np.cross(u, v)
    return r * p[3:6] + p[0:3]


def family_instances():
    rng = np.random.RandomState(106)
    mesh = np.concatenate([_icosphere(1), (rng.uniform(-1.0, 1.0, (30, 1, 3)) + rng.normal(size=(30, 3, 3)) * 0.4).astype(np.float32)])
    back = _box((-90.0,) * 3, (90.0,) * 3)
    instances = []
    for i in range(12):
        scale = (0.25, 1.0, 4.0) if i == 0 else tuple(rng.uniform(0.25, 4.0, 3))
        instances.append((0, tuple(rng.uniform(-10.0, 10.0, 3)), tuple(rng.uniform(-3.1, 3.1, 3)), scale))
    instances.append((1,) + IDENTITY)
    host, view = _scene([mesh, back], instances)
    words = oracle_lib.view_arrays(view)["instance_transforms"].reshape(-1, 8)
    world = [_instance_world(words[i], mesh) for i in range(12)]
    host.close()
    n = 2500
    inst = rng.randint(0, 12, n)
    idx = rng.randint(0, len(mesh), n)
    tgt = np.zeros((n, 3))
    for i in range(12):
        sel = inst == i
        tgt[sel] = _targets(rng, world[i], idx[sel], 0.2, 0.7)
    o = rng.uniform(-15.0, 15.0, (n, 3)).astype(np.float32)
    d = _normalise32(tgt - o.astype(np.float64))
    o2, d2, tags2 = _axis_parallel_rays(rng, np.concatenate(world), 1000, 0.2, 0.7)
    return Family([mesh, back], instances, np.concatenate([o, o2]), np.concatenate([d, d2]), np.concatenate([np.full(n, INTERIOR), tags2]))


def family_self_hits():
    rng = np.random.RandomState(107)
    soup = _soup(rng, 200, 4.0).astype(np.float32)
    soup[180:200] = soup[0:20]  # coplanar duplicates inside the mesh; the second instance duplicates every triangle
    back = _box((-50.0,) * 3, (50.0,) * 3)
    n = 2000
    idx = rng.randint(0, len(soup), n)
    o = _targets(rng, soup, idx).astype(np.float32)  # on the triangle: t = 0 for it
    d = rng.normal(size=(n, 3))
    d = _normalise32(d)
    ign = _no_ignore(n)
    with_handle = rng.randint(0, 2, n).astype(bool)
    ign[with_handle, 0] = rng.randint(0, 2, int(with_handle.sum()))
    ign[with_handle, 1] = idx[with_handle]
    # rays aimed at a triangle from outside, ignoring it: the duplicate or whatever lies behind answers
    m = 1000
    idx2 = rng.randint(0, len(soup), m)
    tgt = _targets(rng, soup, idx2, 0.2, 0.7)
    o2 = rng.uniform(-8.0, 8.0, (m, 3)).astype(np.float32)
    d2 = _normalise32(tgt - o2.astype(np.float64))
    ign2 = _no_ignore(m)
    ign2[:, 0] = rng.randint(0, 2, m)
    ign2[:, 1] = idx2
    return Family([soup, back], [(0,) + IDENTITY, (0,) + IDENTITY, (1,) + IDENTITY], np.concatenate([o, o2]), np.concatenate([d, d2]), np.full(n + m, OTHER),
                  ignore=np.concatenate([ign, ign2]))


FAMILIES = {
    "axis_parallel": family_axis_parallel,
    "flat_boxes": family_flat_boxes,
    "far_shallow": family_far_shallow,
    "scale_1e-3": functools.partial(family_scale, 1e-3),
    "scale_1": functools.partial(family_scale, 1.0),
    "scale_1e3": functools.partial(family_scale, 1e3),
    "edges_vertices": family_edges,
    "instances": family_instances,
    "self_hits": family_self_hits,
}


@functools.lru_cache(maxsize=None)
def _prepared(name):
    """(family, host, view, solution, the oracle's brute-force answers): computed once, shared by the tests, never modified."""
    fam = FAMILIES[name]()
    host, view = _scene(fam.meshes, fam.instances)
    sol = ray_truth.solve(ray_truth.scene_of_view(view), fam.o, fam.d, fam.ignore)
    want = oracle_lib.trace_closest(view, fam.o, fam.d, fam.ignore, use_bvh=False)
    want.setflags(write=False)
    return fam, host, view, sol, want


def _failures(sol, answers, bad, limit=5):
    return "\n".join(sol.describe(int(i), answers[i]) for i in np.nonzero(bad)[0][:limit])


# ---- CPU: the truth on known answers ----
def _single(tris, o, d, instances=None, ignore=None):
    host, view = _scene([np.asarray(tris, dtype=np.float32)], instances or [(0,) + IDENTITY])
    o, d = np.float32([o]), np.float32([d])
    sol = ray_truth.solve(ray_truth.scene_of_view(view), o, d, ignore)
    return sol, oracle_lib.trace_closest(view, o, d, ignore, use_bvh=False), view


TRI = [[[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 3.0, 0.0]]]


def _answer(inst, tri, t):
    return np.array([[inst, tri, np.float32(t).view(np.uint32)]], dtype=np.uint32)


def test_truth_known_answers():
    # through the centroid, straight down from z = 5: the hit is certain, at t = 5
    sol, got, _ = _single(TRI, (1.0, 1.0, 5.0), (0.0, 0.0, -1.0))
    assert sol.decisive[0] and sol.has_certain_hit[0] and sol.expected()[0][0] == 0 and sol.expected()[1][0] == 0
    assert sol.check(_answer(0, 0, 5.0))[0][0] and sol.check(got)[0][0]
    assert not sol.check(_answer(ray_truth.SKY, 0, 3.4e38))[0][0]
    assert not sol.check(_answer(0, 0, 5.00001))[0][0], "bt of a well-conditioned hit is a few ulp, not 1e-5"
    assert not sol.check(_answer(0, 1, 5.0))[0][0], "a triangle that does not exist"
    # 1e-3 outside the edge y = 0: a certain miss
    sol, got, _ = _single(TRI, (1.0, -1e-3, 5.0), (0.0, 0.0, -1.0))
    assert sol.decisive[0] and not sol.has_certain_hit[0] and sol.expected()[0][0] == ray_truth.SKY
    assert sol.check(got)[0][0] and got[0, 0] == ray_truth.SKY and not sol.check(_answer(0, 0, 5.0))[0][0]
    # 1e-3 inside the same edge: a certain hit
    sol, got, _ = _single(TRI, (1.0, 1e-3, 5.0), (0.0, 0.0, -1.0))
    assert sol.decisive[0] and sol.has_certain_hit[0] and sol.check(got)[0][0]
    # exactly on the edge, every product exact: float32 computes v = 0 without any error, and v = 0 is a hit
    sol, got, _ = _single(TRI, (1.0, 0.0, 5.0), (0.0, 0.0, -1.0))
    assert sol.decisive[0] and sol.has_certain_hit[0] and sol.check(got)[0][0] and got[0, 0] == 0
    # aimed at a point of the edge along a direction that has to be rounded: either answer
    aim = np.float64([1.1, 0.0, 0.0]) - np.float64(np.float32([0.3, -0.7, 5.1]))
    sol, got, _ = _single(TRI, (0.3, -0.7, 5.1), tuple(_normalise32([aim])[0]))
    t_edge = float(np.linalg.norm(aim))
    assert not sol.decisive[0] and sol.check(_answer(0, 0, t_edge))[0][0] and sol.check(_answer(ray_truth.SKY, 0, 3.4e38))[0][0] and sol.check(got)[0][0]
    # behind the origin
    sol, got, _ = _single(TRI, (1.0, 1.0, 5.0), (0.0, 0.0, 1.0))
    assert sol.decisive[0] and not sol.has_certain_hit[0] and got[0, 0] == ray_truth.SKY and not sol.check(_answer(0, 0, 5.0))[0][0]
    # the ignored triangle
    ign = np.array([[0, 0]], dtype=np.uint32)
    sol, got, _ = _single(TRI, (1.0, 1.0, 5.0), (0.0, 0.0, -1.0), ignore=ign)
    assert sol.decisive[0] and not sol.has_certain_hit[0] and got[0, 0] == ray_truth.SKY and not sol.check(_answer(0, 0, 5.0))[0][0]


def test_truth_known_answer_on_a_rotated_and_scaled_instance():
    # rotation by pi / 2 about z, scale (2, 1, 0.5), translation (10, 20, 30); the centroid (1, 1, 0) is mapped with the decoded transform
    inst = [(0, (10.0, 20.0, 30.0), (0.0, 0.0, np.pi / 2), (2.0, 1.0, 0.5))]
    host, view = _scene([np.float32(TRI)], inst)
    words = oracle_lib.view_arrays(view)["instance_transforms"].reshape(-1, 8)
    c = _instance_world(words[0], np.float64([[1.0, 1.0, 0.0]]))[0]
    corners = _instance_world(words[0], np.float64(TRI[0]))
    # S * R * v + T: the edge along x turns into y (scale 1), the edge along y into x (scale 2); quat16 keeps 15 bits of the rotation
    assert np.allclose(np.abs(corners[1] - corners[0]), [0.0, 3.0, 0.0], atol=2e-3) and np.allclose(np.abs(corners[2] - corners[0]), [6.0, 0.0, 0.0], atol=2e-3), corners
    o = np.float32([[c[0], c[1], c[2] + 4.0], [c[0] + 50.0, c[1], c[2] + 4.0]])
    d = np.float32([[0.0, 0.0, -1.0], [0.0, 0.0, -1.0]])
    sol = ray_truth.solve(ray_truth.scene_of_view(view), o, d)
    got = oracle_lib.trace_closest(view, o, d, None, use_bvh=False)
    assert sol.decisive.all() and sol.has_certain_hit[0] and not sol.has_certain_hit[1]
    ok, why = sol.check(got)
    assert ok.all(), why
    assert got[0, 0] == 0 and abs(float(got[0:1, 2].view(np.float32)[0]) - 4.0) < 1e-3  # distances are world distances
    assert sol.check(np.concatenate([_answer(0, 0, 4.0), _answer(ray_truth.SKY, 0, 3.4e38)]))[0].all()
    assert not sol.check(np.concatenate([_answer(0, 0, 4.01), _answer(0, 0, 4.0)]))[0].any()
    host.close()


# ---- CPU: the oracle's brute force alone, per family ----
@pytest.mark.parametrize("name", list(FAMILIES))
def test_the_reference_alone_passes_and_the_truth_decides(name):
    fam, _, _, sol, want = _prepared(name)
    ok, _ = sol.check(want)
    print("%s: %d rays, %d pairs per ray, oracle brute force rejected %d" % (name, len(fam.o), sol.scene.num_pairs, int((~ok).sum())))
    for tag, label in TAG_NAMES.items():
        sel = fam.tags == tag
        if sel.any():
            print("  %-14s %5d rays, decisive share %.4f (certain hits on %.4f)" % (label, int(sel.sum()), sol.decisive[sel].mean(), sol.has_certain_hit[sel].mean()))
    assert ok.all(), "float32 brute force rejected by the truth (%d rays):\n%s" % (int((~ok).sum()), _failures(sol, want, ~ok))
    for tag, share in SHARE.items():
        sel = fam.tags == tag
        if sel.any():
            assert sol.decisive[sel].mean() >= share, "%s, %s rays: decisive share %.4f below %.2f" % (name, TAG_NAMES[tag], sol.decisive[sel].mean(), share)
            # an interior-aimed ray hits what it is aimed at or something in front of it
            assert sol.has_certain_hit[sel & sol.decisive].mean() > 0.9
    if fam.never_sky:
        assert not (want[:, 0] == ray_truth.SKY).any()
    # on decisive rays the truth names the answer itself
    inst, tri = sol.expected()
    dec = sol.decisive
    assert np.array_equal(inst[dec], want[dec, 0]) and np.array_equal(tri[dec & sol.has_certain_hit], want[dec & sol.has_certain_hit, 1])


@pytest.mark.parametrize("name", list(FAMILIES))
def test_the_acceptor_can_fail(name):
    fam, _, _, sol, want = _prepared(name)
    hit = sol.decisive & sol.has_certain_hit
    assert hit.sum() > 0
    # "sky" where a triangle is certainly hit
    mutated = want.copy()
    mutated[hit, 0], mutated[hit, 1], mutated[hit, 2] = ray_truth.SKY, 0, np.float32(3.402823466e38).view(np.uint32)
    ok, _ = sol.check(mutated)
    assert not ok[hit].any() and np.array_equal(ok[~hit], sol.check(want)[0][~hit])
    # the second-nearest certain hit (with its own, correct distance) where there is one
    far = hit & (sol.farther_hit >= 0)
    print("%s: %d decisive hits mutated to sky, %d to the second-nearest certain hit" % (name, int(hit.sum()), int(far.sum())))
    assert far.sum() > 0
    inst, tri = sol.scene.handle_of(np.where(far, sol.farther_hit, 0))
    _, t, _ = sol.pair_values(np.where(far, sol.farther_hit, -1))
    mutated = want.copy()
    mutated[far, 0], mutated[far, 1], mutated[far, 2] = inst[far], tri[far], t[far].astype(np.float32).view(np.uint32)
    ok, _ = sol.check(mutated)
    assert not ok[far].any()
    # a distance 1e-3 off, on the right triangle: far outside the bound of a hit the ray was aimed at
    aimed = hit & (fam.tags == INTERIOR)
    if aimed.any():
        off = want.copy()
        off[aimed, 2] = (off[aimed, 2].copy().view(np.float32) * np.float32(1.001)).view(np.uint32)
        ok, _ = sol.check(off)
        print("%s: a distance 1e-3 off passes on %.4f of %d aimed decisive hits" % (name, ok[aimed].mean(), int(aimed.sum())))
        assert ok[aimed].mean() < 0.05  # (the few that pass: needle triangles and hits a few 1e-4 from the origin, whose bt is honestly that wide)


# ---- GPU ----
@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["sah", "sah_gpu", "lbvh", "ploc"])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_gpu_closest_hits_against_the_truth(name, builder):
    from luminary_amd.core import Core
    fam, _, view, sol, want = _prepared(name)
    core = Core(0)
    try:
        core.set_bvh_builder(builder)
        core.upload(view)
        used = core.bvh_meshes_by_builder()
        assert builder == "sah" or used["lbvh"] >= 1, "%s: no mesh was built on the device: %s" % (builder, used)
        core.set_flavour("exact")
        exact = core.trace_closest_host(fam.o, fam.d, fam.ignore)
        core.set_flavour("fast")
        fast = core.trace_closest_host(fam.o, fam.d, fam.ignore)
    finally:
        core.close()
    where = "%s, %s" % (name, builder)
    ok_e, why_e = sol.check(exact)
    ok_f, why_f = sol.check(fast)
    same = (exact == want).all(axis=1)
    dec = sol.decisive
    agree = (fast[:, 0] == exact[:, 0]) & (fast[:, 1] == exact[:, 1])
    print("%s: %d rays | exact: %d differ from the brute force, %d rejected | fast: %d rejected, %d of %d decisive rays on another triangle" % (
        where, len(fam.o), int((~same).sum()), int((~ok_e).sum()), int((~ok_f).sum()), int((dec & ~agree).sum()), int(dec.sum())))
    assert same.all(), "%s: the exact flavour differs from the oracle's brute force on %d rays (oracle's answer first):\n%s\n%s" % (
        where, int((~same).sum()), _failures(sol, want, ~same), _failures(sol, exact, ~same))
    assert ok_e.all(), "%s: exact flavour rejected on %d rays:\n%s\n%s" % (where, int((~ok_e).sum()), list(why_e[~ok_e][:5]), _failures(sol, exact, ~ok_e))
    assert ok_f.all(), "%s: fast flavour rejected on %d rays (a hit must lie within the pair's bt of the truth):\n%s\n%s" % (
        where, int((~ok_f).sum()), list(why_f[~ok_f][:5]), _failures(sol, fast, ~ok_f))
    assert (agree | ~dec).all(), "%s: on %d decisive rays the fast flavour's triangle is not the exact flavour's:\n%s\n%s" % (
        where, int((dec & ~agree).sum()), _failures(sol, fast, dec & ~agree), _failures(sol, exact, dec & ~agree))
    if fam.never_sky:
        assert not (exact[:, 0] == ray_truth.SKY).any() and not (fast[:, 0] == ray_truth.SKY).any(), "%s: a ray fell through the backdrop" % where
