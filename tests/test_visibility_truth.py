"""Visibility rays (k_shadow_rays, ShadowState in dev_trace.h) against the float64 truth of tests/ray_truth.py (solve_visibility) on segments chosen to be
hostile to what distinguishes the visibility walk from the closest-hit walk: children visited farthest first, 4-byte stack entries that are never culled, a
finite tmax = dist clipping the boxes from the first node on, the window t > kEps && t < dist, two triangles skipped by handle, leaves that re-read their
last triangle, the transparency product (binary64 in the exact flavour, binary32 in traversal order in the fast one) and the kBvhTriOpaque shortcut.

The truth walks no tree; the oracle's brute force (oracle_trace_shadow, use_bvh = 0) neither. Families: the closest-hit families of test_ray_truth.py as
segments that end before, behind, exactly at and one float32 step around the nearest occluder; segments that end on a named target with occluders at
dist (1 +- 1e-6) in flat boxes and coplanar duplicates; origins on a triangle with occluders at 0 .. 1e-3 around kEps; stacks of 1 .. 12 transparent sheets
with an opaque sheet at every position; non-finite rays and degenerate distances; queue shapes around the wave and workgroup sizes.

The device stores alpha and albedo as unorm16, so a nominal alpha of 0.5 is 32768 / 65535 and its factor no power of two: no stack of "dyadic" alphas has an
exact float32 product on the device. "Both flavours equal the product bit for bit" is therefore asserted where it is provable for the STORED factors: on the
decisive rays with at most two factors (one commutative multiplication, rounded once in binary32 as in binary64-then-binary32); with three or more factors
the acceptor's bounds apply.

NOT covered here: uv-dependent textured alpha (textures are constant-texel, which still takes the textured branch and the kBvhTriOpaque classification), the
ambient-reuse equivalence (a closest-hit ray answering a visibility question), the particle tree.

CPU tests: the acceptor on hand-made cases; the oracle's brute force passes it on every family, with the decisive share of interior-aimed rays >= 0.9 and at
most 1 % undecided rays (conditions on the families, not tuned to results); mutated answers are rejected.
GPU tests: per family and builder, the exact flavour is bit-identical to the oracle's brute force, both flavours pass the acceptor, and on decisive rays the
fast flavour is blocked exactly where the exact one is, with a product within the float32 product bound of the exact flavour's.
"""
import functools

import numpy as np
import pytest

import oracle_lib
import ray_truth
import test_ray_truth as rt
from luminary_amd import Host, scenes

NONE = 0xFFFFFFFF
FLT_MAX = np.float32(3.402823466e38)
INTERIOR, OTHER = 0, 2
K_EPS = np.float32(ray_truth.K_EPS)
BUILDERS = ["sah", "sah_gpu", "lbvh", "ploc"]


# ---- scenes with materials ----
def _vis_scene(meshes, instances, materials, textures=()):
    """meshes: list of (tris [n, 3, 3], material index per triangle); materials: list of dicts (alpha, albedo, coloured, tex = index into `textures` or None);
    textures: list of constant RGBA8 texels. Returns (host, view)."""
    host = Host()
    scenes.apply_benchmark_settings(host, 16, 16, 2, sky=(0.5, 0.5, 0.5))
    tex_ids = [host.add_texture(np.tile(np.array(t, dtype=np.uint8), (4, 4, 1)), 1.0) for t in textures]
    mat_ids = []
    for m in materials:
        mm = scenes._material(m.get("albedo", (0.6, 0.6, 0.6)), 0.6, alpha=m.get("alpha", 1.0))
        mm.colored_transparency = bool(m.get("coloured", False))
        if m.get("tex") is not None:
            mm.albedo_tex = tex_ids[m["tex"]]
        mat_ids.append(host.add_material(mm))
    ids = [host.add_mesh(np.asarray(t, dtype=np.float32).reshape(len(t), 9), np.asarray([mat_ids[k] for k in mi], dtype=np.uint16)) for (t, mi) in meshes]
    for (m, pos, rot, scale) in instances:
        host.new_instance(ids[m], pos, rot, scale)
    scenes.set_camera(host, (0.0, 0.0, 30.0), (0.0, 0.0, 0.0))
    return host, oracle_lib.with_luts(host.device_scene())


class VFamily:
    def __init__(self, o, d, dist, ids, tags, scene=None, view=None, host=None, num_tris=0, expect_transparent=False):
        self.o, self.d = np.ascontiguousarray(o, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32)
        self.dist, self.ids = np.ascontiguousarray(dist, dtype=np.float32), np.ascontiguousarray(ids, dtype=np.uint32)
        self.tags = np.asarray(tags)
        self.scene, self.view, self.host = scene, view, host
        self.expect_transparent = expect_transparent
        n = len(self.o)
        assert self.o.shape == self.d.shape == (n, 3) and self.dist.shape == (n,) and self.ids.shape == (n, 4) and len(self.tags) == n <= 20000
        assert num_tris <= 4000


def _no_ids(n):
    return np.full((n, 4), NONE, dtype=np.uint32)


def _flat_tri(centre, z, size=1.0, axis=2):
    """An axis-aligned triangle around `centre` (the two in-plane coordinates) in the plane coordinate[axis] = z: its box has zero thickness."""
    p = np.zeros((3, 3))
    b, c = (axis + 1) % 3, (axis + 2) % 3
    p[:, axis] = z
    p[:, b] = centre[0] + size * np.array([-1.0, 1.5, -1.0])
    p[:, c] = centre[1] + size * np.array([-1.0, -1.0, 1.5])
    return p


# 1. the closest-hit families as segments
SEGMENT_FAMILIES = ["axis_parallel", "flat_boxes", "far_shallow", "scale_1e-3", "scale_1", "scale_1e3", "instances"]


def family_segments(name):
    fam, host, view, sol, _ = rt._prepared(name)
    rng = np.random.RandomState(900 + SEGMENT_FAMILIES.index(name))
    n = len(fam.o)
    _, t, _ = sol.pair_values(np.where(sol.has_certain_hit, sol.the_acceptable, -1))
    t32 = t.astype(np.float32)
    kind = rng.randint(0, 6, n)
    dist = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                     [np.full(n, FLT_MAX), (0.5 * t).astype(np.float32), (2.0 * t).astype(np.float32), t32, np.nextafter(t32, np.float32(np.inf))],
                     np.nextafter(t32, np.float32(-np.inf))).astype(np.float32)
    dist[~sol.has_certain_hit] = FLT_MAX
    tags = np.where((fam.tags == rt.INTERIOR) & ((kind <= 2) | ~sol.has_certain_hit), INTERIOR, OTHER)  # a segment that ends AT the occluder is ambiguous by design
    return VFamily(fam.o, fam.d, dist, _no_ids(n), tags, sol.scene, view, host, sum(len(m) for m in fam.meshes))


# 2. segments that end on a target
def family_targets():
    rng = np.random.RandomState(201)
    tris, mats, rays = [], [], []
    planes = [0.0, 1.0, -3.0, 100.0, 0.37]
    for cell in range(150):
        axis = cell % 3
        centre = np.array([8.0 * (cell % 13) - 48.0, 8.0 * (cell // 13) - 24.0])
        z0 = np.float64(np.float32(planes[cell % len(planes)] + (0.0 if cell % 2 else 0.013 * cell)))
        mode = cell % 6  # 0 nothing in the way | 1 a coplanar duplicate | 2, 3 an occluder at dist (1 -+ 1e-6) | 4 an occluder half way | 5 a transparent one half way
        target = len(tris)
        tris.append(_flat_tri(centre, z0, 1.0, axis)); mats.append(0)
        height = rng.uniform(2.0, 9.0) * rng.choice([-1.0, 1.0])
        origin = np.zeros(3)
        origin[axis] = z0 + height
        origin[(axis + 1) % 3], origin[(axis + 2) % 3] = centre + rng.uniform(-0.3, 0.3, 2)
        origin = origin.astype(np.float32).astype(np.float64)
        h = origin[axis] - z0
        if mode == 1:
            tris.append(_flat_tri(centre, z0, 1.0, axis)); mats.append(0)
        elif mode in (2, 3):
            tris.append(_flat_tri(centre, origin[axis] - h * (1.0 - 1e-6 if mode == 2 else 1.0 + 1e-6), 1.2, axis)); mats.append(0)
        elif mode >= 4:
            tris.append(_flat_tri(centre, origin[axis] - 0.5 * h, 1.2, axis)); mats.append(0 if mode == 4 else 1)
        for _ in range(16):
            u, v = rng.uniform(0.15, 0.5), rng.uniform(0.15, 0.35)
            q = tris[target]
            p = np.float32(q[0]).astype(np.float64) + u * (np.float32(q[1]).astype(np.float64) - np.float32(q[0])) + v * (np.float32(q[2]).astype(np.float64) - np.float32(q[0]))
            d = rt._normalise32([p - origin])[0]
            dist = np.float32(np.linalg.norm(p - origin))
            named = rng.randint(0, 4) > 0
            rays.append((origin, d, dist, [0, target, NONE, NONE] if named else [NONE] * 4, INTERIOR if (mode in (0, 4, 5) and named) else OTHER))
    host, view = _vis_scene([(np.array(tris), mats)], [(0,) + rt.IDENTITY], [{"alpha": 1.0}, {"alpha": 0.5, "albedo": (0.9, 0.5, 0.25), "coloured": True}])
    return VFamily([r[0] for r in rays], [r[1] for r in rays], [r[2] for r in rays], [r[3] for r in rays], [r[4] for r in rays], ray_truth.scene_of_view(view), view, host,
                   len(tris), expect_transparent=True)


# 3. self and eps
EPS_OFFSETS = [0.0, 1e-8, float(K_EPS), float(np.nextafter(K_EPS, np.float32(1.0))), 1e-6, 1e-3]


def family_self_eps():
    rng = np.random.RandomState(202)
    tris, mats, rays = [], [], []
    for cell in range(144):
        axis = cell % 3
        centre = np.array([8.0 * (cell % 12) - 44.0, 8.0 * (cell // 12) - 44.0])
        z0 = [0.0, 1.0, -2.5][(cell // 3) % 3]
        base = len(tris)
        tris.append(_flat_tri(centre, z0, 1.0, axis)); mats.append(0)
        off = EPS_OFFSETS[(cell // 9) % len(EPS_OFFSETS)]
        side = 1.0 if (cell // 54) % 2 == 0 else -1.0
        tris.append(_flat_tri(centre, np.float32(z0) + np.float32(side * off), 1.3, axis)); mats.append(0 if cell % 2 else 1)
        for k in range(16):
            u, v = rng.uniform(0.15, 0.5), rng.uniform(0.15, 0.35)
            q = np.float32(tris[base])
            o = (q[0] + np.float32(u) * (q[1] - q[0]) + np.float32(v) * (q[2] - q[0])).astype(np.float32)
            o[axis] = np.float32(z0)  # on the triangle's plane, exactly
            d = np.zeros(3)
            d[axis] = side
            if k % 2:
                d[(axis + 1) % 3], d[(axis + 2) % 3] = rng.uniform(-0.4, 0.4, 2)
            d = rt._normalise32([d])[0]
            named = k % 4 < 2
            rays.append((o, d, FLT_MAX, [NONE, NONE, 0, base] if named else [NONE] * 4, INTERIOR if off in (0.0, 1e-8, 1e-3) else OTHER))
    host, view = _vis_scene([(np.array(tris), mats)], [(0,) + rt.IDENTITY], [{"alpha": 1.0}, {"alpha": 0.25}])
    return VFamily([r[0] for r in rays], [r[1] for r in rays], [r[2] for r in rays], [r[3] for r in rays], [r[4] for r in rays], ray_truth.scene_of_view(view), view, host,
                   len(tris), expect_transparent=True)


# 4. transparency stacks
STACK_TEXTURES = [(255, 255, 255, 0), (200, 120, 90, 128), (90, 90, 90, 255), (200, 120, 90, 0)]  # constant texels of alpha 0, 128 / 255, 1 and 0 again
STACK_MATERIALS = ([{"alpha": 1.0}] + [{"alpha": a} for a in (0.0, 0.25, 0.5, 0.75, 0.1, 0.3, 1.0 / 3.0, 0.9)] +
                   [{"alpha": a, "albedo": (0.9, 0.5, 0.25), "coloured": True} for a in (0.0, 0.25, 0.5, 0.75, 0.1, 0.3, 1.0 / 3.0, 0.9)] +
                   [{"tex": 0}, {"tex": 1}, {"tex": 1, "coloured": True}, {"tex": 2}, {"tex": 3, "coloured": True}])
DYADIC = [1, 2, 3, 4, 9, 10, 11, 12]  # nominal alphas 0, 0.25, 0.5, 0.75, plain and coloured
TRANSPARENT = list(range(1, 17)) + [17, 18, 19, 21]
OPAQUE_MATS = [0, 20]


def family_stacks():
    rng = np.random.RandomState(203)
    sheets, cells = [], []  # (cell, position, material)
    cell = 0
    for k in range(1, 13):
        for variant in range(12):
            pool = DYADIC if variant % 3 == 0 else TRANSPARENT
            mats = [pool[i] for i in rng.randint(0, len(pool), k)]
            if variant >= 6:  # an opaque sheet: at every position of the stack over the variants and the stack heights, stored last in the mesh (below)
                mats[(variant + k) % k] = OPAQUE_MATS[variant % 2]
            cells.append((cell, k, mats))
            cell += 1
    first, last = [], []
    for (c, k, mats) in cells:
        centre = np.array([7.0 * (c % 12) - 38.5, 7.0 * (c // 12) - 38.5])
        for j, m in enumerate(mats):
            (last if m in OPAQUE_MATS else first).append((_flat_tri(centre, float(j + 1), 1.0 + 0.05 * j), m))
    rng.shuffle(first)  # storage order is not the order along the ray
    allsheets = first + last
    tris, mats = np.array([s[0] for s in allsheets]), [s[1] for s in allsheets]
    rays = []
    for (c, k, _) in cells:
        centre = np.array([7.0 * (c % 12) - 38.5, 7.0 * (c // 12) - 38.5])
        for r in range(20):
            o = np.float32([centre[0] + rng.uniform(-0.3, 0.3), centre[1] + rng.uniform(-0.3, 0.3), 0.0 if r % 2 else 13.5])
            d = np.array([0.0, 0.0, 1.0 if r % 2 else -1.0])
            if r % 4 >= 2:
                d[0:2] = rng.uniform(-0.02, 0.02, 2)
            d = rt._normalise32([d])[0]
            dist = FLT_MAX if r % 5 else np.float32(rng.randint(1, 13) + 0.5)
            rays.append((o, d, dist, [NONE] * 4, INTERIOR))
    host, view = _vis_scene([(tris, mats)], [(0,) + rt.IDENTITY], STACK_MATERIALS, STACK_TEXTURES)
    return VFamily([r[0] for r in rays], [r[1] for r in rays], [r[2] for r in rays], [r[3] for r in rays], [r[4] for r in rays], ray_truth.scene_of_view(view), view, host,
                   len(tris), expect_transparent=True)


# 5. non-finite and degenerate input
def family_degenerate():
    rng = np.random.RandomState(204)
    soup = rt._soup(rng, 120, 4.0).astype(np.float32)  # no backdrop: a ray that crosses nothing, or transparent surfaces only, has to say so under every dist
    mats = list(rng.randint(0, 3, len(soup)))
    n = 1200
    idx = rng.randint(0, len(soup), n)
    tgt = rt._targets(rng, soup, idx, 0.2, 0.7)
    o = rng.uniform(-8.0, 8.0, (n, 3)).astype(np.float32)
    d = rt._normalise32(tgt - o.astype(np.float64))
    dist = np.array([0.0, 1e-45, 1e-40, 1e-8, FLT_MAX, np.inf], dtype=np.float32)[rng.randint(0, 6, n)]
    tags = np.full(n, INTERIOR)
    bad = rng.randint(0, n, 400)  # NaN or +-inf in one component of the origin or of the direction
    comp = rng.randint(0, 6, 400)
    val = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[rng.randint(0, 3, 400)]
    for b, c, v in zip(bad, comp, val):
        (o if c < 3 else d)[b, c % 3] = v
    dist[bad[:200]] = FLT_MAX
    host, view = _vis_scene([(soup, mats)], [(0,) + rt.IDENTITY], [{"alpha": 1.0}, {"alpha": 0.5}, {"alpha": 0.3, "albedo": (0.9, 0.5, 0.25), "coloured": True}])
    return VFamily(o, d, dist, _no_ids(n), tags, ray_truth.scene_of_view(view), view, host, len(soup), expect_transparent=True)


FAMILIES = {("segments_" + n): functools.partial(family_segments, n) for n in SEGMENT_FAMILIES}
FAMILIES.update({"targets": family_targets, "self_eps": family_self_eps, "stacks": family_stacks, "degenerate": family_degenerate})


@functools.lru_cache(maxsize=None)
def _prepared(name):
    """(family, solution, the oracle's brute-force answers): computed once, shared by the tests, never modified."""
    fam = FAMILIES[name]()
    kind, factor = ray_truth.surface_factors(fam.view)
    sol = ray_truth.solve_visibility(fam.scene, kind, factor, fam.o, fam.d, fam.dist, fam.ids)
    want = oracle_lib.trace_shadow(fam.view, fam.o, fam.d, fam.dist, fam.ids, use_bvh=False)
    want.setflags(write=False)
    return fam, sol, want


def _describe(fam, sol, answers, bad, why=None, limit=5):
    out = []
    for i in np.nonzero(bad)[0][:limit]:
        out.append("ray %d o=%s d=%s dist=%.9g ids=%s | truth: must block %s, may block %s, %d certain factor(s) product %s, %d ambiguous | answer %s%s" % (
            i, [float(x) for x in fam.o[i]], [float(x) for x in fam.d[i]], float(fam.dist[i]), [int(x) for x in fam.ids[i]], bool(sol.must_block[i]), bool(sol.may_block[i]),
            int(sol.k_certain[i]), [float(x) for x in sol.product[i]], int(sol.num_ambiguous[i]), [float(x) for x in answers[i]], (" | " + str(why[i])) if why is not None else ""))
    return "\n".join(out)


# ---- CPU: the acceptor on known answers ----
def _one(tris, mats, materials, o, d, dist, ids=None, textures=()):
    host, view = _vis_scene([(np.array(tris), mats)], [(0,) + rt.IDENTITY], materials, textures)
    kind, factor = ray_truth.surface_factors(view)
    o, d = np.float32([o]), np.float32([d])
    dist, ids = np.float32([dist]), np.array([ids if ids is not None else [NONE] * 4], dtype=np.uint32)
    sol = ray_truth.solve_visibility(ray_truth.scene_of_view(view), kind, factor, o, d, dist, ids)
    got = oracle_lib.trace_shadow(view, o, d, dist, ids, use_bvh=False)
    return sol, got, factor


def _ok(sol, answer, fast=False):
    return bool(sol.check(np.float32([answer]), fast)[0][0])


def test_acceptor_known_answers():
    half = {"alpha": 0.5}
    tint = {"alpha": 0.25, "albedo": (0.9, 0.5, 0.25), "coloured": True}
    opaque = {"alpha": 1.0}
    down = ((0.0, 0.0, 10.0), (0.0, 0.0, -1.0))
    # one sheet: the answer is its factor, 1 - 32768 / 65535 as the device decodes it
    sol, got, f = _one([_flat_tri((0, 0), 5.0)], [0], [half], *down, FLT_MAX)
    assert sol.decisive[0] and not sol.must_block[0] and sol.k_certain[0] == 1
    assert abs(float(f[0, 0]) - 0.5) < 1e-5 and f[0, 0] != 0.5
    for fast in (False, True):
        assert _ok(sol, f[0], fast) and _ok(sol, got[0], fast)
        assert not _ok(sol, (1.0, 1.0, 1.0), fast) and not _ok(sol, (0.0, 0.0, 0.0), fast) and not _ok(sol, (0.5, 0.5, 0.5), fast)
        assert not _ok(sol, np.nextafter(f[0], np.float32(1.0)), fast), "one factor: no rounding at all"
    # two sheets, one coloured: the product of two float32 factors is exact in binary64 and rounded once
    sol, got, f = _one([_flat_tri((0, 0), 5.0), _flat_tri((0, 0), 3.0)], [0, 1], [half, tint], *down, FLT_MAX)
    p = (f[0].astype(np.float64) * f[1].astype(np.float64)).astype(np.float32)
    assert sol.decisive[0] and sol.k_certain[0] == 2 and np.array_equal(sol.expected()[0], p) and np.array_equal(got[0], p)
    assert _ok(sol, p) and _ok(sol, p, True) and not _ok(sol, f[0]) and not _ok(sol, f[1]) and not _ok(sol, p * np.float32(1.001), True)
    assert not _ok(sol, np.nextafter(p, np.float32(0.0))), "the exact flavour rounds once: the neighbouring float is rejected"
    # an opaque sheet behind dist does not count; in front of it, it blocks
    sheets = [_flat_tri((0, 0), 5.0), _flat_tri((0, 0), 2.0)]
    sol, got, f = _one(sheets, [0, 1], [half, opaque], *down, 7.0)
    assert sol.decisive[0] and not sol.must_block[0] and _ok(sol, f[0]) and np.array_equal(got[0], f[0]) and not _ok(sol, (0.0, 0.0, 0.0))
    sol, got, _ = _one(sheets, [0, 1], [half, opaque], *down, 9.0)
    assert sol.decisive[0] and sol.must_block[0] and _ok(sol, (0.0, 0.0, 0.0)) and np.all(got[0] == 0.0) and not _ok(sol, f[0]) and not _ok(sol, (1.0, 1.0, 1.0))
    # an opaque sheet inside eps of the origin does not count; 1e-3 away it blocks; at t = eps exactly the window is open (t > eps is false), which float32
    # decides on a rounded t: the truth calls it ambiguous and accepts the oracle's "not crossed"
    for off, blocks in ((1e-8, False), (1e-3, True)):
        sol, got, _ = _one([_flat_tri((0, 0), off)], [0], [opaque], (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), FLT_MAX)
        assert sol.decisive[0] and bool(sol.must_block[0]) == blocks and _ok(sol, got[0]) and _ok(sol, (0.0,) * 3) == blocks and _ok(sol, (1.0,) * 3) != blocks, off
    sol, got, _ = _one([_flat_tri((0, 0), float(K_EPS))], [0], [opaque], (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), FLT_MAX)
    assert not sol.must_block[0] and np.all(got[0] == 1.0) and _ok(sol, got[0]) and not _ok(sol, (0.5,) * 3)
    # the target is skipped, and so is self; unnamed, the target at dist is ambiguous: either answer
    tri = [_flat_tri((0, 0), 5.0)]
    sol, got, _ = _one(tri, [0], [opaque], *down, 5.0, [0, 0, NONE, NONE])
    assert sol.decisive[0] and not sol.must_block[0] and np.all(got[0] == 1.0) and _ok(sol, (1.0,) * 3) and not _ok(sol, (0.0,) * 3)
    sol, got, _ = _one(tri, [0], [opaque], *down, FLT_MAX, [NONE, NONE, 0, 0])
    assert sol.decisive[0] and not sol.must_block[0] and np.all(got[0] == 1.0) and not _ok(sol, (0.0,) * 3)
    sol, got, _ = _one(tri, [0], [opaque], (0.3, 0.1, 10.0), tuple(rt._normalise32([[0.01, 0.02, -1.0]])[0]), np.float32(5.00125), None)
    assert _ok(sol, got[0])
    # a constant texture of alpha 1 is opaque, of alpha 0 absent; a non-finite ray crosses nothing
    sol, got, _ = _one([_flat_tri((0, 0), 5.0), _flat_tri((0, 0), 3.0)], [0, 1], [{"tex": 0}, {"tex": 1}], *down, FLT_MAX, textures=[(9, 9, 9, 255), (255, 255, 255, 0)])
    assert sol.decisive[0] and sol.must_block[0] and np.all(got[0] == 0.0)
    sol, got, _ = _one([_flat_tri((0, 0), 3.0)], [0], [{"tex": 0}], *down, FLT_MAX, textures=[(255, 255, 255, 0)])
    assert sol.decisive[0] and sol.k_certain[0] == 0 and np.all(got[0] == 1.0) and _ok(sol, (1.0,) * 3)
    sol, got, _ = _one(tri, [0], [opaque], (0.0, np.nan, 10.0), (0.0, 0.0, -1.0), FLT_MAX)
    assert sol.decisive[0] and np.all(got[0] == 1.0) and _ok(sol, (1.0,) * 3) and not _ok(sol, (0.0,) * 3)


# ---- CPU: the oracle's brute force alone, per family ----
@pytest.mark.parametrize("name", list(FAMILIES))
def test_the_reference_alone_passes_and_the_truth_decides(name):
    fam, sol, want = _prepared(name)
    ok, why = sol.check(want)
    aimed = fam.tags == INTERIOR
    blocked = np.all(want == 0.0, axis=1)
    print("%s: %d rays, %d pairs per ray | oracle brute force rejected %d | decisive share of the %d interior-aimed rays %.4f, of all rays %.4f | undecided %.4f | blocked %.3f, "
          "clear %.3f, transparent %.3f" % (name, len(fam.o), fam.scene.num_pairs, int((~ok).sum()), int(aimed.sum()), sol.decisive[aimed].mean(), sol.decisive.mean(),
                                          sol.undecided.mean(), blocked.mean(), np.all(want == 1.0, axis=1).mean(), (~blocked & ~np.all(want == 1.0, axis=1)).mean()))
    assert ok.all(), "float32 brute force rejected by the truth (%d rays):\n%s" % (int((~ok).sum()), _describe(fam, sol, want, ~ok, why))
    assert aimed.sum() > 0 and sol.decisive[aimed].mean() >= 0.9
    assert sol.undecided.mean() <= 0.01
    dec = sol.decisive
    assert np.array_equal(sol.expected()[dec].view(np.uint32), want[dec].view(np.uint32)), "on decisive rays the truth names the answer itself"
    assert blocked[dec].any() and (~blocked[dec]).any()


@pytest.mark.parametrize("name", list(FAMILIES))
def test_the_acceptor_can_fail(name):
    fam, sol, want = _prepared(name)
    dec = sol.decisive & sol.finite
    # (1, 1, 1) where an opaque pair is certainly crossed
    must = sol.must_block
    mutated = want.copy()
    mutated[must] = 1.0
    assert must.sum() > 0 and not sol.check(mutated)[0][must].any()
    # 0 where nothing is possibly crossed
    clear = dec & ~must & (sol.k_certain == 0)
    mutated = want.copy()
    mutated[clear] = 0.0
    assert clear.sum() > 0 and not sol.check(mutated)[0][clear].any()
    # one factor dropped, one factor doubled
    prod = dec & ~must & (sol.k_certain >= 1)
    print("%s: mutated %d blocked rays to (1, 1, 1), %d clear rays to 0, %d products by one factor" % (name, int(must.sum()), int(clear.sum()), int(prod.sum())))
    if fam.expect_transparent:
        assert prod.sum() > 0
    if prod.any():
        f = sol.one_factor.astype(np.float64)
        assert (f[prod] <= 0.91).all()  # every factor is at least 9 % off 1: far outside either bound
        for mutated in ((want.astype(np.float64) / f).astype(np.float32), (want.astype(np.float64) * f).astype(np.float32)):
            for fast in (False, True):
                assert not sol.check(mutated, fast)[0][prod].any()


def _order_independent(sol):
    """Decisive, unblocked rays with at most two factors: one float32 multiplication is commutative and rounds once, like the binary64 product rounded once, so
    both flavours must return the same bits whatever the traversal order."""
    return sol.decisive & sol.finite & ~sol.must_block & (sol.k_certain <= 2)


def test_stack_family_covers_what_it_is_for():
    fam, sol, want = _prepared("stacks")
    dec = sol.decisive
    assert sol.k_certain[dec].max() == ray_truth.MAX_FACTORS and set(range(0, 13)) <= set(int(k) for k in sol.k_certain[dec])
    assert float(np.min(want[np.all(want > 0.0, axis=1)])) > 2.0 ** -100  # nothing near the underflow threshold
    kind, factor = ray_truth.surface_factors(fam.view)
    assert factor[kind == ray_truth.FACTOR].min() >= 2.0 ** -6
    assert (kind == ray_truth.OPAQUE).sum() >= 60 and (kind == ray_truth.ABSENT).sum() > 0
    single = _order_independent(sol)
    assert single.sum() > 100


# ---- GPU ----
def _trace_both(fam, builder, order=None):
    from luminary_amd.core import Core
    core = Core(0)
    try:
        core.set_bvh_builder(builder)
        core.upload(fam.view)
        used = core.bvh_meshes_by_builder()
        assert builder == "sah" or used["lbvh"] >= 1, "%s: no mesh was built on the device: %s" % (builder, used)
        core.set_flavour("exact")
        exact = core.trace_visibility_host(fam.o, fam.d, fam.dist, fam.ids, order)
        core.set_flavour("fast")
        fast = core.trace_visibility_host(fam.o, fam.d, fam.dist, fam.ids, order)
    finally:
        core.close()
    return exact, fast


@pytest.mark.gpu
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", list(FAMILIES))
def test_gpu_visibility_against_the_truth(name, builder):
    fam, sol, want = _prepared(name)
    exact, fast = _trace_both(fam, builder)
    where = "%s, %s" % (name, builder)
    same = (exact.view(np.uint32) == want.view(np.uint32)).all(axis=1)
    ok_e, why_e = sol.check(exact)
    ok_f, why_f = sol.check(fast, fast=True)
    dec = sol.decisive
    blocked_e, blocked_f = np.all(exact == 0.0, axis=1), np.all(fast == 0.0, axis=1)
    ku = np.maximum(sol.k_certain - 1, 0) * ray_truth.U
    bound = (ku / (1.0 - ku))[:, None] * np.abs(exact.astype(np.float64))
    close = (np.abs(fast.astype(np.float64) - exact.astype(np.float64)) <= bound).all(axis=1)
    exactly = _order_independent(sol)
    bitwise = (fast.view(np.uint32) == exact.view(np.uint32)).all(axis=1) & (exact.view(np.uint32) == sol.expected().view(np.uint32)).all(axis=1)
    print("%s: %d rays | exact: %d differ from the brute force, %d rejected | fast: %d rejected; of %d decisive rays %d blocked differently, %d products outside the bound, "
          "%d of %d order-independent products not bit-identical" % (where, len(fam.o), int((~same).sum()), int((~ok_e).sum()), int((~ok_f).sum()), int(dec.sum()),
                                                                    int((dec & (blocked_e != blocked_f)).sum()), int((dec & ~close).sum()), int((exactly & ~bitwise).sum()), int(exactly.sum())))
    assert not np.isnan(exact).any() and not np.isnan(fast).any(), "%s: a ray nobody answered" % where
    assert same.all(), "%s: the exact flavour differs from the oracle's brute force on %d rays (the oracle's answer first):\n%s\n%s" % (
        where, int((~same).sum()), _describe(fam, sol, want, ~same), _describe(fam, sol, exact, ~same))
    assert ok_e.all(), "%s: exact flavour rejected on %d rays:\n%s" % (where, int((~ok_e).sum()), _describe(fam, sol, exact, ~ok_e, why_e))
    assert ok_f.all(), "%s: fast flavour rejected on %d rays:\n%s" % (where, int((~ok_f).sum()), _describe(fam, sol, fast, ~ok_f, why_f))
    bad = dec & (blocked_e != blocked_f)
    assert not bad.any(), "%s: on %d decisive rays the fast flavour is blocked where the exact one is not, or the other way round:\n%s" % (where, int(bad.sum()), _describe(fam, sol, fast, bad))
    bad = dec & ~close
    assert not bad.any(), "%s: on %d decisive rays the fast product is outside (k - 1) u / (1 - (k - 1) u) of the exact flavour's:\n%s\n%s" % (
        where, int(bad.sum()), _describe(fam, sol, fast, bad), _describe(fam, sol, exact, bad))
    bad = exactly & ~bitwise
    assert not bad.any(), "%s: %d order-independent products are not bit-identical in both flavours:\n%s" % (where, int(bad.sum()), _describe(fam, sol, fast, bad))


@pytest.mark.gpu
def test_gpu_queue_shapes():
    """Every ray answered once whatever the number of items (around the wave of 64, the chunk of 256 and the workgroup of 1024), results independent of n, and
    a permuted work order gives the same answers."""
    from luminary_amd.core import Core
    fam, sol, want = _prepared("stacks")
    rng = np.random.RandomState(77)
    core = Core(0)
    try:
        core.upload(fam.view)
        for flavour in ("exact", "fast"):
            core.set_flavour(flavour)
            full = core.trace_visibility_host(fam.o, fam.d, fam.dist, fam.ids)
            assert not np.isnan(full).any()
            if flavour == "exact":
                assert np.array_equal(full.view(np.uint32), want.view(np.uint32))
            perm = rng.permutation(len(fam.o)).astype(np.uint32)
            assert np.array_equal(core.trace_visibility_host(fam.o, fam.d, fam.dist, fam.ids, perm).view(np.uint32), full.view(np.uint32)), flavour
            assert core.trace_visibility_host(fam.o[:0], fam.d[:0], fam.dist[:0], fam.ids[:0]).shape == (0, 3)
            for n in (1, 63, 64, 65, 257, 1025):
                got = core.trace_visibility_host(fam.o[:n], fam.d[:n], fam.dist[:n], fam.ids[:n])
                assert not np.isnan(got).any(), "%s, n = %d: a ray nobody answered" % (flavour, n)
                assert np.array_equal(got.view(np.uint32), full[:n].view(np.uint32)), "%s, n = %d" % (flavour, n)
                perm = rng.permutation(n).astype(np.uint32)
                assert np.array_equal(core.trace_visibility_host(fam.o[:n], fam.d[:n], fam.dist[:n], fam.ids[:n], perm).view(np.uint32), full[:n].view(np.uint32)), (flavour, n)
    finally:
        core.close()
