"""The light-BVH query of BSDF-sampled directions (light_query in dev_trace.h, through k_light_query_probe) against the float64 truth of tests/ray_truth.py
(solve_lights). light_query walks the light tree twice with tmax = t* and accepts t <= t*: the opaque light that defined t* sits exactly on the cull
boundary of the second pass, and the within / reachable comparisons have to keep it.

Families, each on a scene of 8 .. 64 emissive triangles: axis-aligned flat lights stacked along the ray - the nearest opaque one at t*, transparent coloured
ones before it, at it (a coplanar duplicate) and behind it, fully transparent uncoloured ones among them -, with straight, dead-component (test_ray_truth.DEAD)
and oblique directions; rays that start on a light with self named; rays that cross no light; non-finite rays. Every ray is asked with 16 random numbers,
so the hash pick is exercised.

CPU tests: known answers; the oracle's brute force alone passes the acceptor with a decisive share >= 0.9 on aimed rays; mutated answers are rejected.
GPU tests: per family and builder, the exact flavour equals the oracle's brute force, both flavours are accepted, and on decisive rays both flavours give
the truth's (id, num_hits). (The light tree itself is always built on the host; the builder parameter varies the scene trees next to it.)

NOT covered here: uv-dependent textured alpha, the ambient-reuse equivalence, the particle tree.
"""
import functools

import numpy as np
import pytest

import oracle_lib
import ray_truth
import test_ray_truth as rt
from luminary_amd import Host, scenes

NONE = 0xFFFFFFFF
AIMED, OTHER = 0, 2
RANDOMS = 16
BUILDERS = ["sah", "sah_gpu", "lbvh", "ploc"]
OPAQUE, TINT, CLEAR = 0, 1, 2  # emissive materials: alpha 1 | alpha 0.5 coloured | alpha 0 uncoloured (absent for the query)


def _light_scene(tris, mats):
    host = Host()
    scenes.apply_benchmark_settings(host, 16, 16, 2, sky=(0.5, 0.5, 0.5))
    ids = []
    for alpha, coloured in ((1.0, False), (0.5, True), (0.0, False)):
        m = scenes._material((0.9, 0.5, 0.25), 0.7, emission=(5.0, 4.0, 3.0), alpha=alpha)
        m.colored_transparency = coloured
        ids.append(host.add_material(m))
    mesh = host.add_mesh(np.asarray(tris, dtype=np.float32).reshape(len(tris), 9), np.asarray([ids[k] for k in mats], dtype=np.uint16))
    host.new_instance(mesh, *rt.IDENTITY)
    scenes.set_camera(host, (0.0, 0.0, 30.0), (0.0, 0.0, 0.0))
    return host, oracle_lib.with_luts(host.device_scene())


def _flat(centre, z, size=1.0, axis=2):
    p = np.zeros((3, 3))
    p[:, axis] = z
    p[:, (axis + 1) % 3] = centre[0] + size * np.array([-1.0, 1.5, -1.0])
    p[:, (axis + 2) % 3] = centre[1] + size * np.array([-1.0, -1.0, 1.5])
    return p


# stacks along +axis, bottom to top: (height, material)
STACKS = [
    [(1.0, TINT), (2.0, CLEAR), (3.0, OPAQUE), (3.0, TINT), (4.0, TINT), (5.0, OPAQUE)],        # t* at 3 with a coplanar transparent duplicate
    [(1.0, CLEAR), (2.0, TINT), (2.5, TINT), (3.0, TINT), (4.0, OPAQUE), (4.0, OPAQUE)],        # two opaque lights at t*: coplanar duplicates
    [(1.0, OPAQUE), (2.0, TINT), (3.0, OPAQUE)],                                                # the first light is opaque
    [(1.0, TINT), (2.0, TINT), (3.0, CLEAR), (4.0, TINT)],                                      # no opaque light: t* = FLT_MAX
    [(0.5, TINT), (100.25, OPAQUE), (100.25, TINT), (1e4, TINT)],                               # large coordinates
    [(1.0, CLEAR), (2.0, CLEAR)],                                                               # nothing to count
    [(1.0, TINT), (1.0 + 1e-6, OPAQUE), (1.0 + 2e-6, TINT)],                                    # lights within a few float32 steps of t*
    [(2.0, OPAQUE), (2.0, TINT), (2.0, TINT), (2.0, CLEAR), (2.0, OPAQUE)],                     # everything in one plane
    [(1.0, TINT), (2.0, TINT), (3.0, OPAQUE), (4.0, TINT), (5.0, OPAQUE)],                      # t* at 3, lights clearly before and behind it
    [(1.0, CLEAR), (2.0, TINT), (3.0, OPAQUE), (3.5, TINT)],
]
# Stacks with a light AT t* other than the opaque one that defines it (or within a few float32 steps) are ambiguous by design: whether t <= t* holds there is
# decided by float32 rounding. Their rays are not "aimed" rays for the decisive share.
CLEAR_CUT = [False, False, True, True, False, True, False, False, True, True]


class LFamily:
    def __init__(self, tris, mats, o, d, self_handles, tags):
        assert 8 <= len(tris) <= 64
        self.host, self.view = _light_scene(tris, mats)
        assert self.view.num_lights == len(tris), "every emissive triangle is a light: %d of %d" % (self.view.num_lights, len(tris))
        rng = np.random.RandomState(len(o))
        self.o = np.repeat(np.ascontiguousarray(o, dtype=np.float32), RANDOMS, axis=0)
        self.d = np.repeat(np.ascontiguousarray(d, dtype=np.float32), RANDOMS, axis=0)
        self.self_handles = np.repeat(np.ascontiguousarray(self_handles, dtype=np.uint32), RANDOMS, axis=0)
        self.tags = np.repeat(np.asarray(tags), RANDOMS)
        self.randoms = rng.uniform(0.0, 1.0, len(self.o)).astype(np.float32)
        assert len(self.o) <= 20000


def _stack_scene(axis):
    tris, mats, cells = [], [], []
    for c, stack in enumerate(STACKS):
        centre = np.array([9.0 * (c % 3) - 9.0, 9.0 * (c // 3) - 9.0])
        first = len(tris)
        for (z, m) in stack:
            tris.append(_flat(centre, z, 1.0, axis)); mats.append(m)
        cells.append((centre, first, len(stack)))
    return tris, mats, cells


def family_stacked(axis, directions):
    """directions: 'straight' (dead components exactly 0), 'dead' (the dead components of test_ray_truth.DEAD), 'oblique'."""
    rng = np.random.RandomState(300 + axis)
    tris, mats, cells = _stack_scene(axis)
    o, d, sh, tags = [], [], [], []
    for c, (centre, first, count) in enumerate(cells):
        for r in range(24):
            org = np.zeros(3)
            org[axis] = -2.0 if r % 3 else 0.25
            org[(axis + 1) % 3], org[(axis + 2) % 3] = centre + rng.uniform(-0.3, 0.3, 2)
            dd = np.zeros(3)
            dd[axis] = 1.0
            if directions == "dead":
                dd[(axis + 1) % 3], dd[(axis + 2) % 3] = rng.choice(rt.DEAD, 2)
            elif directions == "oblique":
                dd[(axis + 1) % 3], dd[(axis + 2) % 3] = rng.uniform(-0.03, 0.03, 2)
                dd = rt._normalise32([dd])[0]
            o.append(org); d.append(dd); sh.append([NONE, NONE]); tags.append(AIMED if CLEAR_CUT[c] else OTHER)
    return LFamily(tris, mats, o, d, sh, tags)


def family_from_lights():
    """Rays that start on a light, self named and not named, towards the lights above it and away from them; rays that cross no light; non-finite rays."""
    rng = np.random.RandomState(310)
    tris, mats, cells = _stack_scene(2)
    o, d, sh, tags = [], [], [], []
    for c, (centre, first, count) in enumerate(cells):
        for j in range(count):
            for r in range(4):
                q = np.float32(tris[first + j])
                org = (q[0] + np.float32(rng.uniform(0.2, 0.4)) * (q[1] - q[0]) + np.float32(rng.uniform(0.2, 0.4)) * (q[2] - q[0])).astype(np.float32)
                org[2] = q[0][2]
                dd = rt._normalise32([[rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), 1.0 if r % 2 else -1.0]])[0]
                o.append(org); d.append(dd); sh.append([0, first + j] if r < 2 else [NONE, NONE]); tags.append(AIMED if CLEAR_CUT[c] else OTHER)
    for _ in range(40):  # past every stack
        o.append(rng.uniform(-3.0, 3.0, 3) + np.array([40.0, 40.0, -5.0])); d.append(rt._normalise32([rng.normal(size=3)])[0]); sh.append([NONE, NONE]); tags.append(AIMED)
    for k in range(36):  # NaN or +-inf in one component
        org, dd = np.float32([cells[0][0][0], cells[0][0][1], -2.0]), np.float32([0.0, 0.0, 1.0])
        (org if k % 6 < 3 else dd)[k % 3] = [np.nan, np.inf, -np.inf][(k // 6) % 3]
        o.append(org); d.append(dd); sh.append([NONE, NONE]); tags.append(OTHER)
    return LFamily(tris, mats, o, d, sh, tags)


FAMILIES = {"stacked_z_straight": functools.partial(family_stacked, 2, "straight"), "stacked_x_dead": functools.partial(family_stacked, 0, "dead"),
            "stacked_y_dead": functools.partial(family_stacked, 1, "dead"), "stacked_z_oblique": functools.partial(family_stacked, 2, "oblique"),
            "from_lights": family_from_lights}


@functools.lru_cache(maxsize=None)
def _prepared(name):
    fam = FAMILIES[name]()
    sol = ray_truth.solve_lights(fam.view, fam.o, fam.d, fam.self_handles, fam.randoms)
    ids, hits = oracle_lib.trace_light_bvh(fam.view, fam.o, fam.d, fam.self_handles, fam.randoms, use_bvh=False)
    ids.setflags(write=False); hits.setflags(write=False)
    return fam, sol, ids, hits


def _describe(fam, sol, ids, hits, bad, why=None, limit=5):
    return "\n".join("ray %d o=%s d=%s self=%s random=%r | certain %s possible %s | answer (%d, %d)%s" % (
        i, [float(x) for x in fam.o[i]], [float(x) for x in fam.d[i]], [int(x) for x in fam.self_handles[i]], float(fam.randoms[i]), list(np.nonzero(sol.certain[i])[0]),
        list(np.nonzero(sol.possible[i])[0]), int(ids[i]), int(hits[i]), (" | " + str(why[i])) if why is not None else "") for i in np.nonzero(bad)[0][:limit])


# ---- CPU ----
def test_the_hash_is_the_oracles():
    rng = np.random.RandomState(5)
    ctr = rng.randint(0, 2 ** 32, 200, dtype=np.uint64).astype(np.uint32)
    want = np.array([oracle_lib.lib().oracle_squares32(0xfcbd6e15, int(c)) for c in ctr], dtype=np.uint32)
    assert np.array_equal(ray_truth.squares32(0xfcbd6e15, ctr), want)


def test_known_answers():
    fam, sol, ids, hits = _prepared("stacked_z_straight")
    a = oracle_lib.view_arrays(fam.view)
    handles = a["light_tri_handles"].reshape(-1, 2)
    light_of = {int(h[1]): l for l, h in enumerate(handles)}  # scene triangle -> light id (one instance)
    per_cell = 24 * RANDOMS
    # cell 0 from below the stack: the tint at 1 and the opaque light at 3 are certain, the opaque light's coplanar tinted duplicate is possible (t <= t* is
    # decided by two float32 distances that the truth only knows to within their bounds); the clear one at 2 is absent, 4 and 5 lie behind t*
    rows = np.arange(per_cell)[fam.o[:per_cell, 2] == -2.0]
    for i in rows:
        assert not sol.decisive[i] and list(np.nonzero(sol.certain[i])[0]) == sorted(light_of[t] for t in (0, 2)) and hits[i] == 3
        assert list(np.nonzero(sol.possible[i])[0]) == sorted(light_of[t] for t in (0, 2, 3))
    # cell 3: no opaque light, three tinted ones and an absent one: 16 random numbers per ray pick every candidate at least once
    rows = 3 * per_cell + np.arange(per_cell)[fam.o[3 * per_cell:4 * per_cell, 2] == -2.0]
    want = sorted(light_of[cells_first(3) + t] for t in (0, 1, 3))
    for i in rows:
        assert sol.decisive[i] and list(np.nonzero(sol.certain[i])[0]) == want and hits[i] == 3 and ids[i] == ray_truth.light_pick(want, sol.random_bits[i])
    assert len(set(int(x) for x in ids[rows])) == 3
    # cell 5: only fully transparent uncoloured lights - nothing to count
    rows = 5 * per_cell + np.arange(per_cell)
    assert (hits[rows] == 0).all() and (ids[rows] == ray_truth.LIGHT_INVALID).all() and sol.decisive[rows].all()
    # cell 2: the first light is opaque, it alone counts; cell 8 from below: two tints and the opaque light at 3
    rows = 2 * per_cell + np.arange(per_cell)
    assert (hits[rows] == 1).all() and (ids[rows] == light_of[cells_first(2)]).all() and sol.decisive[rows].all()
    rows = 8 * per_cell + np.arange(per_cell)[fam.o[8 * per_cell:9 * per_cell, 2] == -2.0]
    assert (hits[rows] == 3).all() and sol.decisive[rows].all() and set(int(x) for x in ids[rows]) <= set(light_of[cells_first(8) + t] for t in (0, 1, 2))


def cells_first(c):
    return sum(len(s) for s in STACKS[:c])


@pytest.mark.parametrize("name", list(FAMILIES))
def test_the_reference_alone_passes_and_the_truth_decides(name):
    fam, sol, ids, hits = _prepared(name)
    ok, why = sol.check(ids, hits)
    aimed = fam.tags == AIMED
    print("%s: %d rays on %d lights | oracle brute force rejected %d | decisive share of the %d aimed rays %.4f | num_hits 0: %.3f, 1: %.3f, more: %.3f" % (
        name, len(fam.o), fam.view.num_lights, int((~ok).sum()), int(aimed.sum()), sol.decisive[aimed].mean(), (hits == 0).mean(), (hits == 1).mean(), (hits > 1).mean()))
    assert ok.all(), "brute force rejected by the truth (%d rays):\n%s" % (int((~ok).sum()), _describe(fam, sol, ids, hits, ~ok, why))
    assert sol.decisive[aimed].mean() >= 0.9
    want_ids, want_hits = sol.expected()
    dec = sol.decisive
    assert np.array_equal(want_ids[dec], ids[dec]) and np.array_equal(want_hits[dec], hits[dec]), "on decisive rays the truth names the answer itself"
    assert (hits[dec] > 1).any()


@pytest.mark.parametrize("name", list(FAMILIES))
def test_the_acceptor_can_fail(name):
    fam, sol, ids, hits = _prepared(name)
    dec = sol.decisive
    # the count off by one, either way
    for delta in (1, -1):
        sel = dec & (hits.astype(np.int64) + delta >= 0)
        mutated = (hits.astype(np.int64) + delta).clip(0).astype(np.uint32)
        assert sel.sum() > 0 and not sol.check(ids, mutated)[0][sel & (mutated != hits)].any()
    # a light behind t*: any light that is not a possible candidate
    behind = dec & (hits > 0) & ~sol.possible.all(axis=1)
    mutated = ids.copy()
    mutated[behind] = np.argmin(sol.possible[behind], axis=1)
    assert behind.sum() > 0 and not sol.check(mutated, hits)[0][behind].any()
    # invalid where a candidate is certain
    some = sol.certain.any(axis=1)
    mutated = ids.copy()
    mutated[some] = ray_truth.LIGHT_INVALID
    print("%s: mutated the count of %d rays, the light of %d, the validity of %d" % (name, int(dec.sum()), int(behind.sum()), int(some.sum())))
    assert some.sum() > 0 and not sol.check(mutated, hits)[0][some].any()


# ---- GPU ----
@pytest.mark.gpu
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", list(FAMILIES))
def test_gpu_light_queries_against_the_truth(name, builder):
    from luminary_amd.core import Core
    fam, sol, ids, hits = _prepared(name)
    core = Core(0)
    try:
        core.set_bvh_builder(builder)
        core.upload(fam.view)
        core.set_flavour("exact")
        e_ids, e_hits = core.light_query_host(fam.o, fam.d, fam.self_handles, fam.randoms)
        core.set_flavour("fast")
        f_ids, f_hits = core.light_query_host(fam.o, fam.d, fam.self_handles, fam.randoms)
    finally:
        core.close()
    where = "%s, %s" % (name, builder)
    same = (e_ids == ids) & (e_hits == hits)
    ok_e, why_e = sol.check(e_ids, e_hits)
    ok_f, why_f = sol.check(f_ids, f_hits)
    want_ids, want_hits = sol.expected()
    dec = sol.decisive
    right_e = (e_ids == want_ids) & (e_hits == want_hits)
    right_f = (f_ids == want_ids) & (f_hits == want_hits)
    print("%s: %d rays | exact: %d differ from the brute force, %d rejected, %d of %d decisive rays off the truth | fast: %d rejected, %d decisive rays off the truth" % (
        where, len(fam.o), int((~same).sum()), int((~ok_e).sum()), int((dec & ~right_e).sum()), int(dec.sum()), int((~ok_f).sum()), int((dec & ~right_f).sum())))
    assert same.all(), "%s: the exact flavour differs from the oracle's brute force on %d rays:\n%s" % (where, int((~same).sum()), _describe(fam, sol, e_ids, e_hits, ~same))
    assert ok_e.all(), "%s: exact flavour rejected:\n%s" % (where, _describe(fam, sol, e_ids, e_hits, ~ok_e, why_e))
    assert ok_f.all(), "%s: fast flavour rejected:\n%s" % (where, _describe(fam, sol, f_ids, f_hits, ~ok_f, why_f))
    assert (right_e | ~dec).all(), "%s: exact flavour off the truth on decisive rays:\n%s" % (where, _describe(fam, sol, e_ids, e_hits, dec & ~right_e))
    assert (right_f | ~dec).all(), "%s: fast flavour off the truth on decisive rays:\n%s" % (where, _describe(fam, sol, f_ids, f_hits, dec & ~right_f))
