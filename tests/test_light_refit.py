"""The light tree's refit, without a GPU: scene.cpp build_light_tree's LightRefitPlan and csrc/host/light_refit.{h,cpp} - the host twin that defines the bytes the
refit kernels (light_refit.hip; tests/test_light_refit_gpu.py) must produce.

The twin is held to a numpy restatement in float32, one operation at a time, byte for byte; to a float64 evaluation of the same statistics within a bound derived
from the operation count; its fragments to build_light_tree on the moved scene; its exponent function to ceil(log2(x)) in float64."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
from luminary_amd import Host, scenes
from luminary_amd.core import (LIGHT_REFIT_NOT_FINITE, LIGHT_REFIT_ZERO_AREA, LightRefitPlan, light_refit_ceil_log2, light_refit_host, light_root_children)
from test_instance_transforms_api import moved_instances
from test_mesh_positions_api import bend
from test_mesh_refit import soup

F, D, U = np.float32, np.float64, np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE = 64


# ---- scenes and what a refit needs of them ----
def lamp_scene(lights, seed=0, width=48, height=32, rotation=(0.3, -0.4, 0.2), scale=(1.0, 1.3, 0.8), second=True):
    """A floor, and `lights` emissive triangles as a soup in one mesh under a rotated, unevenly scaled instance (non-zero w lanes) - a third of them in a second,
    unrotated instance of another mesh when second."""
    rng = np.random.RandomState(1000 + lights + seed)
    host = Host()
    scenes.apply_benchmark_settings(host, width, height, 3, sky=(0.02, 0.02, 0.03))
    grey = host.add_material(scenes._material((0.6, 0.6, 0.6), 0.6))
    lamp = host.add_material(scenes._material((0.8, 0.8, 0.8), 0.5, emission=(6.0, 5.0, 4.0)))
    dim = host.add_material(scenes._material((0.8, 0.8, 0.8), 0.5, emission=(0.5, 2.0, 1.0)))
    floor = np.float32([[-14, -6, -14, 14, -6, -14, 14, -6, 14], [-14, -6, -14, 14, -6, 14, -14, -6, 14]])
    host.new_instance(host.add_mesh(floor, np.full(2, grey, dtype=np.uint16)))
    b = lights // 3 if (second and lights >= 3) else 0
    a = lights - b
    tris = soup(rng, a, spread=5.0).reshape(a, 9)
    host.new_instance(host.add_mesh(tris, np.where(np.arange(a) % 4 == 3, dim, lamp).astype(np.uint16)), position=(0.5, 1.0, -0.5), rotation=rotation, scale=scale)
    if b:
        host.new_instance(host.add_mesh(soup(rng, b, spread=4.0).reshape(b, 9) + F(0.25), np.full(b, lamp, dtype=np.uint16)), position=(-1.0, 0.5, 1.0))
    scenes.set_camera(host, (0.0, 2.0, 22.0), (0.0, 0.0, 0.0))
    return host


def light_arrays(view):
    """Copies of what a refit starts from and what it is compared with."""
    a = oracle_lib.view_arrays(view)
    root = np.asarray(a["light_tree_root"], dtype=np.uint8).copy()
    return {"root": root, "root_children": light_root_children(root), "nodes": np.asarray(a["light_tree_nodes"], dtype=np.uint8).reshape(-1, 64).copy(),
            "handles": np.asarray(a["light_tri_handles"], dtype=U).reshape(-1, 2).copy(), "tris": np.asarray(a["light_bvh_tris"]).view(F).reshape(-1, 12).copy(),
            "vertices": np.asarray(a["vertices"]).view(F).reshape(-1, 4).copy(), "mesh_tri_offset": np.asarray(a["mesh_tri_offset"], dtype=U).copy()}


class Built:
    """A host's light tree as built: the arrays, and a plan that owns its storage (the host's goes with its next build)."""

    def __init__(self, host):
        self.arrays = light_arrays(host.device_scene())
        self.plan = host.light_refit_plan().copy()

    def refit(self, vertices, plan=None):
        a = self.arrays
        return light_refit_host(plan or self.plan, vertices, a["mesh_tri_offset"], a["root"], a["root_children"], a["nodes"])


def transforms_of(host, plan):
    """The plan's transform table as build_light_tree forms it, from the host's instances as they now stand."""
    out = np.zeros((plan.num_transforms, 10), F)
    for k, i in enumerate(plan.arrays()[2]):
        inst = host.get_instance(int(i))
        q = _quaternion(inst.rotation)
        out[k, :4] = [-q[0], -q[1], -q[2], q[3]]
        out[k, 4:7] = [inst.scale.x, inst.scale.y, inst.scale.z]
        out[k, 7:] = [inst.position.x, inst.position.y, inst.position.z]
    return out


def _quaternion(r):
    import luminary_amd
    fn = luminary_amd._lib().luminary_ext_euler_to_quaternion
    fn.restype = C.c_uint64
    rot, q = (C.c_float * 3)(r.x, r.y, r.z), (C.c_float * 4)()
    assert fn(rot, q) == 0
    return np.float32(list(q))


def moved_emitters(host, phase=0.0, amount=0.2):
    """Every mesh with an emissive triangle, bent: the host holds the moved vertices afterwards. Returns the meshes."""
    out = []
    for m in range(host.get_num_meshes()):
        p, _, _, mats = host.get_mesh(m)
        if any(host.get_material(int(i)).emission_active for i in set(mats)):
            host.set_mesh_positions(m, bend(p, amount, phase))
            out.append(m)
    assert out
    return out


# ---- the numpy restatement: float32, one operation at a time ----
def fma32(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64, the sum is rounded to odd there, and the cast to float32 rounds once."""
    s, c = a.astype(D) * b.astype(D), c.astype(D)
    t = s + c
    bb = t - s
    err = (s - (t - bb)) + (c - bb)
    ti = np.atleast_1d(t).view(np.int64).copy()
    fix = (np.atleast_1d(err) != 0) & ((ti & 1) == 0)
    ti[fix] += np.where((np.atleast_1d(err) > 0) == (np.atleast_1d(t) > 0), 1, -1)[fix]
    return ti.view(D).reshape(np.shape(t)).astype(F)


def np_world(p, t):
    """lrf_world over points p [n, 3] with transform rows t [n, 10]: (xyz [n, 3], w [n])."""
    q, scale, offset = t[:, :4], t[:, 4:7], t[:, 7:]
    two = F(2.0)
    dqa = (p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]) + p[:, 2] * q[:, 2]
    dqq = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
    cr = np.stack([q[:, 1] * p[:, 2] - q[:, 2] * p[:, 1], q[:, 2] * p[:, 0] - q[:, 0] * p[:, 2], q[:, 0] * p[:, 1] - q[:, 1] * p[:, 0]], axis=1)
    s = q[:, 3] * q[:, 3] - dqq
    out = np.zeros_like(p)
    for k in range(3):
        v = q[:, k] * (two * dqa)
        v = v + p[:, k] * s
        v = v + cr[:, k] * (two * q[:, 3])
        out[:, k] = v * scale[:, k] + offset[:, k]
    w = q[:, 3] * (two * dqa)
    w = w + F(0.0) * s
    w = w + F(0.0) * (two * q[:, 3])
    return out, w * F(1.0) + F(0.0)


def np_fragments(fragments, transforms, vertices, mesh_tri_offset):
    """Records [n, 5, 4] float32 and flags, as lrf_fragment."""
    f = fragments
    t = transforms[f[:, 4]]
    first = 3 * (mesh_tri_offset[f[:, 1]].astype(np.int64) + f[:, 2])
    rec = np.zeros((len(f), 5, 4), F)
    with np.errstate(all="ignore"):
        for k in range(3):
            rec[:, k, :3], rec[:, k, 3] = np_world(vertices[first + k, :3], t)
        a, b, c = rec[:, 0], rec[:, 1], rec[:, 2]
        u, v = b[:, :3] - a[:, :3], c[:, :3] - a[:, :3]
        cr = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
        area = F(0.5) * np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 2] * cr[:, 2]) + (cr[:, 1] * cr[:, 1] + F(0.0)))
        rec[:, 3] = (a + (b + c)) * (F(1.0) / F(3.0))
        rec[:, 4, 0] = f[:, 5].view(F) * area * f[:, 6].view(F)
    flags = 0
    if not (np.isfinite(rec[:, :4]).all() and np.isfinite(rec[:, 4, 0]).all() and np.isfinite(vertices[(first[:, None] + np.arange(3)).reshape(-1), :3]).all()):
        flags |= LIGHT_REFIT_NOT_FINITE
    if (area == 0).any() or (rec[:, 4, 0] == 0).any():
        flags |= LIGHT_REFIT_ZERO_AREA
    return rec, flags


def butterfly(p):
    """[64, ...] partials through the xor butterfly 32, 16, 8, 4, 2, 1; lane 0's value."""
    lanes = np.arange(WAVE)
    for k in (32, 16, 8, 4, 2, 1):
        p = p + p[lanes ^ k]
    return p[0]


def np_slot(rec, first, count):
    """(power, variance, mean [4]) of one slot in the wave-shaped order."""
    if count == 0:
        return F(0), F(0), np.zeros(4, F)
    rows = (count + WAVE - 1) // WAVE
    items = np.zeros((rows * WAVE, 5, 4), F)
    items[:count] = rec[first:first + count]
    items = items.reshape(rows, WAVE, 5, 4)
    valid = (np.arange(rows * WAVE) < count).reshape(rows, WAVE)
    acc = np.zeros(WAVE, F)
    for r in range(rows):
        acc = np.where(valid[r], acc + items[r, :, 4, 0], acc)
    power = butterfly(acc)
    inv_total = F(1.0) / power
    m = np.zeros((WAVE, 4), F)
    for r in range(rows):
        w = items[r, :, 4, 0] * inv_total
        m = np.where(valid[r][:, None], fma32(items[r, :, 3], np.broadcast_to(w[:, None], (WAVE, 4)), m), m)
    mean = butterfly(m)
    var = np.zeros(WAVE, F)
    third = F(1.0) / F(3.0)
    for r in range(rows):
        w = third * items[r, :, 4, 0] * inv_total
        for k in range(3):
            d = items[r, :, k] - mean
            var = np.where(valid[r], var + w * ((d[:, 0] * d[:, 0] + d[:, 2] * d[:, 2]) + (d[:, 1] * d[:, 1] + d[:, 3] * d[:, 3])), var)
    return power, butterfly(var), mean


def ceil_log2(x):
    """Exact, in float64 (a float32's log2 is exact there only at powers of two, where frexp decides)."""
    m, e = np.frexp(np.float64(x))
    return int(e - 1) if m == 0.5 else int(e)


def np_exponent_for(rng):
    x = F(rng) * F(1.0) / F(255.0)
    if not x > 0:
        return -126
    if not np.isfinite(x):
        return 126
    return int(np.clip(ceil_log2(x), -126, 126))


def pack_float(v, mode):
    b = int(np.float32(v).view(U))
    if (mode == 1 and v >= 0) or (mode == 0 and v < 0):
        b = (b + 0xFFFF) & 0xFFFFFFFF
    return b >> 16


def np_quantiser(stats):
    used = [s for s in stats if s[0] > 0]
    mn, mx = np.full(3, F(1e10)), np.full(3, F(-1e10))
    max_var = max_power = F(0)
    for power, var, mean in used:
        for a in range(3):
            mn[a] = mean[a] if mean[a] < mn[a] else mn[a]
            mx[a] = mean[a] if mx[a] < mean[a] else mx[a]
        max_var = var if max_var < var else max_var
        max_power = power if max_power < power else max_power
    sd = np.sqrt(F(max_var))
    base = [pack_float(mn[a], 0) for a in range(3)]
    lo = np.array([b << 16 for b in base], dtype=U).view(F)
    e = [np_exponent_for(mx[a] - lo[a]) if mx[a] != lo[a] else 0 for a in range(3)] + [np_exponent_for(sd) if sd > 0 else 0]
    c = [np.ldexp(F(1.0), -k).astype(F) for k in e]
    return base, lo, e, c, F(max_power)


def np_child(q, stat, scale):
    base, lo, e, c, max_power = q
    power, var, mean = stat
    m = [int(np.floor((mean[a] - lo[a]) * c[a] + F(0.5))) & 0xFF for a in range(3)]
    sd = max(int(np.sqrt(F(var)) * c[3] + F(0.5)), 1) & 0xFF
    pw = max(int(np.floor(F(scale) * power / max_power + F(0.5))), 1)
    return m, sd, pw


def np_refit(plan, vertices, mesh_tri_offset, root, root_children, nodes):
    """The whole twin again: returns None for a fallback, else (root, root_children, nodes, tris, stats)."""
    fragments, transforms, _, slots = plan.arrays()
    rec, flags = np_fragments(fragments, transforms, vertices, mesh_tri_offset)
    if flags:
        return None
    root, root_children, nodes = root.copy(), root_children.copy(), nodes.copy()
    tris = np.zeros((len(fragments), 12), F)
    tris[fragments[:, 3]] = rec[:, :3].reshape(-1, 12)
    stats = [np_slot(rec, int(f), int(c)) for f, c in slots]
    sections = int(root[10])
    q = np_quantiser(stats[:128])
    base, lo, e, c, max_power = q
    root[0:6] = np.array(base, dtype=np.uint16).view(np.uint8)
    root[8:10] = np.array([pack_float(max_power, 1)], dtype=np.uint16).view(np.uint8)
    root[12:16] = np.array(e, dtype=np.int8).view(np.uint8)
    for ch in range(8 * sections):
        m, sd, pw = ([0, 0, 0], 0, 0)
        if stats[ch][0] > 0:
            m, sd, pw = np_child(q, stats[ch], 0xFFFF)
            sec = root[16 + 48 * (ch // 8):]
            k = ch % 8
            sec[k], sec[8 + k], sec[16 + k], sec[24 + k] = m[0], m[1], m[2], sd
            sec[32 + 2 * k], sec[33 + 2 * k] = pw & 0xFF, (pw >> 8) & 0xFF
        for a in range(3):
            root_children[8 * ch + a] = F(m[a]) * np.ldexp(F(1.0), e[a]).astype(F) + lo[a]
        root_children[8 * ch + 3] = F(sd) * np.ldexp(F(1.0), e[3]).astype(F)
        root_children[8 * ch + 4] = F(pw & 0xFFFF)
    for j in range(len(nodes)):
        st = stats[128 + 8 * j:136 + 8 * j]
        q = np_quantiser(st)
        nodes[j, 0:6] = np.array(q[0], dtype=np.uint16).view(np.uint8)
        nodes[j, 8:12] = np.array(q[2], dtype=np.int8).view(np.uint8)
        for ch in range(8):
            if st[ch][0] > 0:
                m, sd, pw = np_child(q, st[ch], 0xFF)
                nodes[j, 24 + ch], nodes[j, 32 + ch], nodes[j, 40 + ch], nodes[j, 48 + ch], nodes[j, 56 + ch] = m[0], m[1], m[2], sd, pw & 0xFF
    return root, root_children, nodes, tris, stats


def assert_twin_is_numpy(built, vertices, where, plan=None):
    plan = plan or built.plan
    a = built.arrays
    out = light_refit_host(plan, vertices, a["mesh_tri_offset"], a["root"], a["root_children"], a["nodes"])
    want = np_refit(plan, vertices, a["mesh_tri_offset"], a["root"], a["root_children"], a["nodes"])
    assert want is not None and out["report"].refitted == 1 and out["report"].flags == 0, where
    root, table, nodes, tris, stats = want
    got_stats = out["slot_stats"]
    for s, (power, var, mean) in enumerate(stats):
        ref = np.concatenate([[power, var], mean, [0, 0]]).astype(F)
        assert np.array_equal(got_stats[s].view(U), ref.view(U)), "%s: slot %d statistics %s, numpy %s" % (where, s, got_stats[s], ref)
    assert np.array_equal(out["light_bvh_tris"].view(U), tris.view(U)), where + ": light_bvh_tris"
    assert np.array_equal(out["root"], root), "%s: %d root bytes differ" % (where, int((out["root"] != root).sum()))
    assert np.array_equal(out["root_children"].view(U), table.view(U)), where + ": the root's float table"
    assert np.array_equal(out["nodes"], nodes), "%s: %d node bytes differ" % (where, int((out["nodes"] != nodes).sum()))
    return out, stats


# ---- the exact exponent ----
def test_the_exponent_is_ceil_log2_at_every_power_of_two_their_neighbours_and_a_million_floats():
    bits = []
    for e in range(-149, 128):
        b = int(np.float32(np.ldexp(1.0, e)).view(U))
        bits += [b + k for k in range(-4, 5) if 0 < b + k < 0x7F800000]
    rng = np.random.RandomState(3)
    bits = np.concatenate([np.array(bits, dtype=U), rng.randint(1, 0x7F800000, size=1_000_000).astype(U)])
    x = bits.view(F)
    import luminary_amd
    fn = luminary_amd._lib().lumc_light_refit_ceil_log2
    fn.restype, fn.argtypes = C.c_int, [C.c_float]
    m, e = np.frexp(x.astype(D))
    want = np.where(m == 0.5, e - 1, e)
    got = np.array([fn(float(v)) for v in x[:3000]] + [fn(float(v)) for v in x[3000:]], dtype=np.int64)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "x = %r: %d, ceil(log2) = %d" % (x[bad[0]], got[bad[0]], want[bad[0]])
    assert light_refit_ceil_log2(1.0) == 0 and light_refit_ceil_log2(np.nextafter(F(1), F(2))) == 1 and light_refit_ceil_log2(255.0) == 8


# ---- the plan ----
@pytest.mark.parametrize("lights", [2, 8, 9, 128, 129, 1000])
def test_the_plan_names_every_light_once_and_every_slot_a_range_of_the_tree(lights):
    host = lamp_scene(lights)
    try:
        built = Built(host)
        fragments, transforms, instances, slots = built.plan.arrays()
        a = built.arrays
        assert built.plan.num_fragments == lights == len(a["handles"]) and built.plan.num_nodes == len(a["nodes"])
        assert sorted(fragments[:, 3]) == list(range(lights)), "the light ids are a permutation"
        assert np.array_equal(a["handles"][fragments[:, 3]], fragments[:, [0, 2]]), "a fragment's light id is its handle's place"
        sections = int(a["root"][10])
        used = slots[:128, 1] > 0
        assert used[:used.sum()].all() and (sections - 1) * 8 < used.sum() <= sections * 8, "the root's used slots come first and fill its sections"
        assert int(slots[:128, 1].sum()) == lights, "the root's children partition the lights"
        assert int((slots[:128, 1] == 1).sum()) == int(a["root"][6:8].view(np.uint16)[0]), "the root's leaves are its one-light slots"
        for j, node in enumerate(a["nodes"]):
            s = slots[128 + 8 * j:136 + 8 * j]
            assert int((s[:, 1] == 1).sum()) == node[12], "node %d: byte 12 counts its leaves" % j
            assert ((s[:, 1] > 0) == (node[56:64] > 0)).all(), "node %d: a used slot has a quantised power" % j
        assert len(transforms) == len(set(fragments[:, 0])) and np.array_equal(transforms, transforms_of(host, built.plan)), "one full-precision transform per emitting instance"
        stats = built.refit(a["vertices"])["slot_stats"]
        cost = float((stats[:128, 0].astype(D) * stats[:128, 1].astype(D)).sum())
        assert abs(cost / built.plan.root_cost - 1.0) < 1e-4, "root_cost is the build's sum of power * variance"
    finally:
        host.close()


# ---- the twin against numpy, byte for byte ----
@pytest.mark.parametrize("lights", [2, 8, 9, 128, 129, 1000])
def test_the_twin_is_the_numpy_restatement_on_moved_trees_of_every_shape(lights):
    host = lamp_scene(lights)
    try:
        built = Built(host)
        assert_twin_is_numpy(built, built.arrays["vertices"], "%d lights, unmoved" % lights)
        moved_emitters(host, 0.3)
        moved = light_arrays(host.device_scene())
        out, _ = assert_twin_is_numpy(built, moved["vertices"], "%d lights, moved" % lights)
        assert not np.array_equal(out["root"], built.arrays["root"]), "the move changes the root"
        w = out["light_bvh_tris"][:, [3, 7, 11]]
        assert (w != 0).any(), "a rotated instance leaves non-zero w lanes"
    finally:
        host.close()


def synthetic(counts, seed=5, minus_zero=False):
    """A plan whose root children summarise ranges of the given sizes over a soup of one mesh under one rotated instance; (plan, vertices, offsets, root, table)."""
    rng = np.random.RandomState(seed)
    n = int(sum(counts))
    tris = soup(rng, n, spread=8.0).reshape(n, 3, 3)
    if minus_zero:
        tris[::5, 0, 0] = F(-0.0)
        tris[1::7, 2, 1] = F(-0.0)
    vertices = np.zeros((3 * n, 4), F)
    vertices[:, :3] = tris.reshape(-1, 3)
    fragments = np.zeros((n, 8), U)
    fragments[:, 2] = rng.permutation(n)
    fragments[:, 3] = rng.permutation(n)
    fragments[:, 5] = rng.uniform(0.5, 8.0, n).astype(F).view(U)
    fragments[:, 6] = rng.uniform(0.25, 1.0, n).astype(F).view(U)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    transforms = np.float32([list(q) + [1.0, 0.7, 1.6] + [0.5, -2.0, 3.0]])
    sections = (len(counts) + 7) // 8
    slots = np.zeros((128, 2), U)
    slots[:len(counts), 1] = counts
    slots[:len(counts), 0] = np.concatenate([[0], np.cumsum(counts)[:-1]])
    root = np.zeros(16 + 48 * sections, np.uint8)
    root[10] = sections
    plan = LightRefitPlan.from_arrays(fragments, transforms, [0], slots, 1.0)
    return plan, vertices, np.array([0, n], dtype=U), root, np.zeros(sections * 64 + 16, F)


RANGES = [1, 2, 63, 64, 65, 127, 128, 129, 4097]


@pytest.mark.parametrize("minus_zero", [False, True])
def test_the_twin_is_the_numpy_restatement_on_ranges_around_a_wave(minus_zero):
    plan, vertices, offsets, root, table = synthetic(RANGES, minus_zero=minus_zero)
    nodes = np.zeros((0, 64), np.uint8)
    out = light_refit_host(plan, vertices, offsets, root, table, nodes)
    want = np_refit(plan, vertices, offsets, root, table, nodes)
    assert out["report"].refitted == 1 and want is not None
    for s, (power, var, mean) in enumerate(want[4][:len(RANGES)]):
        ref = np.concatenate([[power, var], mean, [0, 0]]).astype(F)
        assert np.array_equal(out["slot_stats"][s].view(U), ref.view(U)), "range of %d: %s, numpy %s" % (RANGES[s], out["slot_stats"][s], ref)
    assert np.array_equal(out["root"], want[0]) and np.array_equal(out["root_children"].view(U), want[1].view(U)) and np.array_equal(out["light_bvh_tris"].view(U), want[3].view(U))
    assert (out["slot_stats"][len(RANGES):128] == 0).all() and (out["root"][16 + 48 + 1:16 + 48 + 8] == 0).all(), "unused slots stay zero"
    if minus_zero:
        assert (vertices.view(U) == 0x80000000).any()


def test_the_twin_is_the_numpy_restatement_on_a_textured_emitter():
    host = scenes.emissive_texture_scene()
    try:
        built = Built(host)
        fragments = built.plan.arrays()[0]
        assert len(set(fragments[:, 6])) > 1, "texture-integrated intensities differ between triangles"
        assert_twin_is_numpy(built, built.arrays["vertices"], "textured, unmoved")
        moved_emitters(host, 0.2, 0.1)
        moved = light_arrays(host.device_scene())
        assert len(moved["handles"]) == len(built.arrays["handles"]), "the bend keeps the set of lights"
        assert_twin_is_numpy(built, moved["vertices"], "textured, moved")
    finally:
        host.close()


# ---- the statistics against float64, before quantisation ----
def test_the_statistics_are_the_float64_ones_within_the_rounding_of_the_longest_lane_chain():
    """Per slot of k = ceil(count / 64) items per lane. u = 2^-24. Every fragment's power is positive, so the power - k + 6 additions (lane chain, then six
    butterfly steps) - has a relative error of at most (k + 6) u (1 + small). A weight power_i * inv_total carries the power's error, the reciprocal's and the
    product's: (k + 8) u; a mean lane adds k fma roundings and six additions over terms of magnitude <= R (the largest |coordinate| of the slot):
    |mean32 - mean64| <= E = (2 k + 16) u R. A variance term w * dot4(d) has w's (k + 9) u, and for every lane of d one subtraction, one square and at most three
    additions: 6 u relative to |d|^2, plus the shift of d by the mean's error, 2 |d| E + E^2 per lane with |d| <= 2 R; summing 3 k + 6 times adds (3 k + 6) u. With
    weights summing to 1: |var32 - var64| <= (4 k + 24) u var64 + 4 (4 R E + E^2). Both sides are computed from the float32 records the twin reports (the fragment
    arithmetic itself is held to build_light_tree byte for byte below)."""
    u = 2.0 ** -24
    plan, vertices, offsets, root, table = synthetic(RANGES, seed=9)
    out = light_refit_host(plan, vertices, offsets, root, table, np.zeros((0, 64), np.uint8))
    fragments, transforms, _, slots = plan.arrays()
    rec, flags = np_fragments(fragments, transforms, vertices, offsets)
    assert flags == 0
    for s, count in enumerate(RANGES):
        first = int(slots[s, 0])
        r = rec[first:first + count].astype(D)
        k = (count + WAVE - 1) // WAVE
        power = r[:, 4, 0].sum()
        w = r[:, 4, 0] / power
        mean = (r[:, 3] * w[:, None]).sum(axis=0)
        var = (w[:, None] / 3.0 * ((r[:, :3] - mean) ** 2).sum(axis=2)).sum()
        got = out["slot_stats"][s].astype(D)
        R = float(np.abs(r[:, :4]).max())
        E = (2 * k + 16) * u * R
        print("range %5d: power %.3e of %.3e, mean %.3e of %.3e, variance %.3e of %.3e" % (count, abs(got[0] - power), (k + 6) * u * 1.01 * power, np.abs(got[2:6] - mean).max(), E,
                                                                                      abs(got[1] - var), (4 * k + 24) * u * var + 4 * (4 * R * E + E * E)))
        assert abs(got[0] - power) <= (k + 6) * u * 1.01 * power
        assert np.abs(got[2:6] - mean).max() <= E
        assert abs(got[1] - var) <= (4 * k + 24) * u * var + 4 * (4 * R * E + E * E)


# ---- fragments against the build ----
def by_handle(arrays):
    return {(int(i), int(t)): arrays["tris"][k].view(U).tobytes() for k, (i, t) in enumerate(arrays["handles"])}


@pytest.mark.parametrize("scene", ["zoo", "lamps", "instances"])
def test_the_twins_fragments_are_those_of_a_build_of_the_moved_scene(scene):
    host = scenes.zoo_scene(48, 32, 3) if scene == "zoo" else lamp_scene(129)
    try:
        built = Built(host)
        plan = built.plan
        if scene == "instances":
            host.set_instance_transforms(moved_instances(host, 1, every=1))
            f, _, ti, sl = built.plan.arrays()
            plan = LightRefitPlan.from_arrays(f, transforms_of(host, built.plan), ti, sl, built.plan.root_cost)
        else:
            moved_emitters(host, 0.7)
        moved = light_arrays(host.device_scene())
        out = built.refit(moved["vertices"], plan)
        assert out["report"].refitted == 1
        assert len(moved["handles"]) == len(built.arrays["handles"]), "the move keeps the set of lights"
        want = by_handle(moved)
        got = by_handle({"tris": out["light_bvh_tris"], "handles": built.arrays["handles"]})
        assert got.keys() == want.keys(), "the handles are unchanged"
        assert got == want, "%d of %d lights' world-space triangles differ from the build's" % (sum(got[h] != want[h] for h in got), len(got))
        assert got != by_handle(built.arrays), "the move moved them"
    finally:
        host.close()


# ---- structure ----
def test_a_refit_keeps_counts_and_pointers_and_every_quantised_power_is_at_least_one():
    host = scenes.zoo_scene(48, 32, 3)
    try:
        built = Built(host)
        moved_emitters(host, 1.1, 0.3)
        out = built.refit(light_arrays(host.device_scene())["vertices"])
        a, nodes, root = built.arrays, out["nodes"], out["root"]
        assert np.array_equal(nodes[:, 12], a["nodes"][:, 12]) and np.array_equal(nodes[:, 16:24], a["nodes"][:, 16:24]), "byte 12 and bytes 16-23 of every node"
        assert np.array_equal(nodes[:, 6:8], a["nodes"][:, 6:8]) and np.array_equal(nodes[:, 13:16], a["nodes"][:, 13:16])
        assert np.array_equal(root[6:8], a["root"][6:8]) and np.array_equal(root[10:12], a["root"][10:12])
        slots = built.plan.arrays()[3]
        used = slots[128:, 1].reshape(-1, 8) > 0
        assert (nodes[:, 56:64][used] >= 1).all() and (nodes[:, 48:56][used] >= 1).all() and (nodes[:, 56:64][~used] == 0).all()
        for c in np.nonzero(slots[:128, 1])[0]:
            sec = root[16 + 48 * (c // 8):]
            assert int(sec[32 + 2 * (c % 8):34 + 2 * (c % 8)].view(np.uint16)[0]) >= 1 and sec[24 + c % 8] >= 1
        assert np.array_equal(out["root_children"].view(U), light_root_children(root).view(U)), "the float table is the one an upload makes of the refitted root"
    finally:
        host.close()


def test_an_unmoved_refit_reproduces_the_build_up_to_the_last_bits_of_the_powers():
    host = scenes.zoo_scene(48, 32, 3)
    try:
        built = Built(host)
        out = built.refit(built.arrays["vertices"])
        a = built.arrays
        assert np.array_equal(out["light_bvh_tris"].view(U), a["tris"].view(U)), "the fragments are the build's bits"
        assert abs(out["report"].cost_growth - 1.0) < 1e-4
        # the quantised statistics may differ by one step where a binned power's last bits decided a rounding
        assert int(np.abs(out["nodes"].astype(int) - a["nodes"].astype(int)).max()) <= 1 and int(np.abs(out["root"][16:].astype(int) - a["root"][16:].astype(int)).max()) <= 1
    finally:
        host.close()


# ---- sampling stays unbiased: the analytic identity of tests/test_oracle_analytic.py on the refitted tree ----
def _sum_of_weights(view, pos, nrm, n=40_000):
    """E[sum over the 8 lanes of weight * 1] and the lights that were chosen (tests/test_oracle_analytic.py test_light_tree_resampling_weights_are_unbiased)."""
    from test_oracle_analytic import ProbeMaterial, _f3
    ids, w = np.zeros((n, 8), dtype=U), np.zeros((n, 8), dtype=F)
    m = ProbeMaterial((0.8, 0.8, 0.8), 1.0, 0.7, 1.0, 0)
    oracle_lib.lib().oracle_probe_light_tree(C.byref(view), C.byref(m), _f3(pos), _f3(nrm), _f3((0.3, 0.9, 0.1)), 4, 9, 0, n, ids.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p),
                                             C.c_void_p(0))
    valid = ids != 0xFFFFFFFF
    assert valid.any()
    return float((w * valid).sum(axis=1).mean()), np.unique(ids[valid]), ids, w


def with_light_arrays(view, root, nodes, handles, tris):
    """A copy of the view whose light arrays are the given ones (kept alive by the copy)."""
    v = oracle_lib.with_luts(view)
    keep = (np.ascontiguousarray(root, dtype=np.uint8), np.ascontiguousarray(nodes, dtype=np.uint8), np.ascontiguousarray(handles, dtype=U), np.ascontiguousarray(tris, dtype=F))
    v.light_tree_root, v.light_tree_nodes, v.light_tri_handles, v.light_bvh_tris = (k.ctypes.data for k in keep)
    v.num_light_tree_nodes, v.num_lights = keep[1].size // 64, len(keep[2].reshape(-1, 2))
    v._lights = keep
    return v


def test_the_refitted_tree_is_sampled_without_bias_on_the_moved_zoo():
    host = scenes.zoo_scene(48, 32, 3)
    try:
        built = Built(host)
        moved_emitters(host, 0.5, 0.25)
        view = host.device_scene()
        out = built.refit(light_arrays(view)["vertices"])
        refitted = with_light_arrays(view, out["root"], out["nodes"], built.arrays["handles"], out["light_bvh_tris"])
        for pos, nrm in (((0.0, 0.5, 0.0), (0.0, 1.0, 0.0)), ((3.0, 1.0, -2.0), (0.0, 1.0, 0.0))):
            total, chosen, ids, w = _sum_of_weights(refitted, pos, nrm)
            print("at %s: sum of weights %.3f, %d lights chosen" % (pos, total, len(chosen)))
            assert abs(total - len(chosen)) < 0.05 * len(chosen), (total, len(chosen))
            freq = np.array([(ids == l).mean() for l in chosen])
            for l in chosen[np.argsort(-freq)[:4]]:
                est = float((w * (ids == l)).sum(axis=1).mean())
                assert abs(est - 1.0) < 0.05, (int(l), est)
    finally:
        host.close()


# ---- fallbacks ----
@pytest.mark.parametrize("what", ["zero area", "nan", "inf"])
def test_a_fragment_that_leaves_the_set_of_lights_reports_a_fallback_and_writes_nothing(what):
    host = lamp_scene(129)
    try:
        built = Built(host)
        a = built.arrays
        vertices = a["vertices"].copy()
        f = built.plan.arrays()[0][17]
        first = 3 * (int(a["mesh_tri_offset"][f[1]]) + int(f[2]))
        if what == "zero area":
            vertices[first + 1, :3] = vertices[first, :3]
            vertices[first + 2, :3] = vertices[first, :3]
        else:
            vertices[first + 2, 1] = np.nan if what == "nan" else np.inf
        out = built.refit(vertices)
        assert out["report"].refitted == 0 and out["report"].flags & (LIGHT_REFIT_ZERO_AREA if what == "zero area" else LIGHT_REFIT_NOT_FINITE)
        assert np.array_equal(out["root"], a["root"]) and np.array_equal(out["nodes"], a["nodes"]) and np.array_equal(out["root_children"].view(U), a["root_children"].view(U))
        assert (out["light_bvh_tris"] == 0).all() and (out["slot_stats"] == 0).all(), "nothing is written"
        assert np_refit(built.plan, vertices, a["mesh_tri_offset"], a["root"], a["root_children"], a["nodes"]) is None
    finally:
        host.close()


def test_the_one_light_tree_is_left_alone():
    host = lamp_scene(1)
    try:
        built = Built(host)
        assert built.plan.num_fragments == 1
        out = built.refit(built.arrays["vertices"] + F(1.0))
        assert out["report"].refitted == 0 and out["report"].flags == 0 and np.array_equal(out["root"], built.arrays["root"])
    finally:
        host.close()


# ---- the update plan: its old cases are unchanged (tests/test_update_plan.py runs them), the new bit has a check program of its own ----
def _compile_and_run(source, name, tmp_path, flags=()):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", *flags, "-D__HIP_PLATFORM_AMD__", "-DLUM_LRF_HOST_ONLY=1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "luminary_amd", "csrc", "host"),
           os.path.join(ROOT, "tests", "support", source), "-o", exe]
    if source == "light_refit_check.cpp":
        cmd.insert(-2, os.path.join(ROOT, "luminary_amd", "csrc", "host", "light_refit.cpp"))
        cmd += ["-ffp-contract=off"]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    return run.stdout


def test_the_update_plan_takes_the_new_bit_only_with_a_binding_and_without_new_lights(tmp_path):
    out = _compile_and_run("light_refit_plan_check.cpp", "light_refit_plan_check", tmp_path)
    assert "32768 cases" in out, out


def test_the_stats_and_plan_structs_have_the_layout_python_assumes(tmp_path):
    from luminary_amd.core import LightRefitReport, LightRefitStats
    out = _compile_and_run("light_refit_layout_probe.cpp", "light_refit_layout_probe", tmp_path)
    want = {}
    for line in out.split("\n"):
        if line.strip():
            name, rest = line.split(":")
            want[name] = [int(x) for x in rest.split()]
    for cls, name in ((LightRefitStats, "LumLightRefitStats"), (LightRefitReport, "LumLightRefitReport"), (LightRefitPlan, "LumLightRefitPlan")):
        got = [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
        assert got == want[name], "%s: python %s, compiled %s" % (name, got, want[name])
    assert want["LumLightFragment"] == [32] and want["LumLightTransform"] == [40] and want["LumLightSlot"] == [8]


# ---- sanitizers: a stand-alone program runs the twin, nothing loaded into Python ----
def test_the_twin_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    out = _compile_and_run("light_refit_check.cpp", "light_refit_check", tmp_path, flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))
    assert "light_refit_check: ok" in out, out


# ---- the host API's switch, as far as it shows without a device ----
def test_with_the_switch_on_the_hosts_view_follows_a_move_through_the_twin_and_off_it_is_todays_build():
    on, off, toggled = scenes.zoo_scene(48, 32, 3), scenes.zoo_scene(48, 32, 3), scenes.zoo_scene(48, 32, 3)
    try:
        on.set_light_refit(1)
        toggled.set_light_refit(1, 2.0)
        toggled.set_light_refit(0)
        built = Built(on)
        for host in (on, off, toggled):
            moved_emitters(host, 0.45)
            host.set_instance_transforms(moved_instances(host, 2, every=1))
        got, want, again = light_arrays(on.device_scene()), light_arrays(off.device_scene()), light_arrays(toggled.device_scene())
        for k in want:
            assert np.array_equal(want[k].view(np.uint8), again[k].view(np.uint8)), "switched off again, %s is what a host that never had the switch builds" % k
        assert np.array_equal(got["vertices"].view(U), want["vertices"].view(U))
        f, _, ti, sl = built.plan.arrays()
        plan = LightRefitPlan.from_arrays(f, transforms_of(on, built.plan), ti, sl, built.plan.root_cost)
        twin = built.refit(got["vertices"], plan)
        assert twin["report"].refitted == 1
        assert np.array_equal(got["handles"], built.arrays["handles"]), "the topology of the last build is kept"
        assert np.array_equal(got["root"], twin["root"]) and np.array_equal(got["nodes"], twin["nodes"]) and np.array_equal(got["tris"].view(U), twin["light_bvh_tris"].view(U))
        assert not np.array_equal(got["root"], built.arrays["root"])
        # a collapsed triangle changes the set of lights: the view is built again, as without the switch
        for host in (on, off):
            p = host.get_mesh(_first_emitter(host))[0].copy()
            p[2, 3:6] = p[2, 0:3]
            p[2, 6:9] = p[2, 0:3]
            host.set_mesh_positions(_first_emitter(host), p)
        got, want = light_arrays(on.device_scene()), light_arrays(off.device_scene())
        assert len(got["handles"]) == len(built.arrays["handles"]) - 1
        for k in want:
            assert np.array_equal(want[k].view(np.uint8), got[k].view(np.uint8)), k
    finally:
        on.close(); off.close(); toggled.close()


def _first_emitter(host):
    for m in range(host.get_num_meshes()):
        if any(host.get_material(int(i)).emission_active for i in set(host.get_mesh(m)[3])):
            return m
    raise AssertionError("no emissive mesh")
