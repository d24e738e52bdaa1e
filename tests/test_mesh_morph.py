"""Morph targets on the host side (include/lum_core.h lumc_morph_host; include/luminary_amd.h luminary_ext_bind_mesh_morph / _set_mesh_weights; csrc/host/mesh_deform.h,
mesh_deform.cpp, api.cpp), no GPU.

morph(base, deltas, weights) is one function compiled twice; this file holds the host's compilation - the twin - to a numpy restatement of the definition, float32 one
operation at a time with the normal packed in float64, byte for byte, and to a float64 evaluation within the rounding bound; tests/test_mesh_morph_gpu.py holds the
device's to the twin. Then the host layer: what it refuses, the one rest shape a skin and a morph share, that the host mesh of a morphed mesh is the twin's output
whenever something reads it, and that the device scene it hands out is, byte for byte, that of a host which was given those vertices."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import luminary_amd
from luminary_amd import core
from luminary_amd.core import morph_host, skin_host
from test_mesh_positions_api import device_arrays
from test_mesh_skin import (INVALID_API_ARGUMENT, _meshes, _ptr, _raw, _same_bytes, _zoo, pack_normal64, random_bones, random_skin, two_bone_bend, two_bone_weights,
                            unit_normals)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SIZES = [1, 21, 22, 85, 86]  # triangles: 3, 63, 66 corners - either side of a wave -, 255, 258 - of a workgroup
TARGETS = [1, 3, 1024]


# ---- targets and weights shared with tests/test_mesh_morph_gpu.py ----
class Morph:
    """Sparse targets, target-major: offsets [T + 1] into corners [E], delta positions / normals [E, 3]; made from one entry per (target, corner) pair in any order."""

    def __init__(self, target_count, targets, corners, dp, dn):
        targets, corners = np.asarray(targets, np.int64).reshape(-1), np.asarray(corners, np.int64).reshape(-1)
        order = np.lexsort((corners, targets))
        pairs = targets[order] * (int(corners.max()) + 1 if len(corners) else 1) + corners[order]
        assert (np.diff(pairs) > 0).all(), "a corner is in a target at most once"
        self.target_count = target_count
        self.offsets = np.searchsorted(targets[order], np.arange(target_count + 1)).astype(np.uint32)
        self.corners = corners[order].astype(np.uint32)
        self.dp, self.dn = np.asarray(dp, F).reshape(-1, 3)[order], np.asarray(dn, F).reshape(-1, 3)[order]

    @property
    def lists(self):
        return self.offsets, self.corners, self.dp, self.dn


def random_morph(rng, triangles, target_count, per_corner=3.0):
    """Targets over 3 * triangles corners with the three row shapes: corner 0 has an entry in EVERY target, corner 1 in exactly one - the LAST target, which is thereby
    named -, corner 2 in none; every other corner is in per_corner targets on average, in none to a dozen. A share of the deltas is -0."""
    c = 3 * triangles
    count = int(per_corner * max(c - 3, 0))
    pairs = np.unique(rng.randint(0, target_count, count).astype(np.int64) * c + rng.randint(3, max(c, 4), count))
    pairs = np.concatenate([pairs, np.arange(target_count, dtype=np.int64) * c, [np.int64(target_count - 1) * c + 1]])
    dp, dn = rng.uniform(-0.5, 0.5, (len(pairs), 3)).astype(F), rng.uniform(-0.4, 0.4, (len(pairs), 3)).astype(F)
    dp[rng.uniform(size=dp.shape) < 0.1] = F(-0.0)
    dn[rng.uniform(size=dn.shape) < 0.1] = F(-0.0)
    return Morph(target_count, pairs // c, pairs % c, dp, dn)


def random_weights(rng, target_count):
    """Negative weights, weights above 1, exact zeros of either sign; the last target's weight is never zero."""
    w = rng.uniform(-0.75, 1.75, target_count).astype(F)
    kind = rng.uniform(size=target_count)
    w[kind < 0.15] = F(0.0)
    w[(kind >= 0.15) & (kind < 0.3)] = F(-0.0)
    w[-1] = F(1.25)
    if target_count >= 3:
        w[0], w[1] = F(-0.5), F(-0.0)
    return w


def bulge_targets(positions, target_count=3, strength=0.15):
    """Targets over regions of a mesh [n, 9]: target t pushes the corners within a third of the mesh's size of its centre outwards, with a smooth fall-off, and
    tilts their normals the same way. Shared vertices stay shared."""
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    size = float(max((hi - lo).max(), 1e-6))
    middle = 0.5 * (lo + hi)
    targets, corners, dp, dn = [], [], [], []
    for t in range(target_count):
        u = (t + 0.5) / target_count
        centre = lo + (hi - lo) * np.array([u, 1.0 - u, 0.5 + 0.3 * np.sin(5.0 * u)])
        d = np.linalg.norm(p - centre, axis=1) / (0.45 * size)
        fall = np.where(d < 1.0, (1.0 - d * d) ** 2, 0.0)
        out = p - middle
        out /= np.maximum(np.linalg.norm(out, axis=1, keepdims=True), 1e-9)
        out += np.array([0.0, 0.3, 0.0])
        inside = np.nonzero(fall > 0.0)[0]
        targets.append(np.full(len(inside), t)); corners.append(inside)
        dp.append(strength * size * fall[inside, None] * out[inside]); dn.append(0.5 * fall[inside, None] * out[inside])
    return Morph(target_count, np.concatenate(targets), np.concatenate(corners), np.concatenate(dp), np.concatenate(dn))


# ---- the definition, restated ----
def morph_sums_numpy(base_positions, base_normals, morph, weights):
    """The un-normalised morphed positions and normals [c, 3] float32 and the contributing entries per corner: numpy rounds every float32 operation once; targets
    ascending, which is every corner's order."""
    p, n = np.array(base_positions, F).reshape(-1, 3), np.array(base_normals, F).reshape(-1, 3)
    used = np.zeros(len(p), np.int64)
    w = np.asarray(weights, F)
    with np.errstate(all="ignore"):
        for t in range(morph.target_count):
            if w[t] == 0:  # (-0 too)
                continue
            a, b = int(morph.offsets[t]), int(morph.offsets[t + 1])
            idx = morph.corners[a:b]
            for r in range(3):
                p[idx, r] = p[idx, r] + w[t] * morph.dp[a:b, r]
                n[idx, r] = n[idx, r] + w[t] * morph.dn[a:b, r]
            used[idx] += 1
    assert p.dtype == F and n.dtype == F
    return p, n, used


def morph_numpy(base_positions, base_normals, morph, weights):
    """morph() without a skin. Returns positions, normals [n, 9], packed [n, 3]."""
    base_n = np.asarray(base_normals, F).reshape(-1, 3)
    p, n, used = morph_sums_numpy(base_positions, base_normals, morph, weights)
    with np.errstate(all="ignore"):
        len2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        ok = (used > 0) & (len2 > 0) & np.isfinite(len2)
        rl = F(1.0) / np.sqrt(len2)
        out_n = np.where(ok[:, None], n * rl[:, None], base_n)
    assert out_n.dtype == F
    return p.reshape(-1, 9), out_n.reshape(-1, 9), pack_normal64(out_n).reshape(-1, 3)


def _cases():
    """name -> (base positions, base normals, morph, weights)"""
    out = {}
    for n in SIZES:
        for t in TARGETS:
            rng = np.random.RandomState(1000 * n + t)
            morph = random_morph(rng, n, t)
            assert int(morph.offsets[-1]) > int(morph.offsets[-2]), "the last target is named"
            out["%d triangles, %d targets" % (n, t)] = (rng.uniform(-3.0, 3.0, (n, 9)).astype(F), unit_normals(rng, n), morph, random_weights(rng, t))
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_twin_is_the_definition_byte_for_byte(name):
    base_p, base_n, morph, w = CASES[name]
    assert len(w) == 1 or ((w < 0).any() and (w > 1).any() and (w == 0).any() and np.signbit(w[w == 0]).any()), "negative, above 1, and -0 among the weights"
    got, want = morph_host(base_p, base_n, *morph.lists, w), morph_numpy(base_p, base_n, morph, w)
    _same_bytes(got, want, name)
    used = morph_sums_numpy(base_p, base_n, morph, w)[2]
    live = int((w != 0).sum())
    assert used[0] == live and used[1] == 1 and used[2] == 0, "the three row shapes: every target, one, none"
    # the corner without an entry keeps the base record's bytes; a corner something was added to has a unit normal
    assert got[0].reshape(-1, 3)[2].tobytes() == base_p.reshape(-1, 3)[2].tobytes() and got[1].reshape(-1, 3)[2].tobytes() == base_n.reshape(-1, 3)[2].tobytes()
    lengths = np.linalg.norm(got[1].reshape(-1, 3).astype(np.float64), axis=1)
    assert np.abs(lengths - 1.0).max() < 4e-7, name
    # without normal deltas: the same positions
    flat = morph_host(base_p, base_n, morph.offsets, morph.corners, morph.dp, None, w)
    assert flat[0].tobytes() == got[0].tobytes()


@pytest.mark.parametrize("name", sorted(CASES))
def test_all_weights_zero_give_the_base_records(name):
    base_p, base_n, morph, w = CASES[name]
    skewed = (base_n * F(1.7)).astype(F)  # not unit: nothing may normalise it
    for zero in (np.zeros_like(w), np.full_like(w, -0.0)):
        got = morph_host(base_p, skewed, *morph.lists, zero)
        _same_bytes(got, (base_p, skewed, pack_normal64(skewed.reshape(-1, 3)).reshape(-1, 3)), name)


def _one_corner(entries, base_p=(0.0, 0.0, 0.0), base_n=(0.0, 0.0, 1.0)):
    """A triangle whose corner 0 has the entries [(dp, dn)], one target each, in that order."""
    p, n = np.zeros((1, 9), F), np.tile(F(base_n), 3).reshape(1, 9)
    p[0, :3] = base_p
    return p, n, Morph(len(entries), np.arange(len(entries)), np.zeros(len(entries), np.int64), F([e[0] for e in entries]), F([e[1] for e in entries]))


def test_one_target_at_weight_one_is_base_plus_delta_in_one_rounding():
    base_p, base_n, morph, _ = CASES["22 triangles, 1 targets"]
    got = morph_host(base_p, base_n, *morph.lists, F([1.0]))[0].reshape(-1, 3)
    want = base_p.reshape(-1, 3).copy()
    want[morph.corners] = want[morph.corners] + morph.dp
    assert got.tobytes() == want.tobytes()


def test_the_order_of_the_additions_is_the_targets():
    a, b, c = F(1.0), F(1.0), F(-2.0 ** 24)
    p = F(2.0 ** 24)
    forward, backward = ((p + a) + b) + c, ((p + c) + b) + a
    assert forward.dtype == F and backward.dtype == F and forward != backward, "the values must tell the two orders apart in binary32"
    base_p, base_n, morph = _one_corner([((a, 0, 0), (0, 0, 0)), ((b, 0, 0), (0, 0, 0)), ((c, 0, 0), (0, 0, 0))], base_p=(p, 0, 0))
    got = morph_host(base_p, base_n, *morph.lists, F([1, 1, 1]))[0]
    assert got[0, 0] == forward and got[0, 0] != backward


def test_an_entry_of_weight_zero_is_skipped_not_multiplied():
    huge = F(3e38)
    base_p, base_n, morph = _one_corner([((huge, -huge, huge), (huge, huge, huge))], base_p=(1.5, -2.5, 0.25), base_n=(0.0, 0.0, 2.0))
    for zero in (F(0.0), F(-0.0)):
        got = morph_host(base_p, base_n, *morph.lists, F([zero]))
        _same_bytes(got, (base_p, base_n, pack_normal64(base_n.reshape(-1, 3)).reshape(-1, 3)), "weight %r" % zero)
    # and with a weight the same entry overflows: the twin counts it where the kernel flags it
    assert not np.isfinite(morph_host(base_p, base_n, *morph.lists, F([2.0]))[0]).all()


def test_normals_that_cancel_keep_the_base_normal():
    base_p, base_n, morph = _one_corner([((0.5, 0, 0), (0, 0, -0.5)), ((0, 0.5, 0), (0, 0, -0.5))])
    got = morph_host(base_p, base_n, *morph.lists, F([1, 1]))
    assert got[0][0, :3].tobytes() == F([0.5, 0.5, 0.0]).tobytes()
    assert got[1].tobytes() == base_n.tobytes(), "a normal of zero length must leave the base normal"
    inf_len = _one_corner([((0, 0, 0), (2e19, 2e19, 2e19))])
    assert morph_host(inf_len[0], inf_len[1], *inf_len[2].lists, F([1]))[1].tobytes() == inf_len[1].tobytes(), "so must one whose squared length overflows"


@pytest.mark.parametrize("name", sorted(CASES))
def test_positions_against_a_float64_evaluation(name):
    """k products and k additions: to first order (k + 1) 2^-24 of the absolute sum per coordinate; (k + 2) covers the second-order terms up to k = 1024."""
    base_p, base_n, morph, w = CASES[name]
    truth = base_p.reshape(-1, 3).astype(np.float64)
    mass = np.abs(truth)
    k = np.zeros(len(truth))
    for t in range(morph.target_count):
        if w[t] == 0:
            continue
        a, b = int(morph.offsets[t]), int(morph.offsets[t + 1])
        idx = morph.corners[a:b]
        term = np.float64(w[t]) * morph.dp[a:b].astype(np.float64)
        truth[idx] += term
        mass[idx] += np.abs(term)
        k[idx] += 1
    got = morph_host(base_p, base_n, *morph.lists, w)[0].reshape(-1, 3).astype(np.float64)
    bound = (k[:, None] + 2.0) * 2.0 ** -24 * mass
    print("%s: largest error %.3g of its bound" % (name, float((np.abs(got - truth) / np.maximum(bound, 1e-300)).max())))
    excess = np.abs(got - truth) - bound
    assert (excess <= 0.0).all(), "%s: %d coordinates beyond the bound" % (name, int((excess > 0).sum()))


@pytest.mark.parametrize("name", ["1 triangles, 1024 targets", "22 triangles, 3 targets", "86 triangles, 1024 targets", "85 triangles, 1 targets"])
def test_with_a_skin_the_twin_is_the_skin_of_the_unnormalised_morph(name):
    base_p, base_n, morph, w = CASES[name]
    rng = np.random.RandomState(7)
    for bone_count in (2, 1024):
        ids, sw = random_skin(rng, len(base_p), bone_count)
        bones = random_bones(rng, bone_count, scale=True)
        p, n, _ = morph_sums_numpy(base_p, base_n, morph, w)
        assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() > 1e-3, "the morphed normals are not unit: the skin must get them as they are"
        want = skin_host(p.reshape(-1, 9), n.reshape(-1, 9), ids, sw, bones)
        got = morph_host(base_p, base_n, *morph.lists, w, ids, sw, bones)
        _same_bytes(got, want, "%s, %d bones" % (name, bone_count))


def test_the_twin_refuses_what_the_bind_refuses():
    base_p, base_n, morph, w = CASES["22 triangles, 3 targets"]
    o, c, dp, dn = morph.lists

    def refused(*args):
        with pytest.raises(core.CoreError):
            morph_host(base_p, base_n, *args)

    refused(o + np.uint32(1), np.concatenate([c, c[:1]]), np.concatenate([dp, dp[:1]]), None, w)  # offsets that do not start at 0
    down = o.copy(); down[1], down[2] = o[2], o[1]
    if o[1] != o[2]:
        refused(down, c, dp, dn, w)
    bad = c.copy(); bad[-1] = 66
    refused(o, bad, dp, dn, w)
    twice = c.copy(); twice[1] = twice[0]
    refused(o, twice, dp, dn, w)
    swapped = c.copy(); swapped[[0, 1]] = swapped[[1, 0]]
    refused(o, swapped, dp, dn, w)
    for value in (np.nan, np.inf):
        d = dp.copy(); d[3, 1] = value
        refused(o, c, d, dn, w)
        d = dn.copy(); d[0, 2] = value
        refused(o, c, dp, d, w)
        bad_w = w.copy(); bad_w[1] = value
        refused(o, c, dp, dn, bad_w)
    refused(np.zeros(1026, np.uint32), c[:0], dp[:0], None, np.zeros(1025, F))  # 1025 targets


# ---- the host layer ----
def _snapshot(host):
    meshes = [tuple(x.tobytes() for x in host.get_mesh(m)) for m in range(host.get_num_meshes())]
    return meshes, device_arrays(host.device_scene()), host.mesh_morph_stats(), host.mesh_skin_stats(), host.is_rendering()


def test_every_refusal_leaves_the_host_as_it_was():
    host = _zoo()
    try:
        _, mesh = _meshes(host)
        p = host.get_mesh(mesh)[0]
        n = len(p)
        morph = bulge_targets(p)
        o, c, dp, dn = morph.lists
        w = F([0.5, -0.25, 1.5])
        before = _snapshot(host)
        bind, set_weights, unbind = "luminary_ext_bind_mesh_morph", "luminary_ext_set_mesh_weights", "luminary_ext_unbind_mesh_morph"
        u32 = C.c_uint32

        def refused(what, name, *args):
            assert _raw(name, host, *args) == INVALID_API_ARGUMENT, what
            assert _snapshot(host) == before, "a refused call (%s) changed the host" % what

        def bind_args(mesh=mesh, n=n, t=3, o=o, c=c, dp=dp, dn=dn):
            return u32(mesh), u32(n), u32(t), _ptr(o), _ptr(c), _ptr(dp), _ptr(dn)

        refused("unknown mesh", bind, *bind_args(mesh=host.get_num_meshes()))
        refused("one triangle short", bind, *bind_args(n=n - 1))
        refused("one triangle more", bind, *bind_args(n=n + 1))
        refused("no offsets", bind, *bind_args(o=None))
        refused("no corners", bind, *bind_args(c=None))
        refused("no deltas", bind, *bind_args(dp=None))
        refused("no targets", bind, *bind_args(t=0))
        refused("1025 targets", bind, *bind_args(t=1025, o=np.zeros(1026, np.uint32)))
        refused("offsets from 1", bind, *bind_args(o=o + np.uint32(1)))
        down = o.copy(); down[1], down[2] = o[2], o[1]
        assert o[1] != o[2]
        refused("offsets that decrease", bind, *bind_args(o=down))
        bad = c.copy(); bad[int(o[1]) - 1] = 3 * n
        refused("a corner that is 3 n", bind, *bind_args(c=bad))
        twice = c.copy(); twice[1] = twice[0]
        refused("a corner twice in a target", bind, *bind_args(c=twice))
        swapped = c.copy(); swapped[[0, 1]] = swapped[[1, 0]]
        refused("corners that decrease in a target", bind, *bind_args(c=swapped))
        for value in (np.nan, np.inf, -np.inf):
            d = dp.copy(); d[len(d) // 2, 1] = value
            refused("position delta %r" % value, bind, *bind_args(dp=d))
            d = dn.copy(); d[len(d) // 3, 2] = value
            refused("normal delta %r" % value, bind, *bind_args(dn=d))
        refused("weights for an unbound mesh", set_weights, u32(mesh), _ptr(w), u32(3))
        refused("an unbind for an unbound mesh", unbind, u32(mesh))
        host.bind_mesh_morph(mesh, n, *morph.lists)
        assert _snapshot(host) == before, "binding moves nothing"
        refused("another target count", set_weights, u32(mesh), _ptr(w), u32(2))
        refused("no weights", set_weights, u32(mesh), _ptr(None), u32(3))
        for value in (np.nan, np.inf):
            bad_w = w.copy(); bad_w[1] = value
            refused("weight %r" % value, set_weights, u32(mesh), _ptr(bad_w), u32(3))
        refused("a pose for a mesh without a skin", "luminary_ext_set_mesh_pose", u32(mesh), _ptr(np.zeros((1, 12), F)), u32(0))
        refused("a skin unbind for a mesh without a skin", "luminary_ext_unbind_mesh_skin", u32(mesh))
        moved = np.ascontiguousarray(p + F(0.5))
        refused("set_mesh_positions on a bound mesh", "luminary_ext_set_mesh_positions", u32(mesh), _ptr(moved), _ptr(None), u32(n))
        # 1024 targets are taken, without normal deltas too
        wide = random_morph(np.random.RandomState(3), n, 1024)
        host.bind_mesh_morph(mesh, n, wide.offsets, wide.corners, wide.dp, None)
        host.unbind_mesh_morph(mesh)
        assert _snapshot(host) == before
    finally:
        host.close()


def _same_scene(host, twin, where):
    a, b = device_arrays(host.device_scene()), device_arrays(twin.device_scene())
    assert sorted(a) == sorted(b)
    for key in sorted(a):
        assert a[key] == b[key], "%s: %s differs from the twin host's" % (where, key)
    return a


@pytest.mark.parametrize("which", ["emissive", "plain"])
def test_a_morphed_host_without_a_device_is_a_host_that_was_given_the_twin_s_vertices(which):
    host, twin = _zoo(), _zoo()
    try:
        mesh = _meshes(host)[0 if which == "emissive" else 1]
        base_p, base_n = host.get_mesh(mesh)[:2]
        morph = bulge_targets(base_p)
        lights_before = {k: v for k, v in device_arrays(host.device_scene()).items() if k.startswith("light_")}
        assert lights_before, "the zoo has lights"
        host.bind_mesh_morph(mesh, len(base_p), *morph.lists)
        made0 = host.mesh_morph_stats()["host_materialisations"]
        for step, w in enumerate((F([0.8, 0.0, -0.4]), F([0.0, 1.3, 0.6]))):
            host.set_mesh_weights(mesh, w)
            want_p, want_n, _ = morph_host(base_p, base_n, *morph.lists, w)
            assert not np.array_equal(want_p, base_p)
            made = host.mesh_morph_stats()["host_materialisations"] - made0
            assert made == (step + 1 if which == "emissive" else step), "an emitter is blended on the host at once, any other mesh when something reads it"
            got = host.get_mesh(mesh)
            _same_bytes((got[0], got[1]), (want_p, want_n), "%s mesh, weights %d: get_mesh" % (which, step))
            host.get_mesh(mesh)
            assert host.mesh_morph_stats()["host_materialisations"] - made0 == step + 1, "read twice, blended once"
            assert host.mesh_skin_stats()["host_materialisations"] == host.mesh_morph_stats()["host_materialisations"], "one counter"
            twin.set_mesh_positions(mesh, want_p, want_n)
            a = _same_scene(host, twin, "%s mesh, weights %d" % (which, step))
            lights = {k: v for k, v in a.items() if k.startswith("light_")}
            assert (lights != lights_before) == (which == "emissive"), "the light arrays follow a morphed emitter and nothing else"
        host.unbind_mesh_morph(mesh)
        final = host.get_mesh(mesh)
        _same_bytes((final[0], final[1]), (want_p, want_n), "after the unbind the mesh is the last shape")
        moved = np.ascontiguousarray(want_p + F(0.25))
        host.set_mesh_positions(mesh, moved)  # plain again
        twin.set_mesh_positions(mesh, moved)
        assert device_arrays(host.device_scene()) == device_arrays(twin.device_scene())
    finally:
        host.close(); twin.close()


@pytest.mark.parametrize("first", ["morph", "skin"])
@pytest.mark.parametrize("unbind_first", ["morph", "skin"])
def test_a_mesh_has_one_rest_shape(first, unbind_first):
    host, twin = _zoo(), _zoo()
    try:
        mesh = _meshes(host)[1]
        rest_p, rest_n = host.get_mesh(mesh)[:2]
        n = len(rest_p)
        morph = bulge_targets(rest_p)
        ids, sw = two_bone_weights(rest_p)
        w, bones = F([0.7, -0.3, 1.2]), two_bone_bend(rest_p, 0.5, 0.2)

        def holds(want, where):
            got = host.get_mesh(mesh)
            _same_bytes((got[0], got[1]), want[:2], where)
            twin.set_mesh_positions(mesh, want[0], want[1])
            _same_scene(host, twin, where)

        if first == "morph":  # bind morph, then skin, then set weights and pose
            host.bind_mesh_morph(mesh, n, *morph.lists)
            host.set_mesh_weights(mesh, w)
            holds(morph_host(rest_p, rest_n, *morph.lists, w), "morph alone")
            host.bind_mesh_skin(mesh, ids, sw, 2)  # shares the rest shape: NOT the morphed shape it holds now
            holds(morph_host(rest_p, rest_n, *morph.lists, w), "a skin without a pose shapes nothing")
            host.set_mesh_pose(mesh, bones)
        else:  # bind skin and pose, then the morph over the same rest pose
            host.bind_mesh_skin(mesh, ids, sw, 2)
            host.set_mesh_pose(mesh, bones)
            holds(skin_host(rest_p, rest_n, ids, sw, bones), "skin alone")
            host.bind_mesh_morph(mesh, n, *morph.lists)  # shares the rest pose: NOT the posed shape it holds now
            holds(skin_host(rest_p, rest_n, ids, sw, bones), "a morph without weights shapes nothing")
            host.set_mesh_weights(mesh, w)
        both = morph_host(rest_p, rest_n, *morph.lists, w, ids, sw, bones)
        assert both[0].tobytes() not in (morph_host(rest_p, rest_n, *morph.lists, w)[0].tobytes(), skin_host(rest_p, rest_n, ids, sw, bones)[0].tobytes())
        holds(both, "both")
        # binding a kind again while the other is bound keeps the rest shape
        other = bulge_targets(rest_p, 2, 0.1)
        host.bind_mesh_morph(mesh, n, *other.lists)
        holds(skin_host(rest_p, rest_n, ids, sw, bones), "new targets: weights 0 over the same rest")
        host.set_mesh_weights(mesh, w[:2])
        holds(morph_host(rest_p, rest_n, *other.lists, w[:2], ids, sw, bones), "new targets")
        host.bind_mesh_skin(mesh, ids, sw, 3)
        holds(morph_host(rest_p, rest_n, *other.lists, w[:2]), "a new skin: no pose over the same rest")
        host.set_mesh_pose(mesh, np.concatenate([bones, bones[:1]]))
        holds(morph_host(rest_p, rest_n, *other.lists, w[:2], ids, sw, bones), "a new skin")
        refused = _raw("luminary_ext_set_mesh_positions", host, C.c_uint32(mesh), _ptr(rest_p), _ptr(None), C.c_uint32(n))
        assert refused == INVALID_API_ARGUMENT
        if unbind_first == "morph":
            host.unbind_mesh_morph(mesh)
            last = skin_host(rest_p, rest_n, ids, sw, bones)
            holds(last, "the skin alone over the rest")
            assert _raw("luminary_ext_set_mesh_positions", host, C.c_uint32(mesh), _ptr(rest_p), _ptr(None), C.c_uint32(n)) == INVALID_API_ARGUMENT
            host.unbind_mesh_skin(mesh)
        else:
            host.unbind_mesh_skin(mesh)
            last = morph_host(rest_p, rest_n, *other.lists, w[:2])
            holds(last, "the morph alone over the rest")
            assert _raw("luminary_ext_set_mesh_positions", host, C.c_uint32(mesh), _ptr(rest_p), _ptr(None), C.c_uint32(n)) == INVALID_API_ARGUMENT
            host.unbind_mesh_morph(mesh)
        holds(last, "plain again: the current shape")
        moved = np.ascontiguousarray(last[0] + F(0.25))
        host.set_mesh_positions(mesh, moved)
        twin.set_mesh_positions(mesh, moved)
        _same_scene(host, twin, "moved by the host route")
    finally:
        host.close(); twin.close()


def test_a_binding_that_never_shaped_the_mesh_leaves_with_the_rest_shape():
    host = _zoo()
    try:
        mesh = _meshes(host)[1]
        rest_p, rest_n = host.get_mesh(mesh)[:2]
        morph = bulge_targets(rest_p)
        ids, sw = two_bone_weights(rest_p)
        host.bind_mesh_morph(mesh, len(rest_p), *morph.lists)
        host.set_mesh_weights(mesh, F([1, 1, 1]))
        host.bind_mesh_skin(mesh, ids, sw, 2)
        host.unbind_mesh_morph(mesh)  # the skin has no pose: the mesh is the rest shape again
        got = host.get_mesh(mesh)
        _same_bytes((got[0], got[1]), (rest_p, rest_n), "the rest shape")
        host.unbind_mesh_skin(mesh)
        got = host.get_mesh(mesh)
        _same_bytes((got[0], got[1]), (rest_p, rest_n), "plain")
        # a mesh with a morph alone: binding again makes the current shape the base shape, as a skin does
        host.bind_mesh_morph(mesh, len(rest_p), *morph.lists)
        host.set_mesh_weights(mesh, F([1, 0, 0]))
        first = morph_host(rest_p, rest_n, *morph.lists, F([1, 0, 0]))
        host.bind_mesh_morph(mesh, len(rest_p), *morph.lists)
        host.set_mesh_weights(mesh, F([1, 0, 0]))
        got = host.get_mesh(mesh)
        _same_bytes((got[0], got[1]), morph_host(first[0], first[1], *morph.lists, F([1, 0, 0]))[:2], "bound again")
    finally:
        host.close()


def test_the_stats_structs_have_the_headers_layout():
    src = '#include "luminary_amd.h"\n#include "lum_core.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(LumMeshMorphStats), ' \
          'sizeof(LuminaryMeshMorphStats), offsetof(LumMeshMorphStats, last_bytes_uploaded), offsetof(LumMeshMorphStats, seconds_morph), ' \
          'offsetof(LuminaryMeshMorphStats, seconds), offsetof(LuminaryMeshMorphStats, host_materialisations), sizeof(LumMeshSkinStats), sizeof(LuminaryMeshSkinStats));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "p")]).split()]
    a, b = core.MeshMorphStats, luminary_amd.MeshMorphStats
    assert got == [C.sizeof(a), C.sizeof(b), a.last_bytes_uploaded.offset, a.seconds_morph.offset, b.seconds.offset, b.host_materialisations.offset,
                   C.sizeof(core.MeshSkinStats), C.sizeof(luminary_amd.MeshSkinStats)] == [56, 64, 24, 48, 32, 56, 56, 64]
    assert [name for name, _ in a._fields_] == ["applied", "rebuild_downloads", "last_meshes", "last_launches", "last_bytes_uploaded", "seconds", "seconds_upload", "seconds_morph"]


def test_stand_alone_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/support/mesh_morph_check.cpp: the twin over the sizes, 1, 3 and 1024 targets, the last target named, with and without a skin, as a program of its own
    built with the sanitizers."""
    exe = str(tmp_path / "mesh_morph_check")
    host = os.path.join(ROOT, "luminary_amd", "csrc", "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-ffp-contract=off",
           os.path.join(ROOT, "tests", "support", "mesh_morph_check.cpp"), os.path.join(host, "mesh_deform.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)  # (the runtimes are linked statically: the program needs nothing preloaded)
    assert ran.returncode == 0 and "mesh_morph_check: ok" in ran.stdout, ran.stdout
