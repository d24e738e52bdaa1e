"""Skinned meshes on the host side (include/lum_core.h lumc_skin_host; include/luminary_amd.h luminary_ext_bind_mesh_skin / _set_mesh_pose; csrc/host/mesh_deform.h,
mesh_deform.cpp, api.cpp), no GPU.

skin(rest, ids, weights, bones) is one function compiled twice; this file holds the host's compilation - the twin - to a numpy restatement of the definition, float32
one operation at a time with the normal packed in float64, byte for byte, and to a float64 evaluation within the rounding bound; tests/test_mesh_skin_gpu.py holds
the device's to the twin. Then the host layer: what it refuses, that the host mesh of a posed mesh is the twin's output whenever something reads it, and that the
device scene it hands out is, byte for byte, that of a host which was given those vertices."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import luminary_amd
from luminary_amd import Host, core, scenes
from luminary_amd.core import skin_host
from test_mesh_positions_api import device_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_API_ARGUMENT = 3
F = np.float32
SIZES = [1, 21, 22, 85, 86]  # triangles: 3, 63, 66, 255, 258 corners - either side of a wave and of a workgroup


# ---- bones and weights shared with tests/test_mesh_skin_gpu.py ----
def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    k = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * k + (1.0 - np.cos(angle)) * (k @ k)


def bone(r=None, t=(0.0, 0.0, 0.0), pivot=(0.0, 0.0, 0.0)):
    """A bone [12] float32, row-major 3 x 4: x -> r (x - pivot) + pivot + t."""
    r = np.eye(3) if r is None else np.asarray(r, dtype=np.float64)
    pivot = np.asarray(pivot, dtype=np.float64)
    return np.concatenate([r, (pivot - r @ pivot + np.asarray(t, dtype=np.float64)).reshape(3, 1)], axis=1).astype(F).reshape(12)


def two_bone_weights(positions):
    """ids and weights [n, 12] of a bend over two bones: the weight of bone 1 grows smoothly along the mesh's longest axis; slots 2 and 3 are empty."""
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    axis = int(np.argmax(hi - lo))
    u = np.clip((p[:, axis] - lo[axis]) / max(hi[axis] - lo[axis], 1e-9), 0.0, 1.0)
    s = (u * u * (3.0 - 2.0 * u)).astype(F)
    w = np.zeros((len(p), 4), F)
    w[:, 0], w[:, 1] = F(1.0) - s, s
    ids = np.zeros((len(p), 4), np.uint16)
    ids[:, 1] = 1
    return ids.reshape(-1, 12), w.reshape(-1, 12)


def two_bone_bend(positions, angle, lift=0.0):
    """The palette [2, 12] of that bend: bone 0 stays, bone 1 turns about the mesh's centre by `angle` and rises by `lift`."""
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    centre = 0.5 * (p.min(axis=0) + p.max(axis=0))
    return np.stack([bone(), bone(rotation((0.3, 0.2, 1.0), angle), (0.0, lift, 0.0), centre)])


def random_skin(rng, triangles, bone_count, empty_slots=0.3):
    """ids and weights [n, 12] over bone_count bones: weights of a corner sum to about 1, a share of the slots has weight exactly 0; the last bone is named."""
    c = 3 * triangles
    ids = rng.randint(0, bone_count, (c, 4)).astype(np.uint16)
    ids[rng.randint(0, c), rng.randint(0, 4)] = bone_count - 1
    ids[0, 0] = bone_count - 1
    w = rng.uniform(0.05, 1.0, (c, 4))
    w[rng.uniform(size=(c, 4)) < empty_slots] = 0.0
    w[:, 0] = np.where(w.sum(axis=1) == 0.0, 1.0, w[:, 0])
    w /= w.sum(axis=1, keepdims=True)
    return ids.reshape(-1, 12), w.astype(F).reshape(-1, 12)


def random_bones(rng, bone_count, scale=False):
    out = np.zeros((bone_count, 12), F)
    for b in range(bone_count):
        r = rotation(rng.normal(size=3), rng.uniform(-1.5, 1.5)) * (rng.uniform(0.5, 2.0) if scale else 1.0)
        out[b] = bone(r, rng.uniform(-2.0, 2.0, 3), rng.uniform(-1.0, 1.0, 3))
    return out


def unit_normals(rng, triangles):
    n = rng.normal(size=(3 * triangles, 3))
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F).reshape(-1, 9)


# ---- the definition, restated ----
def pack_normal64(n):
    """scene.cpp pack_normal in float64, one operation at a time ([c, 3] float32 -> [c] uint32)."""
    with np.errstate(all="ignore"):
        x, y, z = (n[:, k].astype(np.float64) for k in range(3))
        rn = 1.0 / (np.abs(x) + np.abs(y) + np.abs(z))
        x, y, z = x * rn, y * rn, z * rn
        t = np.fmax(np.fmin(-z, 1.0), 0.0)
        x = x + np.where(x >= 0.0, t, -t)
        y = y + np.where(y >= 0.0, t, -t)
        x, y = np.fmax(np.fmin(x, 1.0), -1.0), np.fmax(np.fmin(y, 1.0), -1.0)
        x, y = (x + 1.0) * 0.5, (y + 1.0) * 0.5
        xu, yu = np.floor(x * 65535.0 + 0.5).astype(np.uint32), np.floor(y * 65535.0 + 0.5).astype(np.uint32)
    return (yu << np.uint32(16)) | xu


def skin_numpy(rest_positions, rest_normals, ids, weights, bones):
    """skin() in float32 arrays - numpy rounds every float32 operation once - in the order of the definition. Returns positions, normals [n, 9], packed [n, 3]."""
    p, n = np.asarray(rest_positions, F).reshape(-1, 3), np.asarray(rest_normals, F).reshape(-1, 3)
    i, w, m = np.asarray(ids).reshape(-1, 4), np.asarray(weights, F).reshape(-1, 4), np.asarray(bones, F).reshape(-1, 3, 4)
    ap, an = np.zeros_like(p), np.zeros_like(n)
    with np.errstate(all="ignore"):
        for j in range(4):
            b, on = m[i[:, j]], w[:, j] != 0
            for r in range(3):
                t = ((b[:, r, 0] * p[:, 0] + b[:, r, 1] * p[:, 1]) + b[:, r, 2] * p[:, 2]) + b[:, r, 3]
                u = (b[:, r, 0] * n[:, 0] + b[:, r, 1] * n[:, 1]) + b[:, r, 2] * n[:, 2]
                ap[:, r] = np.where(on, ap[:, r] + w[:, j] * t, ap[:, r])
                an[:, r] = np.where(on, an[:, r] + w[:, j] * u, an[:, r])
        len2 = (an[:, 0] * an[:, 0] + an[:, 1] * an[:, 1]) + an[:, 2] * an[:, 2]
        ok = (len2 > 0) & np.isfinite(len2)
        rl = F(1.0) / np.sqrt(len2)
        out_n = np.where(ok[:, None], an * rl[:, None], n)
    assert ap.dtype == F and out_n.dtype == F
    return ap.reshape(-1, 9), out_n.reshape(-1, 9), pack_normal64(out_n).reshape(-1, 3)


def _same_bytes(got, want, what):
    for name, a, b in zip(("positions", "normals", "packed words"), got, want):
        a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
        assert a.shape == b.shape and np.array_equal(a, b), "%s: %d of %d %s differ" % (what, int((a != b).sum()), a.size, name)


def _cases():
    """name -> (rest positions, rest normals, ids, weights, bones)"""
    out = {}
    for n in SIZES:
        rng = np.random.RandomState(n)
        p, nrm = rng.uniform(-3.0, 3.0, (n, 9)).astype(F), unit_normals(rng, n)
        rigid_ids, rigid_w = np.zeros((n, 12), np.uint16), np.tile(F([1, 0, 0, 0]), (n, 3))
        out["%d triangles, one bone, rigid" % n] = (p, nrm, rigid_ids, rigid_w, random_bones(rng, 1))
        ids, w = random_skin(rng, n, 7, empty_slots=0.0)
        out["%d triangles, four-bone blends" % n] = (p, nrm, ids, w, random_bones(rng, 7, scale=True))
        ids, w = random_skin(rng, n, 1024, empty_slots=0.5)
        out["%d triangles, zero-weight slots, 1024 bones" % n] = (p, nrm, ids, w, random_bones(rng, 1024))
    rng = np.random.RandomState(99)
    n = 22
    p, nrm = rng.uniform(-3.0, 3.0, (n, 9)).astype(F), unit_normals(rng, n)
    # normals that cancel: two slots of weight 1/2, one bone the other's mirror image in its 3 x 3 part
    r = rotation((1.0, 2.0, 0.5), 0.7)
    out["normals that cancel to zero length"] = (p, nrm, np.tile(np.uint16([0, 1, 0, 0]), (n, 3)), np.tile(F([0.5, 0.5, 0, 0]), (n, 3)), np.stack([bone(r, (1, 0, 0)), bone(-r, (0, 1, 0))]))
    # -0 among positions, normals, weights and matrix entries
    pz, nz = p.copy(), nrm.copy()
    pz[::2, 0], pz[1::3, 4], nz[::2, 2] = F(-0.0), F(-0.0), F(-0.0)
    bz = np.stack([bone(), bone(rotation((0, 0, 1), np.pi / 2), (0, -0.0, 0))])
    bz[bz == 0] = F(-0.0)
    wz = np.tile(F([0.5, 0.5, -0.0, 0.0]), (n, 3))
    wz[::3] = np.tile(F([-0.0, 0.0, 1.0, 0.0]), 3)
    out["-0 inputs"] = (pz, nz, np.tile(np.uint16([0, 1, 0, 1]), (n, 3)), wz, bz)
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_twin_is_the_definition_byte_for_byte(name):
    rest_p, rest_n, ids, w, bones = CASES[name]
    got, want = skin_host(rest_p, rest_n, ids, w, bones), skin_numpy(rest_p, rest_n, ids, w, bones)
    _same_bytes(got, want, name)
    assert np.isfinite(got[0]).all()
    if name.startswith("normals that cancel"):
        assert np.array_equal(got[1].view(np.uint32), np.asarray(rest_n).view(np.uint32)), "a normal of zero length must leave the rest normal"
    else:
        lengths = np.linalg.norm(got[1].reshape(-1, 3).astype(np.float64), axis=1)
        assert np.abs(lengths - 1.0).max() < 4e-7, name


@pytest.mark.parametrize("name", sorted(CASES))
def test_positions_against_a_float64_evaluation(name):
    """Every term w_j (m_j p + t_j) passes through at most sixteen roundings of relative size 2^-24 on its way into the sum."""
    rest_p, rest_n, ids, w, bones = CASES[name]
    p, i, w64, m = rest_p.reshape(-1, 3).astype(np.float64), ids.reshape(-1, 4), w.reshape(-1, 4).astype(np.float64), bones.reshape(-1, 3, 4).astype(np.float64)
    truth, bound = np.zeros_like(p), np.zeros_like(p)
    for j in range(4):
        b = m[i[:, j]]
        truth += w64[:, j:j + 1] * (np.einsum("crk,ck->cr", b[:, :, :3], p) + b[:, :, 3])
        bound += np.abs(w64[:, j:j + 1]) * (np.einsum("crk,ck->cr", np.abs(b[:, :, :3]), np.abs(p)) + np.abs(b[:, :, 3]))
    got = skin_host(rest_p, rest_n, ids, w, bones)[0].reshape(-1, 3).astype(np.float64)
    excess = np.abs(got - truth) - 16.0 * 2.0 ** -24 * bound
    print("%s: largest error %.3g of its bound" % (name, float((np.abs(got - truth) / np.maximum(16.0 * 2.0 ** -24 * bound, 1e-300)).max())))
    assert (excess <= 0.0).all(), "%s: %d coordinates beyond the bound" % (name, int((excess > 0).sum()))


def test_the_twin_refuses_what_it_cannot_index():
    rest_p, rest_n, ids, w, bones = CASES["22 triangles, four-bone blends"]
    bad = ids.copy()
    bad[-1, -1] = 7
    with pytest.raises(core.CoreError):
        skin_host(rest_p, rest_n, bad, w, bones)
    with pytest.raises(core.CoreError):
        skin_host(rest_p, rest_n, ids, w, np.zeros((1025, 12), F))


# ---- the host layer ----
def _zoo():
    return scenes.zoo_scene(32, 32, 2)


def _meshes(host):
    """(a mesh with an emissive triangle, a larger mesh without)"""
    emits = [m for m in range(host.get_num_meshes()) if any(host.get_material(int(i)).emission_active for i in set(host.get_mesh(m)[3]))]
    plain = [m for m in range(host.get_num_meshes()) if m not in emits and len(host.get_mesh(m)[3]) >= 8]
    assert emits and plain
    return emits[0], plain[0]


def _raw(name, host, *args):
    fn = getattr(luminary_amd._lib(), name)
    fn.restype = C.c_uint64
    return fn(host._h, *args)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else C.c_void_p(0)


def _snapshot(host):
    meshes = [tuple(x.tobytes() for x in host.get_mesh(m)) for m in range(host.get_num_meshes())]
    return meshes, device_arrays(host.device_scene()), host.mesh_skin_stats(), host.is_rendering()


def test_every_refusal_leaves_the_host_as_it_was():
    host = _zoo()
    try:
        _, mesh = _meshes(host)
        p = host.get_mesh(mesh)[0]
        n = len(p)
        ids, w = two_bone_weights(p)
        pose = two_bone_bend(p, 0.4)
        before = _snapshot(host)
        bind, set_pose, unbind = "luminary_ext_bind_mesh_skin", "luminary_ext_set_mesh_pose", "luminary_ext_unbind_mesh_skin"

        def refused(what, name, *args):
            assert _raw(name, host, *args) == INVALID_API_ARGUMENT, what
            assert _snapshot(host) == before, "a refused call (%s) changed the host" % what

        u32 = C.c_uint32
        refused("unknown mesh", bind, u32(host.get_num_meshes()), _ptr(ids), _ptr(w), u32(n), u32(2))
        refused("one triangle short", bind, u32(mesh), _ptr(ids), _ptr(w), u32(n - 1), u32(2))
        refused("one triangle more", bind, u32(mesh), _ptr(ids), _ptr(w), u32(n + 1), u32(2))
        refused("no ids", bind, u32(mesh), _ptr(None), _ptr(w), u32(n), u32(2))
        refused("no weights", bind, u32(mesh), _ptr(ids), _ptr(None), u32(n), u32(2))
        for value in (-0.25, np.nan, np.inf):
            bad = w.copy()
            bad[n // 2, 5] = value
            refused("weight %r" % value, bind, u32(mesh), _ptr(ids), _ptr(bad), u32(n), u32(2))
        refused("an id that is bone_count", bind, u32(mesh), _ptr(ids), _ptr(w), u32(n), u32(1))
        refused("no bones", bind, u32(mesh), _ptr(ids), _ptr(w), u32(n), u32(0))
        refused("1025 bones", bind, u32(mesh), _ptr(ids), _ptr(w), u32(n), u32(1025))
        refused("a pose for an unbound mesh", set_pose, u32(mesh), _ptr(pose), u32(2))
        refused("an unbind for an unbound mesh", unbind, u32(mesh))
        host.bind_mesh_skin(mesh, ids, w, 2)
        assert _snapshot(host) == before, "binding moves nothing"
        refused("another bone count", set_pose, u32(mesh), _ptr(np.concatenate([pose, pose[:1]])), u32(3))
        refused("no bones in a pose", set_pose, u32(mesh), _ptr(None), u32(2))
        for value in (np.nan, -np.inf):
            bad = pose.copy()
            bad[1, 7] = value
            refused("matrix entry %r" % value, set_pose, u32(mesh), _ptr(bad), u32(2))
        moved = np.ascontiguousarray(p + F(0.5))
        refused("set_mesh_positions on a bound mesh", "luminary_ext_set_mesh_positions", u32(mesh), _ptr(moved), _ptr(None), u32(n))
        # 1024 bones are taken
        host.bind_mesh_skin(mesh, ids, w, 1024)
        host.unbind_mesh_skin(mesh)
        assert _snapshot(host) == before
    finally:
        host.close()


@pytest.mark.parametrize("which", ["emissive", "plain"])
def test_a_posed_host_without_a_device_is_a_host_that_was_given_the_twin_s_vertices(which):
    host, twin = _zoo(), _zoo()
    try:
        mesh = _meshes(host)[0 if which == "emissive" else 1]
        rest_p, rest_n = host.get_mesh(mesh)[:2]
        ids, w = two_bone_weights(rest_p)
        lights_before = {k: v for k, v in device_arrays(host.device_scene()).items() if k.startswith("light_")}
        assert lights_before, "the zoo has lights"
        host.bind_mesh_skin(mesh, ids, w, 2)
        for step, angle in enumerate((0.5, -0.3)):
            pose = two_bone_bend(rest_p, angle, 0.2)
            host.set_mesh_pose(mesh, pose)
            want_p, want_n, _ = skin_host(rest_p, rest_n, ids, w, pose)
            assert not np.array_equal(want_p, rest_p)
            made = host.mesh_skin_stats()["host_materialisations"]
            assert made == (step + 1 if which == "emissive" else step), "an emitter is posed on the host at once, any other mesh when something reads it"
            got = host.get_mesh(mesh)
            _same_bytes((got[0], got[1]), (want_p, want_n), "%s mesh, pose %d: get_mesh" % (which, step))
            host.get_mesh(mesh)
            assert host.mesh_skin_stats()["host_materialisations"] == step + 1, "read twice, posed once"
            twin.set_mesh_positions(mesh, want_p, want_n)
            a, b = device_arrays(host.device_scene()), device_arrays(twin.device_scene())
            assert sorted(a) == sorted(b)
            for key in sorted(a):
                assert a[key] == b[key], "%s mesh, pose %d: %s differs from the twin host's" % (which, step, key)
            lights = {k: v for k, v in a.items() if k.startswith("light_")}
            assert (lights != lights_before) == (which == "emissive"), "the light arrays follow a posed emitter and nothing else"
        host.unbind_mesh_skin(mesh)
        final = host.get_mesh(mesh)
        _same_bytes((final[0], final[1]), (want_p, want_n), "after the unbind the mesh is the last pose")
        moved = np.ascontiguousarray(want_p + F(0.25))
        host.set_mesh_positions(mesh, moved)  # plain again
        twin.set_mesh_positions(mesh, moved)
        assert device_arrays(host.device_scene()) == device_arrays(twin.device_scene())
    finally:
        host.close(); twin.close()


def test_the_stats_structs_have_the_headers_layout():
    src = '#include "luminary_amd.h"\n#include "lum_core.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(LumMeshSkinStats), ' \
          'sizeof(LuminaryMeshSkinStats), offsetof(LumMeshSkinStats, last_bytes_uploaded), offsetof(LumMeshSkinStats, seconds_skin), ' \
          'offsetof(LuminaryMeshSkinStats, seconds), offsetof(LuminaryMeshSkinStats, host_materialisations));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "p")]).split()]
    a, b = core.MeshSkinStats, luminary_amd.MeshSkinStats
    assert got == [C.sizeof(a), C.sizeof(b), a.last_bytes_uploaded.offset, a.seconds_skin.offset, b.seconds.offset, b.host_materialisations.offset] == [56, 64, 24, 48, 32, 56]
    assert core.DIRTY_MESH_SKIN == 512 and not (core.DIRTY_ALL & core.DIRTY_MESH_SKIN)
    # the structs this leaves alone
    assert C.sizeof(core.ResidentRefitStats) == 80 and C.sizeof(core.InstanceUpdateStats) == 88 and C.sizeof(core.MeshRefitStats) == 96


def test_stand_alone_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/support/mesh_skin_check.cpp: the twin over the sizes, 1 and 1024 bones, the last bone named, as a program of its own built with the sanitizers."""
    exe = str(tmp_path / "mesh_skin_check")
    host = os.path.join(ROOT, "luminary_amd", "csrc", "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-ffp-contract=off",
           os.path.join(ROOT, "tests", "support", "mesh_skin_check.cpp"), os.path.join(host, "mesh_deform.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)  # (the runtimes are linked statically: the program needs nothing preloaded)
    assert ran.returncode == 0 and "mesh_skin_check: ok" in ran.stdout, ran.stdout
