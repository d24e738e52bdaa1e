"""luminary_ext_set_mesh_positions on the host side (include/luminary_amd.h; csrc/host/api.cpp, scene.cpp), no GPU: what the call accepts, that it overwrites
the host mesh in place, and that the device scene the encoder brings up to date - only the moved mesh's vertices, and the light tree behind them - is, byte for byte,
the device scene of a host that held the moved mesh before anything was encoded. tests/test_mesh_refit_gpu.py renders from it."""
import ctypes as C

import numpy as np
import pytest

import luminary_amd
from luminary_amd import Host, scenes

INVALID_API_ARGUMENT = 3


def bend(positions, amount=0.25, phase=0.0):
    """A smooth bend of every vertex by up to `amount` of the mesh's size ([n, 9] float32 in, [n, 9] float32 out; shared vertices stay shared)."""
    p = np.asarray(positions, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    size = float(max((hi - lo).max(), 1e-6))
    u = (p - lo) / size
    out = p.copy()
    out[:, 1] += amount * size * np.sin(2.1 * u[:, 0] + phase) * np.cos(1.7 * u[:, 2])
    out[:, 0] += 0.5 * amount * size * np.sin(1.3 * u[:, 1] + 0.4 + phase)
    return out.astype(np.float32).reshape(-1, 9)


def device_arrays(view):
    """The arrays of a device scene a mesh edit can touch, as bytes."""
    tris = int(np.ctypeslib.as_array(C.cast(view.mesh_tri_offset, C.POINTER(C.c_uint32)), shape=(view.num_meshes + 1,))[-1]) if view.num_meshes else 0
    out = {"counts": (view.num_meshes, view.num_instances, view.num_materials, view.num_lights, view.num_light_tree_nodes),
           "mesh_tri_offset": C.string_at(view.mesh_tri_offset, 4 * (view.num_meshes + 1)), "vertices": C.string_at(view.vertices, 48 * tris), "tri_tex": C.string_at(view.tri_tex, 16 * tris),
           "instance_transforms": C.string_at(view.instance_transforms, 32 * view.num_instances)}
    if view.light_tree_root and view.num_lights:
        sections = C.string_at(view.light_tree_root, 16)[10]
        out["light_tree_root"] = C.string_at(view.light_tree_root, 16 * (1 + 3 * sections))
        out["light_tree_nodes"] = C.string_at(view.light_tree_nodes, 64 * view.num_light_tree_nodes)
        out["light_tri_handles"] = C.string_at(view.light_tri_handles, 8 * view.num_lights)
        out["light_bvh_tris"] = C.string_at(view.light_bvh_tris, 48 * view.num_lights)
    return out


def _set_raw(host, mesh_id, positions, normals, count):
    fn = luminary_amd._lib().luminary_ext_set_mesh_positions
    fn.restype = C.c_uint64
    return fn(host._h, C.c_uint32(mesh_id), positions.ctypes.data_as(C.c_void_p) if positions is not None else C.c_void_p(0),
              normals.ctypes.data_as(C.c_void_p) if normals is not None else C.c_void_p(0), C.c_uint32(count))


def _scene(name, tmp_path):
    return scenes.cornell_host(str(tmp_path / name), 32, 32, 2) if name == "cornell" else scenes.zoo_scene(32, 32, 2)


def _emissive_meshes(host):
    out = []
    for m in range(host.get_num_meshes()):
        mats = set(int(x) for x in host.get_mesh(m)[3])
        if any(host.get_material(i).emission_active for i in mats):
            out.append(m)
    return out


def test_the_library_exports_the_three_functions():
    lib = luminary_amd._lib()
    assert all(hasattr(lib, n) for n in ("luminary_ext_set_mesh_positions", "luminary_ext_set_mesh_refit", "luminary_ext_get_mesh_refit_stats", "lumc_set_mesh_refit", "lumc_mesh_refit_stats"))
    from luminary_amd import core
    assert core.DIRTY_MESH_POSITIONS == 128 and core.DIRTY_ALL == 127 and core.DIRTY_MESHES == 16


@pytest.mark.parametrize("name", ["cornell", "zoo"])
def test_every_rejected_call_leaves_the_mesh_as_it_was(name, tmp_path):
    host = _scene(name, tmp_path)
    before_scene = device_arrays(host.device_scene())
    for m in range(host.get_num_meshes()):
        before = host.get_mesh(m)
        n = len(before[3])
        if n == 0:
            continue
        moved = np.ascontiguousarray(bend(before[0]))
        cases = {"mesh id": (host.get_num_meshes(), moved, None, n), "one triangle short": (m, moved, None, n - 1), "one triangle more": (m, np.concatenate([moved, moved[:1]]), None, n + 1),
                 "no positions": (m, None, None, n)}
        for bad, where in ((np.nan, 0), (np.inf, moved.size // 2), (-np.inf, moved.size - 1)):
            p = moved.copy().reshape(-1)
            p[where] = bad
            cases["position %r" % bad] = (m, p, None, n)
        for what, args in cases.items():
            assert _set_raw(host, *args) == INVALID_API_ARGUMENT, "%s, mesh %d: %s" % (name, m, what)
            after = host.get_mesh(m)
            assert all(np.array_equal(a, b) for a, b in zip(before, after)), "%s, mesh %d: a rejected call (%s) changed the mesh" % (name, m, what)
    assert device_arrays(host.device_scene()) == before_scene
    fn = luminary_amd._lib().luminary_ext_set_mesh_refit
    fn.restype = C.c_uint64
    assert fn(host._h, C.c_uint32(2), C.c_float(0.0)) == INVALID_API_ARGUMENT and fn(host._h, C.c_uint32(0), C.c_float(-1.0)) == INVALID_API_ARGUMENT
    assert fn(host._h, C.c_uint32(0), C.c_float(np.nan)) == INVALID_API_ARGUMENT and fn(host._h, C.c_uint32(1), C.c_float(2.0)) == 0
    host.close()


@pytest.mark.parametrize("name", ["cornell", "zoo"])
def test_the_updated_device_scene_is_that_of_a_host_that_held_the_moved_mesh_from_the_start(name, tmp_path):
    a, b = _scene(name, tmp_path), _scene(name, tmp_path)
    original = device_arrays(a.device_scene())  # a's device scene exists: the edits below take the partial path
    emissive = _emissive_meshes(a)
    assert emissive, "%s has no emissive mesh: the light tree would not move" % name
    targets = sorted(set(emissive[:2] + [0, a.get_num_meshes() - 1]))
    p_ptr = C.POINTER(C.c_float)()
    n_out = C.c_uint32()
    for step, m in enumerate(targets):
        pos, nrm, uv, mat = a.get_mesh(m)
        luminary_amd._call("luminary_ext_get_mesh", a._h, C.c_uint32(m), C.byref(p_ptr), None, None, None, C.byref(n_out))
        address = C.addressof(p_ptr.contents)
        moved = bend(pos, 0.25, 0.3 * step)
        normals = None if step % 2 else nrm  # both forms
        a.set_mesh_positions(m, moved, normals)
        b.set_mesh_positions(m, moved, normals)  # b has encoded nothing yet: its first device scene is a full encode of the moved meshes
        got = a.get_mesh(m)
        assert np.array_equal(got[0], moved) and np.array_equal(got[2], uv) and np.array_equal(got[3], mat)
        luminary_amd._call("luminary_ext_get_mesh", a._h, C.c_uint32(m), C.byref(p_ptr), None, None, None, C.byref(n_out))
        assert C.addressof(p_ptr.contents) == address, "the mesh was not overwritten in place"
        va = device_arrays(a.device_scene())  # every intermediate state is encoded
        assert va["vertices"] != original["vertices"]
    vb = device_arrays(b.device_scene())
    for key in vb:
        assert va[key] == vb[key], "%s: %s differs from a fresh host's" % (name, key)
    assert va["light_bvh_tris"] != original["light_bvh_tris"], "the emissive triangles did not move"
    assert va["tri_tex"] == original["tri_tex"] and va["mesh_tri_offset"] == original["mesh_tri_offset"] and va["instance_transforms"] == original["instance_transforms"]
    a.close(); b.close()


def test_a_hand_built_scene_with_the_moved_mesh_added_from_the_start():
    def build(positions, normals=(None, None, None)):
        h = Host()
        scenes.apply_benchmark_settings(h, 16, 16, 2, sky=(0.5, 0.5, 0.5))
        grey = h.add_material(scenes._material((0.6, 0.6, 0.6), 0.6))
        lamp = luminary_amd.default_material()
        lamp.emission_active = True
        lamp.emission.r, lamp.emission.g, lamp.emission.b = 4.0, 3.0, 2.0
        lamp = h.add_material(lamp)
        for k, p in enumerate(positions):
            m = h.add_mesh(p, np.full(len(p), lamp if k == 1 else grey, dtype=np.uint16), normals=normals[k])
            h.new_instance(m, position=(0.5 * k, 0.0, 0.0), rotation=(0.0, 0.3 * k, 0.0), scale=(1.0, 1.0 + 0.5 * k, 1.0))
        return h
    rng = np.random.RandomState(3)
    meshes = [rng.uniform(-2, 2, (n, 9)).astype(np.float32) for n in (37, 12, 5)]
    a = build(meshes)
    a.device_scene()
    moved = [bend(m, 0.25, 0.2) for m in meshes]
    explicit = rng.normal(size=moved[1].shape).astype(np.float32)
    a.set_mesh_positions(1, moved[1], explicit)
    a.set_mesh_positions(2, moved[2])  # face normals (the loader's rule: tests below)
    va, vb = device_arrays(a.device_scene()), device_arrays(build([meshes[0], moved[1], moved[2]], (None, explicit, a.get_mesh(2)[1])).device_scene())
    assert "light_bvh_tris" in va and va == vb


def test_null_normals_are_the_face_normals_of_an_obj_file_without_normals(tmp_path):
    rng = np.random.RandomState(4)
    first, moved = rng.uniform(-1, 1, (9, 9)).astype(np.float32), rng.uniform(-1, 1, (9, 9)).astype(np.float32)
    moved[3, 3:6] = moved[3, 0:3]  # a degenerate triangle: the loader's rule keeps the unnormalised (zero) normal
    def obj(path, tris):
        with open(path, "w") as f:
            f.write("o soup\n")
            for v in tris.reshape(-1, 3):
                f.write("v %s %s %s\n" % tuple(repr(float(x)) for x in v))
            for t in range(len(tris)):
                f.write("f %d %d %d\n" % (3 * t + 1, 3 * t + 2, 3 * t + 3))
    obj(str(tmp_path / "a.obj"), first)
    obj(str(tmp_path / "b.obj"), moved)
    a, b = Host(), Host()
    a.load_obj_file(str(tmp_path / "a.obj"))
    b.load_obj_file(str(tmp_path / "b.obj"))
    assert np.array_equal(a.get_mesh(0)[0], first) and np.array_equal(b.get_mesh(0)[0], moved)
    a.set_mesh_positions(0, moved, None)
    assert np.array_equal(a.get_mesh(0)[0], moved)
    assert a.get_mesh(0)[1].tobytes() == b.get_mesh(0)[1].tobytes()
    a.close(); b.close()
