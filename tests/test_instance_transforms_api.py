"""luminary_ext_set_instance_transforms on the host side (include/luminary_amd.h; csrc/host/api.cpp, scene.cpp), no GPU: what the call accepts, that a rejected
call changes nothing, and that the device scene the encoder brings up to date - the instance transforms, and the light tree behind them - is, byte for byte, the
one that luminary_host_set_instance gives for the same values set one by one. tests/test_instance_update_gpu.py renders from it."""
import ctypes as C

import numpy as np
import pytest

import luminary_amd
from luminary_amd import Host, Instance, Vec3, core, scenes
from test_mesh_positions_api import device_arrays

INVALID_API_ARGUMENT = 3


def view_arrays(view):
    """device_arrays and the rest of what an instance edit could touch."""
    out = device_arrays(view)
    out["instance_mesh_ids"] = C.string_at(view.instance_mesh_ids, 4 * view.num_instances)
    out["materials"] = C.string_at(view.materials, 32 * view.num_materials)
    return out


def copy_instance(inst):
    out = Instance()
    C.memmove(C.byref(out), C.byref(inst), C.sizeof(Instance))
    return out


def instance_bytes(host):
    return [bytes(host.get_instance(i)) for i in range(host.get_num_instances())]


def moved_instances(host, step, every=3):
    """Every `every`-th instance of the host moved and rotated (and one of them scaled unevenly), as Instance records."""
    out = []
    for i in range(step % every, host.get_num_instances(), every):
        inst = host.get_instance(i)
        inst.position = Vec3(inst.position.x + 0.11 * (step + 1), inst.position.y + 0.05 * ((i % 5) - 2), inst.position.z - 0.07 * (step + 1))
        inst.rotation = Vec3(inst.rotation.x + 0.2 * (step + 1), inst.rotation.y - 0.35, inst.rotation.z + 0.1 * (i % 4))
        if i % 2:
            inst.scale = Vec3(inst.scale.x * 1.25, inst.scale.y * 0.8, inst.scale.z * 1.1)
        out.append(inst)
    return out


def _set_raw(host, instances, count=None):
    fn = luminary_amd._lib().luminary_ext_set_instance_transforms
    fn.restype = C.c_uint64
    if instances is None:
        return fn(host._h, C.c_void_p(0), C.c_uint32(count))
    arr = (Instance * max(len(instances), 1))(*instances)
    return fn(host._h, arr, C.c_uint32(len(instances) if count is None else count))


def _scene(name):
    return scenes.zoo_scene(32, 32, 2) if name == "zoo" else scenes.example_scene(width=32, height=32, sphere_segments=6, ground_res=8)


def test_the_library_exports_the_interface():
    lib = luminary_amd._lib()
    names = ("luminary_ext_set_instance_transforms", "luminary_ext_set_instance_update", "luminary_ext_get_instance_update_stats", "lumc_set_instance_update",
             "lumc_instance_update_stats", "lumc_instance_boxes_probe", "lumc_resident_tree_probe", "lumc_host_bvh_nodes_probe")
    assert all(hasattr(lib, n) for n in names)
    assert core.DIRTY_INSTANCE_TRANSFORMS == 256 and core.DIRTY_ALL == 127 and core.DIRTY_ALL & core.DIRTY_INSTANCE_TRANSFORMS == 0
    assert C.sizeof(core.InstanceUpdateStats) == C.sizeof(luminary_amd.InstanceUpdateStats) == 88


@pytest.mark.parametrize("name", ["zoo", "example"])
def test_every_rejected_call_changes_nothing(name):
    host = _scene(name)
    n = host.get_num_instances()
    lost = host.new_instance(host.get_num_meshes() + 5)  # points at no mesh: inactive on the devices (its slot keeps the id)
    before_scene, before = view_arrays(host.device_scene()), instance_bytes(host)
    good = moved_instances(host, 0)
    assert len(good) >= 2
    cases = {"null pointer": None}
    def bad(change):
        inst = copy_instance(good[1])
        change(inst)
        return [good[0], inst, good[-1]]  # the offending entry in the middle: the ones before it must not be applied either
    cases["unknown id"] = bad(lambda i: setattr(i, "id", n + 1))
    cases["changed mesh_id"] = bad(lambda i: setattr(i, "mesh_id", (i.mesh_id + 1) % host.get_num_meshes()))
    inactive = host.get_instance(lost)
    cases["inactive instance"] = [good[0], inactive]
    for field in ("position", "rotation", "scale"):
        for axis in "xyz":
            for value in (np.nan, np.inf, -np.inf):
                cases["%s.%s = %r" % (field, axis, value)] = bad(lambda i, f=field, a=axis, x=value: setattr(getattr(i, f), a, x))
    assert len(cases) == 4 + 27
    for what, instances in cases.items():
        assert _set_raw(host, instances, 3 if instances is None else None) == INVALID_API_ARGUMENT, "%s: %s" % (name, what)
        assert instance_bytes(host) == before, "%s: a rejected call (%s) changed an instance" % (name, what)
    assert view_arrays(host.device_scene()) == before_scene
    assert _set_raw(host, [], 0) == 0 and _set_raw(host, None, 0) == 0  # nothing to do is no error ...
    assert instance_bytes(host) == before and view_arrays(host.device_scene()) == before_scene
    fn = luminary_amd._lib().luminary_ext_set_instance_update
    fn.restype = C.c_uint64
    assert fn(host._h, C.c_uint32(2)) == INVALID_API_ARGUMENT and fn(host._h, C.c_uint32(1)) == 0 and fn(host._h, C.c_uint32(0)) == 0
    assert fn(None, C.c_uint32(0)) != 0
    host.close()


@pytest.mark.parametrize("name", ["zoo", "example"])
def test_the_updated_device_scene_is_that_of_the_same_values_set_one_by_one(name):
    a, b = _scene(name), _scene(name)
    original = view_arrays(a.device_scene())  # both device scenes exist: the edits below take the partial paths
    assert view_arrays(b.device_scene()) == original
    for step in range(3):
        moved = moved_instances(a, step)
        a.set_instance_transforms(moved)
        for inst in moved:
            b.set_instance(inst)
        assert a.is_rendering()[1] == 0, "the integration did not restart"
        for inst in moved:
            assert bytes(a.get_instance(inst.id)) == bytes(inst)
        va, vb = view_arrays(a.device_scene()), view_arrays(b.device_scene())  # every intermediate state is encoded
        assert va["instance_transforms"] == vb["instance_transforms"] and va["instance_transforms"] != original["instance_transforms"]
        for key in vb:
            assert va[key] == vb[key], "%s, step %d: %s differs" % (name, step, key)
    for key in ("mesh_tri_offset", "vertices", "tri_tex", "instance_mesh_ids", "materials"):
        assert va[key] == original[key], "%s: %s changed" % (name, key)
    assert va["counts"][:4] == original["counts"][:4]  # (the light tree follows moved emitters: its node count may differ)
    if "light_bvh_tris" in original:
        assert sorted(np.frombuffer(va["light_tri_handles"], np.uint64).tolist()) == sorted(np.frombuffer(original["light_tri_handles"], np.uint64).tolist())  # the same lights, in the new tree's order
    a.close(); b.close()


def test_the_host_builder_probe_returns_the_tree_the_top_level_is_checked_against():
    rng = np.random.RandomState(5)
    lo = rng.uniform(-10, 10, (65, 3)).astype(np.float32)
    boxes = np.concatenate([lo, lo + rng.uniform(0.1, 2.0, (65, 3)).astype(np.float32)], axis=1)
    nodes, prims, depth = core.host_bvh_nodes_probe(boxes, 1, 16)
    assert sorted(prims.tolist()) == list(range(65)) and 1 <= depth <= 16 and 1 <= len(nodes) < 65
    child = nodes[:, 24:28]
    leaves = child[(child != 0xFFFFFFFF) & (child >= 0x80000000)]
    assert sorted((leaves & 0x0FFFFFFF).tolist()) == list(range(65)) and np.all((leaves >> 28) & 7 == 0), "one primitive per leaf"


def test_rows_and_boxes_of_the_host_functions_through_the_probe():
    host = scenes.zoo_scene(32, 32, 2)
    view = host.device_scene()
    nm = view.num_meshes
    mesh_boxes = np.zeros((nm, 6), np.float32)
    for m in range(nm):
        p = host.get_mesh(m)[0].reshape(-1, 3)
        mesh_boxes[m] = np.concatenate([p.min(axis=0), p.max(axis=0)]) if len(p) else 0.0
    rows, boxes, hittable = core.instance_boxes_probe(view, mesh_boxes, on_gpu=False)
    assert hittable.all() and np.isfinite(boxes).all() and np.all(boxes[:, :3] < boxes[:, 3:])
    t = np.frombuffer(C.string_at(view.instance_transforms, 32 * view.num_instances), np.float32).reshape(-1, 8)
    assert np.array_equal(rows[:, :, 3], t[:, :3]), "the rows' fourth column is the translation"
    host.close()
