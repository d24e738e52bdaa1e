"""Shutter on the device: lumc_mesh_shutter_key / lumc_shutter_time -> LUMC_DIRTY_MESH_SHUTTER -> csrc/host/mesh_shutter.hip k_shutter_vertices, scene_device.hip
shutter_meshes; and luminary_ext_shutter_open / luminary_ext_render_shutter over it (csrc/host/api.cpp).

The kernel's vertex records are held to the host twin's (lumc_shutter_host; tests/test_mesh_shutter.py holds that to the definition) byte for byte. The public
call's accumulators are held, bit for bit, to a reference loop on a fresh core context: per slice the view carries the twin's records (or the numpy float32 blend
of instances and camera, encoded by a second host), goes up through the flags the parent commit has, and the slice's sample ids are rendered without clearing.
Exact flavour, frame 48 x 32, at most 8 sample ids per test."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import luminary_amd
import oracle_lib
from luminary_amd import Vec3, scenes
from luminary_amd.core import (DIRTY_CONSTANTS, DIRTY_INSTANCE_TRANSFORMS, DIRTY_LIGHTS, DIRTY_MESH_POSITIONS, DIRTY_MESH_SHUTTER, DIRTY_MESH_SKIN, Core, CoreError,
                               shutter_host)
from test_light_refit import Built, with_light_arrays
from test_mesh_morph import bulge_targets
from test_mesh_positions_api import bend
from test_mesh_refit import soup
from test_mesh_refit_gpu import _emissive_mesh
from test_mesh_skin import two_bone_bend, two_bone_weights, unit_normals
from test_mesh_skin_gpu import _core, _first_triangle, _plain_meshes, _small_zoo, _view

pytestmark = pytest.mark.gpu
F, U = np.float32, np.uint32
SLICES, PER_SLICE = 4, 2


def _time(k, slices=SLICES):
    return F(2 * k + 1) / F(2 * slices)


def _mesh_records(view, mesh, triangles):
    """A copy of the view's [3 * triangles, 4] vertex records of a mesh, as words."""
    first = 3 * _first_triangle(view, mesh)
    return np.asarray(oracle_lib.view_arrays(view)["vertices"]).reshape(-1, 4)[first:first + 3 * triangles].astype(U).copy()


def _write_records(view, mesh, records):
    """Overwrites the view's vertex records of a mesh (the view's storage belongs to its host: nothing else reads it in between)."""
    records = np.ascontiguousarray(records, dtype=U).reshape(-1)
    buf = (C.c_uint32 * records.size).from_address(view.vertices + 16 * 3 * _first_triangle(view, mesh))
    np.frombuffer(buf, dtype=U)[:] = records


@contextlib.contextmanager
def _main_core(host):
    """The host's main context as a Core that does not own it."""
    core = Core.__new__(Core)
    core._lib, core._ctx = luminary_amd._lib(), C.c_void_p(host.core_context())
    try:
        yield core
    finally:
        core._ctx = C.c_void_p()


def _bits(a):
    return np.ascontiguousarray(a).view(U)


def _same_images(got, want, where):
    for name, a, b in zip(("first moment", "second moment"), got, want):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), "%s: %d of %d values of the %s differ" % (where, int((_bits(a) != _bits(b)).sum()), a.size, name)


def _images(host):
    fm, sm = host.accumulators()
    return np.asarray(fm).copy(), np.asarray(sm).copy()


def _differ(a, b, what):
    assert int((_bits(a[0]) != _bits(b[0])).sum()) > 20, what


def _reference_loop(store, mesh, rec_a, rec_b, first=0, slices=SLICES, light_arrays_of=None):
    """A fresh context that uploads the open view and, per slice, takes the twin's records of `mesh` through LUMC_DIRTY_MESH_POSITIONS (with light arrays from
    light_arrays_of(view, all records) and LUMC_DIRTY_LIGHTS when given) and renders the slice's ids without clearing. `store`: a host whose view carries the
    records."""
    view, core = _view(store), _core()
    try:
        _write_records(view, mesh, rec_a)
        core.upload(view)
        core.set_pixels(None)
        for k in range(slices):
            rec, flags = shutter_host(rec_a, rec_b, _time(k, slices))
            assert flags == 0
            _write_records(view, mesh, rec)
            if light_arrays_of is None:
                core.update(view, DIRTY_MESH_POSITIONS)
            else:
                core.update(light_arrays_of(view), DIRTY_MESH_POSITIONS | DIRTY_LIGHTS)
            core.render(first + k * PER_SLICE, PER_SLICE, samples_per_pass=PER_SLICE)
        fm, sm = core.accumulators()
        return np.asarray(fm).copy(), np.asarray(sm).copy()
    finally:
        core.close()


# ---- 1. the kernel against the twin ----
TRIANGLES = [1, 21, 22, 85, 86, 1000]  # corners: 3, 63, 66 - either side of a wave -, 255, 258 - of a workgroup -, 3000: twelve workgroups, the last one part full


def test_the_kernel_writes_the_twin_s_records():
    rng = np.random.RandomState(5)
    hosts = []
    for key in range(2):  # two hosts with the same meshes at other vertices and normals: their views are the keys
        host = luminary_amd.Host()
        scenes.apply_benchmark_settings(host, 16, 16, 2, sky=(0.5, 0.5, 0.5))
        mat = host.add_material(scenes._material((0.6, 0.6, 0.6), 0.6))
        for k, n in enumerate(TRIANGLES + [30]):
            t, nrm = soup(rng, n).reshape(n, 9), unit_normals(rng, n)
            if key == 1 and k % 2 == 0:
                nrm = hosts_normals[k]  # every other mesh keeps its normal words between the keys
            host.new_instance(host.add_mesh(t, np.full(n, mat, dtype=np.uint16), normals=nrm), position=(3.0 * k, 0.0, 0.0))
        scenes.set_camera(host, (0.0, 0.0, 40.0), (0.0, 0.0, 0.0))
        hosts_normals = [host.get_mesh(m)[1] for m in range(len(TRIANGLES) + 1)]
        hosts.append(host)
    core = _core()
    try:
        views = [_view(h) for h in hosts]
        keys = [[_mesh_records(v, m, n) for m, n in enumerate(TRIANGLES + [30])] for v in views]
        last = len(TRIANGLES)  # the mesh without keys
        core.upload(views[0])
        with pytest.raises(CoreError):
            core.mesh_shutter_key(0, 1)  # a close key without an open key
        with pytest.raises(CoreError):
            core.mesh_shutter_key(len(TRIANGLES) + 1, 0)  # a mesh the scene does not have
        for m in range(last):
            core.mesh_shutter_key(m, 0)
        core.update(views[1], DIRTY_MESH_POSITIONS)
        for m in range(last):
            core.mesh_shutter_key(m, 1)
        for step, t in enumerate([0.25, 0.0, 0.5, 1.0]):
            core.shutter_time(t)
            core.update(views[1], DIRTY_MESH_SHUTTER)
            for m, n in enumerate(TRIANGLES):
                want, flags = shutter_host(keys[0][m], keys[1][m], t)
                got = core.mesh_vertices_probe(m, n)
                assert flags == 0 and np.array_equal(got, want), "t = %g, %d triangles: %d of %d words differ from the twin's" % (t, n, int((got != want).sum()), got.size)
            assert np.array_equal(core.mesh_vertices_probe(last, 30), keys[1][last]), "a mesh without keys keeps its bytes"
            st = core.shutter_stats()
            assert (st.slices, st.last_meshes, st.last_launches, st.last_bytes_uploaded) == (step + 1, last, last, 0), (st.slices, st.last_meshes, st.last_launches)
            assert core.mesh_refit_stats().seconds_hash == 0.0, "the view's vertices are not read"
        # an update that takes the view's vertex arrays over writes the keyed meshes again at their last time; the view's vertices of them are not trusted
        core.shutter_time(0.5)
        core.update(views[1], DIRTY_MESH_SHUTTER)
        core.update(views[0], DIRTY_MESH_POSITIONS)
        assert np.array_equal(core.mesh_vertices_probe(3, TRIANGLES[3]), shutter_host(keys[0][3], keys[1][3], 0.5)[0]), "written again at the last t"
        assert np.array_equal(core.mesh_vertices_probe(last, 30), keys[0][last]), "the mesh without keys follows the view"
        core.mesh_shutter_drop(3)
        with pytest.raises(CoreError):
            core.mesh_shutter_drop(3)
        with pytest.raises(CoreError):
            core.shutter_time(1.5)
    finally:
        core.close()
        for h in hosts:
            h.close()


# ---- 2. moved vertices through the public calls ----
def test_moved_vertices_render_like_the_reference_loop_and_a_second_call_continues():
    host, store, sharp = _small_zoo(), _small_zoo(), _small_zoo()
    try:
        mesh = _plain_meshes(host, 1)[0]
        p0 = host.get_mesh(mesh)[0]
        moved = bend(p0, 0.3, 0.5)
        rec_a = _mesh_records(_view(store), mesh, len(p0))
        store.set_mesh_positions(mesh, moved)
        rec_b = _mesh_records(_view(store), mesh, len(p0))
        host.shutter_open()
        host.set_mesh_positions(mesh, moved)
        host.render_shutter(SLICES, PER_SLICE, PER_SLICE)
        blurred = _images(host)
        want = _reference_loop(store, mesh, rec_a, rec_b)
        _same_images(blurred, want, "four slices of two ids")
        st = host.shutter_stats()
        assert (st["renders"], st["slices"], st["last_moved_meshes"], st["last_moved_instances"], st["last_camera_moved"]) == (1, SLICES, 1, 0, 0), st
        with _main_core(host) as core:
            assert np.array_equal(core.mesh_vertices_probe(mesh, len(p0)), rec_b), "the devices hold the close key afterwards"
            cs = core.shutter_stats()
            assert (cs.slices, cs.last_meshes, cs.last_launches, cs.last_bytes_uploaded) == (SLICES + 1, 1, 1, 0), (cs.slices, cs.last_meshes, cs.last_launches)
        # both sharp renders differ
        sharp.render_samples(0, SLICES * PER_SLICE, samples_per_pass=PER_SLICE)
        _differ(blurred, _images(sharp), "the open key's sharp image")
        sharp.set_mesh_positions(mesh, moved)
        sharp.render_samples(0, SLICES * PER_SLICE, samples_per_pass=PER_SLICE)
        close_sharp = _images(sharp)
        _differ(blurred, close_sharp, "the close key's sharp image")
        # 7. a second call continues the accumulation with first = 8 (one slice of two ids here: ids 8 and 9 at t = 0.5)
        assert host.is_rendering()[1] == SLICES * PER_SLICE
        host.render_shutter(1, PER_SLICE, PER_SLICE)
        assert host.is_rendering()[1] == SLICES * PER_SLICE + PER_SLICE
        view, core = _view(store), _core()
        try:
            _write_records(view, mesh, rec_a)
            core.upload(view)
            core.set_pixels(None)
            for k in range(SLICES + 1):
                t = _time(k) if k < SLICES else _time(0, 1)
                _write_records(view, mesh, shutter_host(rec_a, rec_b, t)[0])
                core.update(view, DIRTY_MESH_POSITIONS)
                core.render(k * PER_SLICE, PER_SLICE, samples_per_pass=PER_SLICE)
            fm, sm = core.accumulators()
        finally:
            core.close()
        _same_images(_images(host), (np.asarray(fm), np.asarray(sm)), "the second call: ids 8 and 9 into the same accumulators")
        # 8. an edit afterwards restarts the integration: the image of a host that never opened a shutter
        again = bend(p0, 0.2, 1.1)
        for h in (host, sharp):
            h.set_mesh_positions(mesh, again)
            h.render_samples(0, 2, samples_per_pass=2)
        _same_images(_images(host), _images(sharp), "after an edit: a host that never opened a shutter")
        assert host.is_rendering()[1] == 2
    finally:
        host.close(); store.close(); sharp.close()


# ---- 3. keys made by two poses and by two weight sets ----
@pytest.mark.parametrize("kind", ["skin", "morph"])
def test_keys_made_on_the_device_by_a_pose_or_by_weights(kind):
    host, store, core = _small_zoo(), _small_zoo(), _core()
    try:
        mesh = _plain_meshes(host, 1)[0]
        p0, n0 = host.get_mesh(mesh)[:2]
        view = _view(store)
        core.upload(view)
        host.render_samples(0, 2, samples_per_pass=2)  # the scene is on the device before anything is bound (a first upload poses on the host)
        if kind == "skin":
            ids, w = two_bone_weights(p0)
            host.bind_mesh_skin(mesh, ids, w, 2)
            core.mesh_skin_bind(mesh, p0, n0, ids, w, 2)
            shapes = [two_bone_bend(p0, 0.3, 0.0), two_bone_bend(p0, 0.7, 0.1)]
            host_set, core_set = host.set_mesh_pose, core.mesh_skin_pose
        else:
            morph = bulge_targets(p0, 3, 0.15)
            host.bind_mesh_morph(mesh, len(p0), *morph.lists)
            core.mesh_morph_bind(mesh, p0, n0, *morph.lists)
            shapes = [F([0.8, 0.0, -0.4]), F([0.0, 1.3, 0.6])]
            host_set, core_set = host.set_mesh_weights, core.mesh_morph_weights
        keys = []
        for shape in shapes:  # the keys, read back from a context that was posed the same way
            core_set(mesh, shape)
            core.update(view, DIRTY_MESH_SKIN)
            keys.append(core.mesh_vertices_probe(mesh, len(p0)))
        assert not np.array_equal(keys[0], keys[1])
        host_set(mesh, shapes[0])
        host.shutter_open()
        host_set(mesh, shapes[1])
        host.render_shutter(SLICES, PER_SLICE, PER_SLICE)
        _same_images(_images(host), _reference_loop(store, mesh, keys[0], keys[1]), "keys by " + kind)
        assert host.mesh_skin_stats()["host_materialisations"] == 0, "nothing was posed or blended on the host"
        with _main_core(host) as main:
            assert np.array_equal(main.mesh_vertices_probe(mesh, len(p0)), keys[1])
            assert main.shutter_stats().last_bytes_uploaded == 0
    finally:
        core.close(); host.close(); store.close()


# ---- 4. moved instances and a moved camera ----
def _blend(a, b, t):
    a, b = F(a), F(b)
    d = b - a
    s = F(t) * d
    return a + s


def _blend_vec(a, b, t):
    return Vec3(float(_blend(a.x, b.x, t)), float(_blend(a.y, b.y, t)), float(_blend(a.z, b.z, t)))


def test_moved_instances_and_a_moved_camera():
    host, plain = _small_zoo(), _small_zoo()
    core = _core()
    try:
        emits = lambda m: any(host.get_material(int(i)).emission_active for i in set(host.get_mesh(m)[3]))
        ids = [i for i in range(host.get_num_instances()) if not emits(host.get_instance(i).mesh_id)][::2]
        assert ids
        opened = [host.get_instance(i) for i in ids]
        closed = []
        for k, i in enumerate(ids):
            inst = host.get_instance(i)
            inst.position = Vec3(inst.position.x + 0.4, inst.position.y + 0.1 * (k % 3), inst.position.z - 0.3)
            inst.rotation = Vec3(inst.rotation.x + 0.5, inst.rotation.y - 0.35, inst.rotation.z + 0.2)
            if k % 2:
                inst.scale = Vec3(inst.scale.x * 1.25, inst.scale.y * 0.8, inst.scale.z * 1.1)
            closed.append(inst)
        cam_a = host.get_camera()
        cam_b = host.get_camera()
        cam_b.pos = Vec3(cam_a.pos.x + 0.6, cam_a.pos.y + 0.2, cam_a.pos.z - 0.4)
        cam_b.rotation = Vec3(cam_a.rotation.x + 0.05, cam_a.rotation.y - 0.08, cam_a.rotation.z)
        host.shutter_open()
        host.set_instance_transforms(closed)
        host.set_camera(cam_b)
        host.render_shutter(SLICES, PER_SLICE, PER_SLICE)
        st = host.shutter_stats()
        assert (st["last_moved_meshes"], st["last_moved_instances"], st["last_camera_moved"]) == (0, len(ids), 1), st
        # the reference loop: a second, plain host is fed the numpy float32 blend and encodes the views
        core.upload(_view(plain))
        core.set_pixels(None)
        for k in range(SLICES):
            t = _time(k)
            blended = []
            for a, b in zip(opened, closed):
                inst = plain.get_instance(a.id)
                inst.position, inst.rotation, inst.scale = _blend_vec(a.position, b.position, t), _blend_vec(a.rotation, b.rotation, t), _blend_vec(a.scale, b.scale, t)
                blended.append(inst)
            plain.set_instance_transforms(blended)
            cam = plain.get_camera()
            cam.pos, cam.rotation = _blend_vec(cam_a.pos, cam_b.pos, t), _blend_vec(cam_a.rotation, cam_b.rotation, t)
            plain.set_camera(cam)
            core.update(_view(plain), DIRTY_INSTANCE_TRANSFORMS | DIRTY_CONSTANTS)
            core.render(k * PER_SLICE, PER_SLICE, samples_per_pass=PER_SLICE)
        fm, sm = core.accumulators()
        _same_images(_images(host), (np.asarray(fm), np.asarray(sm)), "moved instances and camera")
        # afterwards the host's scene and its view hold the close key
        host2 = _small_zoo()
        try:
            host2.set_instance_transforms(closed)
            host2.set_camera(cam_b)
            a, b = oracle_lib.view_arrays(host.device_scene()), oracle_lib.view_arrays(host2.device_scene())
            for name in ("instance_transforms", "vertices"):
                assert np.array_equal(a[name], b[name]), "the host's view holds the close key: " + name
        finally:
            host2.close()
    finally:
        core.close(); host.close(); plain.close()


# ---- 5. and 6. a moving emitter with the light refit on; what the call leaves on the device ----
def test_a_moving_emitter_refits_the_lights_per_slice_and_leaves_the_close_key_s_arrays():
    host, store, sharp = _small_zoo(), _small_zoo(), _small_zoo()
    try:
        for h in (host, sharp):
            h.set_light_refit(1)
            luminary_amd._lib().luminary_ext_set_mesh_refit_in_place(h._h, C.c_uint32(1))
        lamp = _emissive_mesh(host)
        p0 = host.get_mesh(lamp)[0]
        moved = bend(p0, 0.25, 0.7)
        built = Built(store)
        open_view = _view(store)
        rec_a = _mesh_records(open_view, lamp, len(p0))
        all_records = np.asarray(oracle_lib.view_arrays(open_view)["vertices"]).reshape(-1, 4).astype(U).copy()
        first = 3 * _first_triangle(open_view, lamp)
        store.set_mesh_positions(lamp, moved)
        rec_b = _mesh_records(_view(store), lamp, len(p0))
        store.set_mesh_positions(lamp, p0, host.get_mesh(lamp)[1])  # the store's light arrays are those of the open key again

        def light_arrays_of(view):
            records = all_records.copy()
            records[first:first + 3 * len(p0)] = _mesh_records(view, lamp, len(p0))
            out = built.refit(records.view(F))
            assert out["report"].refitted == 1
            return with_light_arrays(view, out["root"], out["nodes"], built.arrays["handles"], out["light_bvh_tris"])

        host.shutter_open()
        host.set_mesh_positions(lamp, moved)
        host.render_shutter(SLICES, PER_SLICE, PER_SLICE)
        _same_images(_images(host), _reference_loop(store, lamp, rec_a, rec_b, light_arrays_of=light_arrays_of), "a moving emitter")
        st = host.light_refit_stats()
        assert st["fallbacks"] == 0 and st["host_rebuilds"] == 0 and st["refits"] >= SLICES + 1, st
        # 6. vertex array, the node array's mesh part and the light arrays: those of a host that made the same edit and rendered without a shutter
        sharp.render_samples(0, 2, samples_per_pass=2)
        sharp.set_mesh_positions(lamp, moved)
        sharp.render_samples(0, 2, samples_per_pass=2)
        with _main_core(host) as a, _main_core(sharp) as b:
            for m in range(host.get_num_meshes()):
                n = len(host.get_mesh(m)[3])
                assert np.array_equal(a.mesh_vertices_probe(m, n), b.mesh_vertices_probe(m, n)), "vertices of mesh %d" % m
            assert np.array_equal(a.resident_mesh_nodes_probe(), b.resident_mesh_nodes_probe()), "the node array's mesh part"
            la, lb = a.light_arrays_probe(), b.light_arrays_probe()
            for k in lb:
                assert np.array_equal(la[k].view(np.uint8), lb[k].view(np.uint8)), "light arrays: " + k
    finally:
        host.close(); store.close(); sharp.close()


# ---- 9. two device slots ----
def test_two_device_slots_give_the_accumulators_of_one(monkeypatch):
    images = []
    for slots in (1, 2):
        if slots > 1:
            monkeypatch.setenv("LUM_FAKE_DEVICES", str(slots))
            monkeypatch.setenv("LUM_MAX_DEVICES", "8")
        host = _small_zoo()
        try:
            assert host.get_device_count() == slots
            for d in range(1, slots):
                host.set_device_enable(d, True)
            mesh = _plain_meshes(host, 1)[0]
            host.shutter_open()
            host.set_mesh_positions(mesh, bend(host.get_mesh(mesh)[0], 0.3, 0.5))
            host.render_shutter(SLICES, PER_SLICE, PER_SLICE)
            images.append(_images(host))
        finally:
            host.close()
    _same_images(images[1], images[0], "two slots against one")


# ---- 10. one slice with equal keys ----
def test_one_slice_where_nothing_moved_is_render_samples():
    host, plain = _small_zoo(), _small_zoo()
    try:
        host.shutter_open()
        host.render_shutter(1, 4, 2)
        plain.render_samples(0, 4, samples_per_pass=2)
        _same_images(_images(host), _images(plain), "nothing moved")
        with _main_core(host) as core:
            assert core.shutter_stats().slices == 0, "no mesh holds keys: nothing was written"
        host.shutter_open()
        host.render_samples(4, 2, samples_per_pass=2)  # any other render call ends the shutter
        with pytest.raises(luminary_amd.LuminaryError):
            host.render_shutter(1, 2, 2)
    finally:
        host.close(); plain.close()
