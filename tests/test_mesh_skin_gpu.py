"""Skinned meshes on the device: lumc_mesh_skin_bind / lumc_mesh_skin_pose -> LUMC_DIRTY_MESH_SKIN -> csrc/host/mesh_deform.hip k_deform_mesh, scene_device.hip skin_meshes.

The kernel's vertex records are held to the host twin's (lumc_skin_host; tests/test_mesh_skin.py holds that to the definition) byte for byte, the packed normal word
included; what the update leaves in the node array to a second context that was given the same vertices through LUMC_DIRTY_MESH_POSITIONS; what is rendered over it
to the CPU oracle on the view of a host that was given those vertices, bit for bit."""
import numpy as np
import pytest

import oracle_lib
from luminary_amd import Host, scenes
from luminary_amd.core import DIRTY_INSTANCE_TRANSFORMS, DIRTY_LIGHTS, DIRTY_MESH_POSITIONS, DIRTY_MESH_SKIN, Core, CoreError, skin_host
from test_instance_transforms_api import moved_instances
from test_instance_update_gpu import _against_oracle, _same, _zoo
from test_mesh_positions_api import bend
from test_mesh_refit import soup
from test_mesh_skin import random_bones, random_skin, two_bone_bend, two_bone_weights, unit_normals
from test_resident_refit_gpu import _counts, _emissive_mesh, _same_layout

pytestmark = pytest.mark.gpu
F = np.float32
MOVED = DIRTY_INSTANCE_TRANSFORMS | DIRTY_LIGHTS


def _small_zoo():
    return _zoo(48, 32, 3)


def _view(host):
    return oracle_lib.with_luts(host.device_scene())


def _core(in_place=0, flavour="exact"):
    core = Core(0)
    core.set_flavour(flavour)
    core.set_mesh_refit_in_place(in_place)
    return core


def _records(positions, packed):
    """The device's vertex records [3 n, 4] words of the twin's positions [n, 9] and packed normals [n, 3]."""
    out = np.zeros((3 * len(positions), 4), np.uint32)
    out[:, :3] = np.ascontiguousarray(positions, dtype=F).reshape(-1, 3).view(np.uint32)
    out[:, 3] = np.asarray(packed, dtype=np.uint32).reshape(-1)
    return out


def _plain_meshes(host, count):
    """Meshes without an emissive triangle, largest first."""
    emits = lambda m: any(host.get_material(int(i)).emission_active for i in set(host.get_mesh(m)[3]))
    plain = sorted((m for m in range(host.get_num_meshes()) if len(host.get_mesh(m)[3]) >= 8 and not emits(m)), key=lambda m: -len(host.get_mesh(m)[3]))
    assert len(plain) >= count
    return plain[:count]


class Skinned:
    """A mesh of `host` bound on `core`, with a twin host that is given every pose's vertices through set_mesh_positions."""

    def __init__(self, core, host, twin, mesh):
        self.core, self.twin, self.mesh = core, twin, mesh
        self.rest_p, self.rest_n = host.get_mesh(mesh)[:2]
        self.ids, self.w = two_bone_weights(self.rest_p)
        core.mesh_skin_bind(mesh, self.rest_p, self.rest_n, self.ids, self.w, 2)

    def pose(self, angle, lift=0.0):
        bones = two_bone_bend(self.rest_p, angle, lift)
        self.core.mesh_skin_pose(self.mesh, bones)
        p, n, packed = skin_host(self.rest_p, self.rest_n, self.ids, self.w, bones)
        self.twin.set_mesh_positions(self.mesh, p, n)
        self.want = _records(p, packed)
        return p

    def check(self, where):
        got = self.core.mesh_vertices_probe(self.mesh, len(self.rest_p))
        assert np.array_equal(got, self.want), "%s: %d of %d words of mesh %d's vertices differ from the twin's" % (where, int((got != self.want).sum()), got.size, self.mesh)


# ---- fails without the feature ----
def test_a_pose_moves_the_vertices_on_the_device_and_renders_like_the_oracle():
    host, twin, core = _small_zoo(), _small_zoo(), _core()
    try:
        stale = _view(host)
        core.upload(stale)
        before = _against_oracle(core, stale, "before the pose")
        mesh = _plain_meshes(host, 1)[0]
        skinned = Skinned(core, host, twin, mesh)
        skinned.pose(0.6, 0.3)
        core.update(stale, DIRTY_MESH_SKIN)  # (the view still holds the rest pose: not read)
        view = _view(twin)
        n = len(skinned.rest_p)
        assert np.array_equal(skinned.want.reshape(-1), oracle_lib.view_arrays(view)["vertices"].reshape(-1, 4)[3 * _first_triangle(view, mesh):][:3 * n].reshape(-1)), \
            "the twin host's view holds the twin's records"
        skinned.check("one pose")
        stats, refit = core.mesh_skin_stats(), core.mesh_refit_stats()
        print("%d corners: %.3f ms: palette %.3f, kernel and flags %.3f; %d bytes up" % (3 * n, 1e3 * stats.seconds, 1e3 * stats.seconds_upload, 1e3 * stats.seconds_skin, stats.last_bytes_uploaded))
        assert (stats.poses, stats.last_meshes, stats.last_launches, stats.rebuild_downloads) == (1, 1, 1, 0)
        assert stats.last_bytes_uploaded < 48 * 2 + 256
        assert refit.seconds_hash == 0.0 and (refit.last_refits, refit.last_rebuilds) == (1, 0)
        after = _against_oracle(core, view, "posed")
        assert int((after != before).sum()) > 20, "the pose must change the image"
        # a second update without a new pose does nothing to the meshes
        core.update(stale, DIRTY_MESH_SKIN)
        assert core.mesh_skin_stats().poses == 1
        skinned.check("no new pose")
        _against_oracle(core, view, "no new pose")
    finally:
        core.close(); host.close(); twin.close()


def _first_triangle(view, mesh):
    return int(oracle_lib.view_arrays(view)["mesh_tri_offset"][mesh])


# ---- sizes at which the kernel can go wrong ----
SOUPS = [1, 21, 22, 85, 86, 171, 87382]  # corners: 3, 63, 66 (a wave), 255, 258 (a workgroup), 513 (two workgroups and one), 262146 (the whole grid once, and two)


def test_soups_on_either_side_of_a_wave_a_workgroup_and_the_grid():
    rng = np.random.RandomState(5)
    host = Host()
    scenes.apply_benchmark_settings(host, 16, 16, 2, sky=(0.5, 0.5, 0.5))
    mat = host.add_material(scenes._material((0.6, 0.6, 0.6), 0.6))
    core = _core()
    try:
        soups = [soup(rng, n).reshape(n, 9) for n in SOUPS]
        normals = [unit_normals(rng, n) for n in SOUPS]
        for k, (tris, nrm) in enumerate(zip(soups, normals)):
            host.new_instance(host.add_mesh(tris, np.full(len(tris), mat, dtype=np.uint16), normals=nrm), position=(3.0 * k, 0.0, 0.0))
        scenes.set_camera(host, (0.0, 0.0, 40.0), (0.0, 0.0, 0.0))
        view = _view(host)
        core.upload(view)
        for bone_count in (1, 1024, 3):
            want = []
            for m, (tris, nrm) in enumerate(zip(soups, normals)):
                ids, w = random_skin(rng, len(tris), bone_count)
                assert int(ids.max()) == bone_count - 1, "the last bone is named"
                bones = random_bones(rng, bone_count, scale=True)
                core.mesh_skin_bind(m, tris, nrm, ids, w, bone_count)
                core.mesh_skin_pose(m, bones)
                p, _, packed = skin_host(tris, nrm, ids, w, bones)
                want.append(_records(p, packed))
            core.update(view, DIRTY_MESH_SKIN)
            stats = core.mesh_skin_stats()
            assert (stats.last_meshes, stats.last_launches, stats.last_bytes_uploaded) == (len(SOUPS), len(SOUPS), 48 * bone_count * len(SOUPS))
            for m, records in enumerate(want):
                got = core.mesh_vertices_probe(m, SOUPS[m])
                assert np.array_equal(got, records), "%d bones, %d triangles: %d of %d words differ, first in corner %d" % (
                    bone_count, SOUPS[m], int((got != records).sum()), got.size, int(np.nonzero((got != records).any(axis=1))[0][0]))
            assert core.mesh_refit_stats().last_refits == len(SOUPS)
        tris, nrm = soups[2], normals[2]
        ids, w = random_skin(rng, len(tris), 1024)
        with pytest.raises(CoreError, match="bone_count is 1 ... 1024"):
            core.mesh_skin_bind(2, tris, nrm, ids, w, 1025)
        with pytest.raises(CoreError, match="bone_count is 1 ... 1024"):
            core.mesh_skin_bind(2, tris, nrm, ids, w, 0)
        with pytest.raises(CoreError, match="bone id"):
            core.mesh_skin_bind(2, tris, nrm, ids, w, 1023)
        with pytest.raises(CoreError, match="triangle count"):
            core.mesh_skin_bind(3, tris, nrm, ids, w, 1024)
        with pytest.raises(CoreError, match="another bone count"):
            core.mesh_skin_pose(2, np.zeros((4, 12), F))
        with pytest.raises(CoreError, match="not finite"):
            core.mesh_skin_pose(2, np.full((3, 12), np.nan, F))
        core.mesh_skin_unbind(2)
        with pytest.raises(CoreError, match="not bound"):
            core.mesh_skin_pose(2, np.zeros((3, 12), F))
    finally:
        core.close(); host.close()


# ---- in place ----
def test_three_poses_in_the_resident_array_leave_the_bytes_of_the_host_route():
    host, twin = _small_zoo(), _small_zoo()
    a, b = _core(1), _core(1)
    try:
        first = _view(host)
        a.upload(first); b.upload(first)  # (the shared tree cache gives both contexts one topology)
        for h in (host, twin):
            h.set_instance_transforms(moved_instances(h, 0))
        a.update(_view(host), MOVED); b.update(_view(twin), MOVED)
        m0, m1 = _plain_meshes(host, 2)
        skins = [Skinned(a, host, twin, m0), Skinned(a, host, twin, m1)]
        for k, (angle, lift) in enumerate([(0.3, 0.0), (0.7, 0.2), (-0.4, 0.1)]):
            for s in skins:
                s.pose(angle * (1.0 if s.mesh == m0 else -0.8), lift)
            for h in (host, twin):
                h.set_instance_transforms(moved_instances(h, k + 1))
            a.update(_view(host), DIRTY_MESH_SKIN | MOVED)  # (host's vertices stay at the rest pose throughout)
            view = _view(twin)
            b.update(view, DIRTY_MESH_POSITIONS | MOVED)
            where = "pose %d" % k
            for s in skins:
                s.check(where)
            assert _counts(a) == {"relayouts": 1, "instance fallbacks": 0, "updates": k + 1, "fallbacks": 0}, (where, _counts(a))
            assert _counts(b) == {"relayouts": 1, "instance fallbacks": 0, "updates": k + 1, "fallbacks": 0}, (where, _counts(b))
            ra, rb = a.mesh_refit_stats(), b.mesh_refit_stats()
            assert (ra.last_refits, ra.last_rebuilds) == (rb.last_refits, rb.last_rebuilds) == (2, 0) and ra.seconds_hash == 0.0 and rb.seconds_hash > 0.0, where
            assert a.mesh_skin_stats().last_bytes_uploaded == 2 * 96
            _same_layout(a, b, host, where)
            _against_oracle(a, view, where, {"the host route": b})
    finally:
        a.close(); b.close(); host.close(); twin.close()


# ---- one mesh by the host route, one by a pose ----
@pytest.mark.parametrize("in_place", [0, 1])
def test_a_mixed_update_and_a_later_upload_with_stale_vertices(in_place):
    host, twin, core = _small_zoo(), _small_zoo(), _core(in_place)
    try:
        core.upload(_view(host))
        ma, mb = _plain_meshes(host, 2)
        skinned = Skinned(core, host, twin, mb)
        pa = host.get_mesh(ma)[0]
        skinned.pose(0.5, 0.2)
        for h in (host, twin):
            h.set_mesh_positions(ma, bend(pa, 0.2, 0.4))
        core.update(_view(host), DIRTY_MESH_POSITIONS | DIRTY_MESH_SKIN | DIRTY_LIGHTS)  # (host's view: mesh a moved, mesh b at rest)
        refit = core.mesh_refit_stats()
        assert (refit.last_refits, refit.last_rebuilds) == (2, 0)
        assert core.mesh_skin_stats().last_meshes == 1
        skinned.check("mixed update")
        _against_oracle(core, _view(twin), "mixed update")
        # mesh a again, by the host route alone: the upload brings mesh b's rest pose, the last palette puts the pose back before anything reads it
        for h in (host, twin):
            h.set_mesh_positions(ma, bend(pa, 0.25, 1.3))
        stale = _view(host)
        rest = oracle_lib.view_arrays(stale)["vertices"].reshape(-1, 4)[3 * _first_triangle(stale, mb):][:len(skinned.want)]
        assert not np.array_equal(rest, skinned.want), "the view's vertices of the posed mesh are stale on purpose"
        core.update(stale, DIRTY_MESH_POSITIONS | DIRTY_LIGHTS)
        refit, stats = core.mesh_refit_stats(), core.mesh_skin_stats()
        assert (refit.last_refits, refit.last_rebuilds) == (1, 0), "the posed mesh holds the same bits: its tree still fits"
        assert (stats.poses, stats.last_meshes, stats.last_launches, stats.last_bytes_uploaded) == (1, 0, 1, 0)
        skinned.check("after the upload")
        _against_oracle(core, _view(twin), "after the upload")
        # unbound: the view is trusted again, and a host-route update of the same mesh refits it
        core.mesh_skin_unbind(mb)
        moved = bend(host.get_mesh(mb)[0], 0.2, 0.9)
        for h in (host, twin):
            h.set_mesh_positions(mb, moved)
        core.update(_view(host), DIRTY_MESH_POSITIONS | DIRTY_LIGHTS)
        assert core.mesh_refit_stats().last_refits == 1
        _against_oracle(core, _view(twin), "unbound, moved by the host route")
    finally:
        core.close(); host.close(); twin.close()


# ---- rebuild ----
def test_a_rebuild_downloads_the_posed_vertices():
    host, twin, core = _small_zoo(), _small_zoo(), _core()
    try:
        stale = _view(host)
        core.upload(stale)
        skinned = Skinned(core, host, twin, _plain_meshes(host, 1)[0])
        core.set_mesh_refit(1, 0.0)
        skinned.pose(0.4)
        core.update(stale, DIRTY_MESH_SKIN)
        refit = core.mesh_refit_stats()
        assert (refit.last_refits, refit.last_rebuilds) == (0, 1) and core.mesh_skin_stats().rebuild_downloads == 1
        skinned.check("mode 1")
        _against_oracle(core, _view(twin), "mode 1")
        core.set_mesh_refit(0, 1.0 + 1e-6)
        skinned.pose(1.4, 0.5)
        core.update(stale, DIRTY_MESH_SKIN)
        refit = core.mesh_refit_stats()
        assert refit.max_cost_growth > 1.0 + 1e-6, "the pose must grow the cost beyond the threshold"
        assert (refit.last_refits, refit.last_rebuilds) == (0, 1) and core.mesh_skin_stats().rebuild_downloads == 2
        skinned.check("beyond max_cost_growth")
        _against_oracle(core, _view(twin), "beyond max_cost_growth")
    finally:
        core.close(); host.close(); twin.close()


# ---- a fallback in the middle of an in-place update that carries a pose ----
def test_a_fallback_in_the_middle_of_an_in_place_update_skins_once():
    """The pose grows its mesh's cost beyond the threshold after the in-place path has refitted both meshes where the nodes live: the update goes on by the
    other path, from the vertices the one skinning launch wrote. The counter literals are what the commit before the one-front-end refactor gave for this test."""
    host, twin, core = _small_zoo(), _small_zoo(), _core(in_place=1)
    try:
        core.upload(_view(host))
        ma, mb = _plain_meshes(host, 2)
        skinned = Skinned(core, host, twin, mb)
        pa = host.get_mesh(ma)[0]
        core.set_mesh_refit(0, 1.0 + 1e-6)
        skinned.pose(1.4, 0.5)
        for h in (host, twin):
            h.set_mesh_positions(ma, bend(pa, 0.2, 0.4))
        before, downloads = _counts(core), core.mesh_skin_stats().rebuild_downloads
        core.update(_view(host), DIRTY_MESH_POSITIONS | DIRTY_MESH_SKIN | DIRTY_LIGHTS)  # (host's view: mesh a moved, mesh b at rest)
        stats, refit, after = core.mesh_skin_stats(), core.mesh_refit_stats(), _counts(core)
        print("fallback: poses %d, last_meshes %d, last_launches %d; refits %d, rebuilds %d, downloads %d, growth %.6f; %s -> %s" % (
            stats.poses, stats.last_meshes, stats.last_launches, refit.last_refits, refit.last_rebuilds, stats.rebuild_downloads - downloads, refit.max_cost_growth, before, after))
        assert (stats.poses, stats.last_meshes, stats.last_launches) == (1, 1, 1), "skinning ran once across the fallback"
        assert after["fallbacks"] == before["fallbacks"] + 1 and after["updates"] == before["updates"]
        assert refit.max_cost_growth > 1.0 + 1e-6, "the pose must grow the cost beyond the threshold"
        assert (refit.last_refits, refit.last_rebuilds) == (0, 2) and stats.rebuild_downloads - downloads == 1, "the bend grows mesh a's cost too: both are built again, the posed one from a download"
        skinned.check("fallback")
        _against_oracle(core, _view(twin), "fallback")
        # a mild update without a threshold runs in place again, in a layout of its own
        core.set_mesh_refit(0, 0.0)
        skinned.pose(0.3, 0.1)
        before = after
        core.update(_view(host), DIRTY_MESH_SKIN | DIRTY_LIGHTS)
        after = _counts(core)
        print("in place again: %s -> %s" % (before, after))
        assert after == {"relayouts": before["relayouts"] + 1, "instance fallbacks": before["instance fallbacks"], "updates": before["updates"] + 1, "fallbacks": before["fallbacks"]}
        assert core.mesh_skin_stats().poses == 2
        skinned.check("in place again")
        _against_oracle(core, _view(twin), "in place again")
    finally:
        core.close(); host.close(); twin.close()


# ---- lights ----
def test_a_posed_emitter_with_its_light_arrays():
    host, twin, core = _small_zoo(), _small_zoo(), _core()
    try:
        core.upload(_view(host))
        skinned = Skinned(core, host, twin, _emissive_mesh(host))
        skinned.pose(0.5, 0.3)
        view = _view(twin)  # (the light tree and the light BVH's triangles of the posed emitter; its vertices are not taken from here)
        core.update(view, DIRTY_MESH_SKIN | DIRTY_LIGHTS)
        skinned.check("emitter")
        assert core.mesh_skin_stats().last_bytes_uploaded == 96
        _against_oracle(core, view, "emitter")
    finally:
        core.close(); host.close(); twin.close()


# ---- a palette that overflows ----
def test_an_overflowing_palette_is_an_error_that_names_the_mesh():
    host, core = _small_zoo(), _core()
    try:
        view = _view(host)
        core.upload(view)
        mesh = _plain_meshes(host, 1)[0]
        rest_p, rest_n = host.get_mesh(mesh)[:2]
        ids, w = two_bone_weights(rest_p)
        core.mesh_skin_bind(mesh, rest_p, rest_n, ids, w, 2)
        bones = two_bone_bend(rest_p, 0.3)
        bones[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] *= F(3e38)  # scale 3e38: every entry finite ...
        bones[1, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = F(3e38)     # ... and a row's sum overflows wherever x + y + z passes 1.14
        assert np.isfinite(bones).all() and not np.isfinite(skin_host(rest_p, rest_n, ids, w, bones)[0]).all(), "the twin must see the overflow too"
        core.mesh_skin_pose(mesh, bones)
        with pytest.raises(CoreError, match="mesh %d: the pose gives a position that is not finite" % mesh):
            core.update(view, DIRTY_MESH_SKIN)
        with pytest.raises(CoreError):
            core.mesh_vertices_probe(mesh, len(rest_p))  # the scene is gone, as after any failed partial update
        core.upload(view)
        _against_oracle(core, view, "a fresh upload after the failed update")
    finally:
        core.close(); host.close()


# ---- the other flavour ----
def test_the_fast_flavour_holds_the_same_vertex_bytes():
    host, twin, core = _small_zoo(), _small_zoo(), _core(flavour="fast")
    try:
        stale = _view(host)
        core.upload(stale)
        skinned = Skinned(core, host, twin, _plain_meshes(host, 1)[0])
        skinned.pose(0.6, 0.3)
        core.update(stale, DIRTY_MESH_SKIN)
        assert core.flavour == "fast"
        skinned.check("fast flavour")
    finally:
        core.close(); host.close(); twin.close()


# ---- the host API ----
@pytest.mark.parametrize("slots", [1, 2])
def test_the_host_api_end_to_end(slots, monkeypatch):
    if slots > 1:
        monkeypatch.setenv("LUM_FAKE_DEVICES", str(slots))
        monkeypatch.setenv("LUM_MAX_DEVICES", "8")
    host = _small_zoo()
    try:
        assert host.get_device_count() == slots
        host.render_samples(0, 2, samples_per_pass=2)
        mesh = _plain_meshes(host, 1)[0]
        rest_p, rest_n = host.get_mesh(mesh)[:2]
        ids, w = two_bone_weights(rest_p)
        host.bind_mesh_skin(mesh, ids, w, 2)
        assert host.is_rendering()[1] == 2, "a binding moves nothing"
        images = []
        for step, angle in enumerate((0.5, -0.4)):
            bones = two_bone_bend(rest_p, angle, 0.2)
            host.set_mesh_pose(mesh, bones)
            assert host.is_rendering()[1] == 0, "the integration did not restart"
            host.render_samples(0, 2, samples_per_pass=2)
            fm, sm = host.accumulators()
            stats = host.mesh_skin_stats()
            assert stats["host_materialisations"] == step, "the render path does not pose on the host"
            assert (stats["poses"], stats["last_meshes"], stats["last_bytes_uploaded"]) == (step + 1, 1, 96), stats
            assert host.mesh_refit_stats()["seconds_hash"] == 0.0
            ofm, osm, _ = oracle_lib.render(_view(host), 0, 2)  # (the public view: posed on the host for it)
            _same(fm, ofm, "%d slots, pose %d: first moment vs oracle" % (slots, step))
            _same(sm, osm, "%d slots, pose %d: second moment vs oracle" % (slots, step))
            want_p, want_n, _ = skin_host(rest_p, rest_n, ids, w, bones)
            got = host.get_mesh(mesh)
            assert got[0].tobytes() == want_p.tobytes() and got[1].tobytes() == want_n.tobytes()
            assert host.mesh_skin_stats()["host_materialisations"] == step + 1
            assert host.is_rendering()[1] == 2, "reading the scene restarts nothing"
            images.append(fm)
        assert not np.array_equal(images[0], images[1])
        host.unbind_mesh_skin(mesh)
        assert host.get_mesh(mesh)[0].tobytes() == want_p.tobytes()
        host.set_mesh_positions(mesh, bend(want_p, 0.2, 0.6))
        host.render_samples(0, 2, samples_per_pass=2)
        fm, sm = host.accumulators()
        ofm, osm, _ = oracle_lib.render(_view(host), 0, 2)
        _same(fm, ofm, "%d slots, unbound and moved by the host route: first moment vs oracle" % slots)
        _same(sm, osm, "%d slots, unbound and moved by the host route: second moment vs oracle" % slots)
    finally:
        host.close()
