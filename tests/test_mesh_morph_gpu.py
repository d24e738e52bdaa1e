"""Morph targets on the device: lumc_mesh_morph_bind / lumc_mesh_morph_weights -> LUMC_DIRTY_MESH_SKIN -> csrc/host/mesh_deform.hip k_deform_mesh, scene_device.hip
skin_meshes.

The kernel's vertex records are held to the host twin's (lumc_morph_host; tests/test_mesh_morph.py holds that to the definition) byte for byte, the packed normal word
included, alone and together with a skin; what the update leaves in the node array to a second context that was given the same vertices through
LUMC_DIRTY_MESH_POSITIONS; what is rendered over it to the CPU oracle on the view of a host that was given those vertices, bit for bit."""
import numpy as np
import pytest

import oracle_lib
from luminary_amd import Host, scenes
from luminary_amd.core import DIRTY_LIGHTS, DIRTY_MESH_POSITIONS, DIRTY_MESH_SKIN, CoreError, morph_host, skin_host
from test_instance_transforms_api import moved_instances
from test_instance_update_gpu import _against_oracle, _same
from test_mesh_morph import bulge_targets, random_morph, random_weights
from test_mesh_positions_api import bend
from test_mesh_refit import soup
from test_mesh_skin import random_bones, random_skin, two_bone_bend, two_bone_weights, unit_normals
from test_mesh_skin_gpu import MOVED, SOUPS, _core, _first_triangle, _plain_meshes, _records, _small_zoo, _view
from test_resident_refit_gpu import _counts, _emissive_mesh, _same_layout

pytestmark = pytest.mark.gpu
F = np.float32
WEIGHTS = [F([0.8, 0.0, -0.4]), F([0.0, 1.3, 0.6]), F([-0.5, 0.25, 1.0])]


class Morphed:
    """A mesh of `host` bound to three bulges on `core` - and, with `skin`, to the two-bone bend -, with a twin host that is given every shape's vertices through
    set_mesh_positions."""

    def __init__(self, core, host, twin, mesh, skin=False, strength=0.15):
        self.core, self.twin, self.mesh = core, twin, mesh
        self.base_p, self.base_n = host.get_mesh(mesh)[:2]
        self.morph = bulge_targets(self.base_p, 3, strength)
        self.w, self.bones = np.zeros(3, F), None
        core.mesh_morph_bind(mesh, self.base_p, self.base_n, *self.morph.lists)
        self.ids, self.sw = two_bone_weights(self.base_p) if skin else (None, None)
        if skin:
            core.mesh_skin_bind(mesh, self.base_p, self.base_n, self.ids, self.sw, 2)

    def _shape(self):
        p, n, packed = morph_host(self.base_p, self.base_n, *self.morph.lists, self.w, self.ids, self.sw, self.bones)
        self.twin.set_mesh_positions(self.mesh, p, n)
        self.want = _records(p, packed)
        return p

    def weights(self, w):
        self.w = F(w)
        self.core.mesh_morph_weights(self.mesh, self.w)
        return self._shape()

    def pose(self, angle, lift=0.0):
        self.bones = two_bone_bend(self.base_p, angle, lift)
        self.core.mesh_skin_pose(self.mesh, self.bones)
        return self._shape()

    def check(self, where):
        got = self.core.mesh_vertices_probe(self.mesh, len(self.base_p))
        assert np.array_equal(got, self.want), "%s: %d of %d words of mesh %d's vertices differ from the twin's" % (where, int((got != self.want).sum()), got.size, self.mesh)


# ---- fails without the feature ----
def test_weights_move_the_vertices_on_the_device_and_render_like_the_oracle():
    host, twin, core = _small_zoo(), _small_zoo(), _core()
    try:
        stale = _view(host)
        core.upload(stale)
        before = _against_oracle(core, stale, "before the weights")
        mesh = _plain_meshes(host, 1)[0]
        morphed = Morphed(core, host, twin, mesh)
        morphed.weights(WEIGHTS[0])
        core.update(stale, DIRTY_MESH_SKIN)  # (the view still holds the base shape: not read)
        view = _view(twin)
        n = len(morphed.base_p)
        assert np.array_equal(morphed.want.reshape(-1), oracle_lib.view_arrays(view)["vertices"].reshape(-1, 4)[3 * _first_triangle(view, mesh):][:3 * n].reshape(-1)), \
            "the twin host's view holds the twin's records"
        morphed.check("one weight set")
        stats, skin, refit = core.mesh_morph_stats(), core.mesh_skin_stats(), core.mesh_refit_stats()
        print("%d corners, %d entries: %.3f ms: weights %.3f, kernel and flags %.3f; %d bytes up" % (
            3 * n, len(morphed.morph.corners), 1e3 * stats.seconds, 1e3 * stats.seconds_upload, 1e3 * stats.seconds_morph, stats.last_bytes_uploaded))
        assert (stats.applied, stats.last_meshes, stats.last_launches, stats.rebuild_downloads, stats.last_bytes_uploaded) == (1, 1, 1, 0, 4 * 3)
        assert (skin.poses, skin.last_launches, skin.last_bytes_uploaded) == (0, 0, 0), "nothing was skinned"
        assert refit.seconds_hash == 0.0 and (refit.last_refits, refit.last_rebuilds) == (1, 0)
        after = _against_oracle(core, view, "morphed")
        assert int((after != before).sum()) > 20, "the weights must change the image"
        # a second update without new weights does nothing to the meshes
        core.update(stale, DIRTY_MESH_SKIN)
        assert core.mesh_morph_stats().applied == 1
        morphed.check("no new weights")
        _against_oracle(core, view, "no new weights")
        # all weights zero: the base records' bytes, which the view of the untouched host holds
        morphed.weights(np.zeros(3, F))
        core.update(stale, DIRTY_MESH_SKIN)
        got = core.mesh_vertices_probe(mesh, n)
        assert np.array_equal(got.reshape(-1), oracle_lib.view_arrays(stale)["vertices"].reshape(-1, 4)[3 * _first_triangle(stale, mesh):][:3 * n].reshape(-1)), \
            "all weights zero must leave the base records"
        _same(_against_oracle(core, stale, "all weights zero"), before, "all weights zero: the image before the weights")
    finally:
        core.close(); host.close(); twin.close()


# ---- sizes at which the kernel can go wrong ----
# SOUPS (tests/test_mesh_skin_gpu.py): 3, 63, 66 corners (a wave), 255, 258 (a workgroup), 513 (two workgroups and one), 262146 (the whole grid once, and two
# corners): k_deform_mesh has one block (256) and one grid cap (1024) for all three of its forms, so the sizes are its sizes.
@pytest.fixture(scope="module")
def soups():
    rng = np.random.RandomState(5)
    host = Host()
    scenes.apply_benchmark_settings(host, 16, 16, 2, sky=(0.5, 0.5, 0.5))
    mat = host.add_material(scenes._material((0.6, 0.6, 0.6), 0.6))
    tris = [soup(rng, n).reshape(n, 9) for n in SOUPS]
    normals = [unit_normals(rng, n) for n in SOUPS]
    for k, (t, nrm) in enumerate(zip(tris, normals)):
        host.new_instance(host.add_mesh(t, np.full(len(t), mat, dtype=np.uint16), normals=nrm), position=(3.0 * k, 0.0, 0.0))
    scenes.set_camera(host, (0.0, 0.0, 40.0), (0.0, 0.0, 0.0))
    yield host, _view(host), tris, normals
    host.close()


@pytest.mark.parametrize("with_skin", [False, True], ids=["morph alone", "with a 1024-bone skin"])
@pytest.mark.parametrize("target_count", [1, 3, 1024])
def test_soups_on_either_side_of_a_wave_a_workgroup_and_the_grid(soups, target_count, with_skin):
    host, view, tris, normals = soups
    rng = np.random.RandomState(100 + target_count)
    core = _core()
    try:
        core.upload(view)
        want = []
        for m, (t, nrm) in enumerate(zip(tris, normals)):
            morph = random_morph(rng, len(t), target_count)
            assert int(morph.offsets[-1]) > int(morph.offsets[-2]), "the last target is named"
            rows = np.bincount(morph.corners, minlength=3 * len(t))
            assert rows[0] == target_count and rows[1] == 1 and rows[2] == 0, "the three row shapes"
            w = random_weights(rng, target_count)
            core.mesh_morph_bind(m, t, nrm, *morph.lists)
            core.mesh_morph_weights(m, w)
            ids = sw = bones = None
            if with_skin:  # 4 KB of weights (at 1024 targets) and 48 KB of palette in LDS
                ids, sw = random_skin(rng, len(t), 1024)
                bones = random_bones(rng, 1024, scale=True)
                core.mesh_skin_bind(m, t, nrm, ids, sw, 1024)
                core.mesh_skin_pose(m, bones)
            p, _, packed = morph_host(t, nrm, *morph.lists, w, ids, sw, bones)
            want.append(_records(p, packed))
        core.update(view, DIRTY_MESH_SKIN)
        stats, skin = core.mesh_morph_stats(), core.mesh_skin_stats()
        assert (stats.applied, stats.last_meshes, stats.last_launches, stats.last_bytes_uploaded) == (len(SOUPS), len(SOUPS), len(SOUPS), 4 * target_count * len(SOUPS))
        # a launch of the combined kernel that applied a new pose counts as a skinning launch too
        assert (skin.poses, skin.last_meshes, skin.last_launches, skin.last_bytes_uploaded) == ((len(SOUPS), len(SOUPS), len(SOUPS), 48 * 1024 * len(SOUPS)) if with_skin else (0, 0, 0, 0))
        for m, records in enumerate(want):
            got = core.mesh_vertices_probe(m, SOUPS[m])
            assert np.array_equal(got, records), "%d targets, %d triangles: %d of %d words differ, first in corner %d" % (
                target_count, SOUPS[m], int((got != records).sum()), got.size, int(np.nonzero((got != records).any(axis=1))[0][0]))
        assert core.mesh_refit_stats().last_refits == len(SOUPS)
        # all weights zero: without a skin the base records, whatever the targets hold
        if not with_skin:
            for m in range(len(SOUPS)):
                core.mesh_morph_weights(m, np.where(np.arange(target_count) % 2 == 0, F(0.0), F(-0.0)))
            core.update(view, DIRTY_MESH_SKIN)
            base = oracle_lib.view_arrays(view)["vertices"].reshape(-1, 4)
            for m in range(len(SOUPS)):
                got = core.mesh_vertices_probe(m, SOUPS[m])
                assert np.array_equal(got, base[3 * _first_triangle(view, m):][:3 * SOUPS[m]]), "%d targets, %d triangles: all weights zero must leave the vertex bytes" % (target_count, SOUPS[m])
    finally:
        core.close()


def test_the_bind_refuses_and_changes_nothing(soups):
    host, view, tris, normals = soups
    core = _core()
    try:
        core.upload(view)
        t, nrm = tris[2], normals[2]
        morph = random_morph(np.random.RandomState(9), len(t), 3)
        o, c, dp, dn = morph.lists
        core.mesh_morph_bind(2, t, nrm, o, c, dp, dn)
        core.mesh_morph_weights(2, F([1, 0.5, -1]))
        with pytest.raises(CoreError, match="triangle count"):
            core.mesh_morph_bind(3, t, nrm, o, c, dp, dn)
        with pytest.raises(CoreError, match="target_count is 1 ... 1024"):
            core.mesh_morph_bind(2, t, nrm, np.zeros(1026, np.uint32), c[:0], dp[:0], None)
        with pytest.raises(CoreError, match="start at 0"):
            core.mesh_morph_bind(2, t, nrm, o + np.uint32(1), np.concatenate([c, c[:1]]), np.concatenate([dp, dp[:1]]), None)
        down = o.copy(); down[1], down[2] = o[2], o[1]
        assert o[1] != o[2]
        with pytest.raises(CoreError, match="decrease"):
            core.mesh_morph_bind(2, t, nrm, down, c, dp, dn)
        bad = c.copy(); bad[-1] = 3 * len(t)
        with pytest.raises(CoreError, match="corner index"):
            core.mesh_morph_bind(2, t, nrm, o, bad, dp, dn)
        twice = c.copy(); twice[1] = twice[0]
        with pytest.raises(CoreError, match="strictly increasing"):
            core.mesh_morph_bind(2, t, nrm, o, twice, dp, dn)
        d = dp.copy(); d[1, 1] = np.inf
        with pytest.raises(CoreError, match="not finite"):
            core.mesh_morph_bind(2, t, nrm, o, c, d, dn)
        with pytest.raises(CoreError, match="another target count"):
            core.mesh_morph_weights(2, np.zeros(4, F))
        with pytest.raises(CoreError, match="not finite"):
            core.mesh_morph_weights(2, F([0, np.nan, 0]))
        # the binding and its pending weights are as they were
        core.update(view, DIRTY_MESH_SKIN)
        p, _, packed = morph_host(t, nrm, o, c, dp, dn, F([1, 0.5, -1]))
        assert np.array_equal(core.mesh_vertices_probe(2, len(t)), _records(p, packed))
        core.mesh_morph_unbind(2)
        with pytest.raises(CoreError, match="not bound"):
            core.mesh_morph_weights(2, np.zeros(3, F))
        with pytest.raises(CoreError, match="not bound"):
            core.mesh_morph_unbind(2)
    finally:
        core.close()


# ---- in place ----
def test_three_weight_sets_in_the_resident_array_leave_the_bytes_of_the_host_route():
    host, twin = _small_zoo(), _small_zoo()
    a, b = _core(1), _core(1)
    try:
        first = _view(host)
        a.upload(first); b.upload(first)  # (the shared tree cache gives both contexts one topology)
        for h in (host, twin):
            h.set_instance_transforms(moved_instances(h, 0))
        a.update(_view(host), MOVED); b.update(_view(twin), MOVED)
        m0, m1 = _plain_meshes(host, 2)
        shapes = [Morphed(a, host, twin, m0), Morphed(a, host, twin, m1, skin=True)]  # one morphed alone, one morphed and skinned
        for k, w in enumerate(WEIGHTS):
            shapes[0].weights(w)
            shapes[1].weights(w[::-1])
            shapes[1].pose(0.3 * (k + 1), 0.1 * k)
            for h in (host, twin):
                h.set_instance_transforms(moved_instances(h, k + 1))
            a.update(_view(host), DIRTY_MESH_SKIN | MOVED)  # (host's vertices stay at the base shape throughout)
            view = _view(twin)
            b.update(view, DIRTY_MESH_POSITIONS | MOVED)
            where = "weights %d" % k
            for s in shapes:
                s.check(where)
            assert _counts(a) == {"relayouts": 1, "instance fallbacks": 0, "updates": k + 1, "fallbacks": 0}, (where, _counts(a))
            assert _counts(b) == {"relayouts": 1, "instance fallbacks": 0, "updates": k + 1, "fallbacks": 0}, (where, _counts(b))
            ra, rb = a.mesh_refit_stats(), b.mesh_refit_stats()
            assert (ra.last_refits, ra.last_rebuilds) == (rb.last_refits, rb.last_rebuilds) == (2, 0) and ra.seconds_hash == 0.0 and rb.seconds_hash > 0.0, where
            stats, skin = a.mesh_morph_stats(), a.mesh_skin_stats()
            assert (stats.last_meshes, stats.last_launches, stats.last_bytes_uploaded) == (2, 2, 2 * 12)
            assert (skin.last_meshes, skin.last_launches, skin.last_bytes_uploaded) == (1, 1, 96), "the combined launch applied the pose"
            _same_layout(a, b, host, where)
            _against_oracle(a, view, where, {"the host route": b})
    finally:
        a.close(); b.close(); host.close(); twin.close()


# ---- one mesh by the host route, one by weights ----
@pytest.mark.parametrize("in_place", [0, 1])
@pytest.mark.parametrize("skin", [False, True], ids=["morph alone", "with a skin"])
def test_a_positions_update_of_another_mesh_applies_the_kept_weights_again(in_place, skin):
    host, twin, core = _small_zoo(), _small_zoo(), _core(in_place)
    try:
        core.upload(_view(host))
        ma, mb = _plain_meshes(host, 2)
        morphed = Morphed(core, host, twin, mb, skin=skin)
        pa = host.get_mesh(ma)[0]
        morphed.weights(WEIGHTS[1])
        if skin:
            morphed.pose(0.5, 0.2)
        for h in (host, twin):
            h.set_mesh_positions(ma, bend(pa, 0.2, 0.4))
        core.update(_view(host), DIRTY_MESH_POSITIONS | DIRTY_MESH_SKIN | DIRTY_LIGHTS)  # (host's view: mesh a moved, mesh b at the base shape)
        refit = core.mesh_refit_stats()
        assert (refit.last_refits, refit.last_rebuilds) == (2, 0)
        assert core.mesh_morph_stats().last_meshes == 1
        morphed.check("mixed update")
        _against_oracle(core, _view(twin), "mixed update")
        # mesh a again, by the host route alone: the upload brings mesh b's base shape, the kept weights (and palette) put the shape back before anything reads it
        for h in (host, twin):
            h.set_mesh_positions(ma, bend(pa, 0.25, 1.3))
        stale = _view(host)
        base = oracle_lib.view_arrays(stale)["vertices"].reshape(-1, 4)[3 * _first_triangle(stale, mb):][:len(morphed.want)]
        assert not np.array_equal(base, morphed.want), "the view's vertices of the morphed mesh are stale on purpose"
        core.update(stale, DIRTY_MESH_POSITIONS | DIRTY_LIGHTS)
        refit, stats, skin_stats = core.mesh_refit_stats(), core.mesh_morph_stats(), core.mesh_skin_stats()
        assert (refit.last_refits, refit.last_rebuilds) == (1, 0), "the morphed mesh holds the same bits: its tree still fits"
        assert (stats.applied, stats.last_meshes, stats.last_launches, stats.last_bytes_uploaded) == (1, 0, 1, 0)
        assert skin_stats.poses == (1 if skin else 0) and skin_stats.last_launches == (1 if skin else 0), "a re-application is no skinning launch: the count is the first update's"
        morphed.check("after the upload")
        _against_oracle(core, _view(twin), "after the upload")
        # unbound: the view is trusted again, and a host-route update of the same mesh refits it
        core.mesh_morph_unbind(mb)
        if skin:
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
def test_a_rebuild_downloads_the_morphed_vertices():
    host, twin, core = _small_zoo(), _small_zoo(), _core()
    try:
        stale = _view(host)
        core.upload(stale)
        morphed = Morphed(core, host, twin, _plain_meshes(host, 1)[0])
        core.set_mesh_refit(1, 0.0)
        morphed.weights(WEIGHTS[0])
        core.update(stale, DIRTY_MESH_SKIN)
        refit = core.mesh_refit_stats()
        assert (refit.last_refits, refit.last_rebuilds) == (0, 1) and core.mesh_morph_stats().rebuild_downloads == 1 and core.mesh_skin_stats().rebuild_downloads == 0
        morphed.check("mode 1")
        _against_oracle(core, _view(twin), "mode 1")
        core.set_mesh_refit(0, 1.0 + 1e-6)
        morphed.weights(F([4.0, -3.0, 4.0]))
        core.update(stale, DIRTY_MESH_SKIN)
        refit = core.mesh_refit_stats()
        assert refit.max_cost_growth > 1.0 + 1e-6, "the weights must grow the cost beyond the threshold"
        assert (refit.last_refits, refit.last_rebuilds) == (0, 1) and core.mesh_morph_stats().rebuild_downloads == 2
        morphed.check("beyond max_cost_growth")
        _against_oracle(core, _view(twin), "beyond max_cost_growth")
    finally:
        core.close(); host.close(); twin.close()


# ---- a fallback in the middle of an in-place update that carries weights ----
def test_a_fallback_in_the_middle_of_an_in_place_update_morphs_once():
    host, twin, core = _small_zoo(), _small_zoo(), _core(in_place=1)
    try:
        core.upload(_view(host))
        ma, mb = _plain_meshes(host, 2)
        morphed = Morphed(core, host, twin, mb)
        pa = host.get_mesh(ma)[0]
        core.set_mesh_refit(0, 1.0 + 1e-6)
        morphed.weights(F([4.0, -3.0, 4.0]))
        for h in (host, twin):
            h.set_mesh_positions(ma, bend(pa, 0.2, 0.4))
        before, downloads = _counts(core), core.mesh_morph_stats().rebuild_downloads
        core.update(_view(host), DIRTY_MESH_POSITIONS | DIRTY_MESH_SKIN | DIRTY_LIGHTS)
        stats, refit, after = core.mesh_morph_stats(), core.mesh_refit_stats(), _counts(core)
        print("fallback: applied %d, last_meshes %d, last_launches %d; refits %d, rebuilds %d, downloads %d, growth %.6f; %s -> %s" % (
            stats.applied, stats.last_meshes, stats.last_launches, refit.last_refits, refit.last_rebuilds, stats.rebuild_downloads - downloads, refit.max_cost_growth, before, after))
        assert (stats.applied, stats.last_meshes, stats.last_launches) == (1, 1, 1), "the kernel ran once across the fallback"
        assert after["fallbacks"] == before["fallbacks"] + 1 and after["updates"] == before["updates"]
        assert refit.max_cost_growth > 1.0 + 1e-6, "the weights must grow the cost beyond the threshold"
        assert refit.last_rebuilds >= 1 and stats.rebuild_downloads - downloads == 1, "the morphed mesh is built again from a download"
        morphed.check("fallback")
        _against_oracle(core, _view(twin), "fallback")
    finally:
        core.close(); host.close(); twin.close()


# ---- lights ----
def test_a_morphed_emitter_with_its_light_arrays():
    host, twin, core = _small_zoo(), _small_zoo(), _core()
    try:
        core.upload(_view(host))
        morphed = Morphed(core, host, twin, _emissive_mesh(host))
        morphed.weights(WEIGHTS[2])
        view = _view(twin)  # (the light tree and the light BVH's triangles of the morphed emitter; its vertices are not taken from here)
        core.update(view, DIRTY_MESH_SKIN | DIRTY_LIGHTS)
        morphed.check("emitter")
        assert core.mesh_morph_stats().last_bytes_uploaded == 12
        _against_oracle(core, view, "emitter")
    finally:
        core.close(); host.close(); twin.close()


# ---- weights that overflow ----
def test_a_result_that_is_not_finite_is_an_error_that_names_the_mesh():
    host, twin, core = _small_zoo(), _small_zoo(), _core()
    try:
        view = _view(host)
        core.upload(view)
        mesh = _plain_meshes(host, 1)[0]
        morphed = Morphed(core, host, twin, mesh, strength=20.0)
        w = F([3e38, 3e38, 0.0])  # finite weights and finite deltas, of which those beyond 1.14 overflow in the product
        assert not np.isfinite(morph_host(morphed.base_p, morphed.base_n, *morphed.morph.lists, w)[0]).all(), "the twin must see the overflow too"
        core.mesh_morph_weights(mesh, w)
        with pytest.raises(CoreError, match="mesh %d: the weights give a position that is not finite" % mesh):
            core.update(view, DIRTY_MESH_SKIN)
        with pytest.raises(CoreError):
            core.mesh_vertices_probe(mesh, len(morphed.base_p))  # the scene is gone, as after any failed partial update
        core.upload(view)
        _against_oracle(core, view, "a fresh upload after the failed update")
    finally:
        core.close(); host.close(); twin.close()


# ---- the other flavour ----
def test_the_fast_flavour_holds_the_same_vertex_bytes():
    host, twin, core = _small_zoo(), _small_zoo(), _core(flavour="fast")
    try:
        stale = _view(host)
        core.upload(stale)
        morphed = Morphed(core, host, twin, _plain_meshes(host, 1)[0], skin=True)
        morphed.weights(WEIGHTS[0])
        core.update(stale, DIRTY_MESH_SKIN)
        assert core.flavour == "fast"
        morphed.check("fast flavour, no pose yet: the morph alone")
        morphed.pose(0.6, 0.3)
        core.update(stale, DIRTY_MESH_SKIN)
        morphed.check("fast flavour, morphed and posed")
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
        morph = bulge_targets(rest_p)
        ids, sw = two_bone_weights(rest_p)
        host.bind_mesh_morph(mesh, len(rest_p), *morph.lists)
        assert host.is_rendering()[1] == 2, "a binding moves nothing"
        images, made = [], host.mesh_morph_stats()["host_materialisations"]

        def rendered(want, where, applied, poses):
            assert host.is_rendering()[1] == 0, "the integration did not restart"
            host.render_samples(0, 2, samples_per_pass=2)
            fm, sm = host.accumulators()
            stats, skin = host.mesh_morph_stats(), host.mesh_skin_stats()
            assert stats["host_materialisations"] == made + len(images), "the render path does not blend on the host"
            assert (stats["applied"], stats["last_bytes_uploaded"], skin["poses"]) == (applied, 12 if stats["last_meshes"] else 0, poses), (where, stats, skin)
            assert host.mesh_refit_stats()["seconds_hash"] == 0.0
            ofm, osm, _ = oracle_lib.render(_view(host), 0, 2)  # (the public view: blended on the host for it)
            _same(fm, ofm, "%d slots, %s: first moment vs oracle" % (slots, where))
            _same(sm, osm, "%d slots, %s: second moment vs oracle" % (slots, where))
            got = host.get_mesh(mesh)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), where
            assert host.mesh_morph_stats()["host_materialisations"] == made + len(images) + 1
            assert host.is_rendering()[1] == 2, "reading the scene restarts nothing"
            images.append(fm)

        host.set_mesh_weights(mesh, WEIGHTS[0])
        rendered(morph_host(rest_p, rest_n, *morph.lists, WEIGHTS[0]), "weights", 1, 0)
        host.bind_mesh_skin(mesh, ids, sw, 2)  # over the same rest shape
        bones = two_bone_bend(rest_p, 0.5, 0.2)
        host.set_mesh_pose(mesh, bones)
        rendered(morph_host(rest_p, rest_n, *morph.lists, WEIGHTS[0], ids, sw, bones), "weights and a pose", 1, 1)
        host.set_mesh_weights(mesh, WEIGHTS[1])
        last = morph_host(rest_p, rest_n, *morph.lists, WEIGHTS[1], ids, sw, bones)
        rendered(last, "new weights under the pose", 2, 1)
        assert not np.array_equal(images[0], images[1]) and not np.array_equal(images[1], images[2])
        host.unbind_mesh_skin(mesh)
        assert host.is_rendering()[1] == 0, "the mesh is the morph's alone again"
        rendered(morph_host(rest_p, rest_n, *morph.lists, WEIGHTS[1]), "the skin unbound", 3, 1)
        host.unbind_mesh_morph(mesh)
        want_p = morph_host(rest_p, rest_n, *morph.lists, WEIGHTS[1])[0]
        assert host.get_mesh(mesh)[0].tobytes() == want_p.tobytes()
        host.set_mesh_positions(mesh, bend(want_p, 0.2, 0.6))
        host.render_samples(0, 2, samples_per_pass=2)
        fm, sm = host.accumulators()
        ofm, osm, _ = oracle_lib.render(_view(host), 0, 2)
        _same(fm, ofm, "%d slots, unbound and moved by the host route: first moment vs oracle" % slots)
        _same(sm, osm, "%d slots, unbound and moved by the host route: second moment vs oracle" % slots)
    finally:
        host.close()


# ---- one binding goes, the other stays ----
def test_a_part_that_is_unbound_leaves_the_other_and_the_last_takes_the_binding_along():
    """22 and 86 triangles (66 corners: just over a wave; 258: just over a workgroup), 3 bones, 3 targets; the skin's rest shape is NOT the morph's base. After every
    update the vertices are the twin's, byte for byte, and the two stats structs count what skin_meshes is documented to count."""
    rng = np.random.RandomState(11)
    sizes = [22, 86]
    host = Host()
    scenes.apply_benchmark_settings(host, 16, 16, 2, sky=(0.5, 0.5, 0.5))
    mat = host.add_material(scenes._material((0.6, 0.6, 0.6), 0.6))
    core = _core()
    try:
        base = [(soup(rng, n).reshape(n, 9), unit_normals(rng, n)) for n in sizes]
        rest = [(soup(rng, n).reshape(n, 9), unit_normals(rng, n)) for n in sizes]
        assert all(not np.array_equal(b[0], r[0]) and not np.array_equal(b[1], r[1]) for b, r in zip(base, rest)), "two shapes per mesh"
        for k, (t, nrm) in enumerate(base):
            host.new_instance(host.add_mesh(t, np.full(len(t), mat, dtype=np.uint16), normals=nrm), position=(3.0 * k, 0.0, 0.0))
        scenes.set_camera(host, (0.0, 0.0, 40.0), (0.0, 0.0, 0.0))
        view = _view(host)
        core.upload(view)
        skins = [random_skin(rng, n, 3) for n in sizes]
        morphs = [random_morph(rng, n, 3) for n in sizes]
        meshes = range(len(sizes))

        def updated(where, want, skin_counts, morph_counts):
            core.update(view, DIRTY_MESH_SKIN)
            for m in meshes:
                p, _, packed = want(m)
                got, records = core.mesh_vertices_probe(m, sizes[m]), _records(p, packed)
                assert np.array_equal(got, records), "%s: %d of %d words of mesh %d differ from the twin's" % (where, int((got != records).sum()), got.size, m)
            s, ms = core.mesh_skin_stats(), core.mesh_morph_stats()
            assert (s.poses, s.last_meshes, s.last_launches, s.last_bytes_uploaded) == skin_counts, (where, "skin")
            assert (ms.applied, ms.last_meshes, ms.last_launches, ms.last_bytes_uploaded) == morph_counts, (where, "morph")
            assert (s.rebuild_downloads, ms.rebuild_downloads) == (0, 0), where

        def new_pose():
            bones = random_bones(rng, 3, scale=True)
            for m in meshes:
                core.mesh_skin_pose(m, bones)
            return bones

        def new_weights():
            w = random_weights(rng, 3)
            for m in meshes:
                core.mesh_morph_weights(m, w)
            return w

        # 1. a skin and a pose: the skin's own rest shape
        for m in meshes:
            core.mesh_skin_bind(m, *rest[m], *skins[m], 3)
        bones = new_pose()
        updated("skin alone", lambda m: skin_host(*rest[m], *skins[m], bones), (2, 2, 2, 2 * 144), (0, 0, 0, 0))
        # 2. a morph next to it: the morph's base under the kept palette, the skin's rest shape is not read; no new pose, so the skin's stats are the last update's
        for m in meshes:
            core.mesh_morph_bind(m, *base[m], *morphs[m].lists)
        w = new_weights()
        updated("morph and skin", lambda m: morph_host(*base[m], *morphs[m].lists, w, *skins[m], bones), (2, 2, 2, 2 * 144), (2, 2, 2, 2 * 12))
        # 3. the skin goes, the morph stays
        for m in meshes:
            core.mesh_skin_unbind(m)
        w = new_weights()
        updated("skin unbound", lambda m: morph_host(*base[m], *morphs[m].lists, w), (2, 2, 2, 2 * 144), (4, 2, 2, 2 * 12))
        # 4. a skin again, without a pose: the morph alone writes
        for m in meshes:
            core.mesh_skin_bind(m, *rest[m], *skins[m], 3)
        w = new_weights()
        updated("skin bound again, no pose yet", lambda m: morph_host(*base[m], *morphs[m].lists, w), (2, 2, 2, 2 * 144), (6, 2, 2, 2 * 12))
        # 5. the morph goes, the skin stays and gets a pose: its own rest shape again
        for m in meshes:
            core.mesh_morph_unbind(m)
        bones = new_pose()
        updated("morph unbound", lambda m: skin_host(*rest[m], *skins[m], bones), (4, 2, 2, 2 * 144), (6, 2, 2, 2 * 12))
        with pytest.raises(CoreError, match="not bound"):
            core.mesh_morph_weights(0, np.zeros(3, F))
        # 6. the last part takes the binding along
        for m in meshes:
            core.mesh_skin_unbind(m)
            with pytest.raises(CoreError, match="not bound"):
                core.mesh_skin_pose(m, bones)
            with pytest.raises(CoreError, match="not bound"):
                core.mesh_skin_unbind(m)
            with pytest.raises(CoreError, match="not bound"):
                core.mesh_morph_unbind(m)
    finally:
        core.close(); host.close()
