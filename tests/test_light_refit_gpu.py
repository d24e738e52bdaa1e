"""The light tree's refit on the device: lumc_light_refit_bind -> LUMC_DIRTY_LIGHT_POSITIONS -> csrc/host/light_refit.hip (k_light_fragments, k_light_slot_stats,
k_light_nodes), the light BVH's refit and k_light_table, scene_device.hip refit_lights.

What the update leaves on the device is held to the host twin (lumc_light_refit_host; tests/test_light_refit.py holds that to its definition) byte for byte - root,
float table, nodes -, the light table to a fresh upload of the moved scene light by light, the light BVH to the host's refit of the tree the upload built; what is
rendered over it to the CPU oracle given the twin's light arrays, bit for bit."""
import numpy as np
import pytest

import oracle_lib
from luminary_amd import scenes
from luminary_amd.core import (DIRTY_INSTANCE_TRANSFORMS, DIRTY_LIGHT_POSITIONS, DIRTY_LIGHTS, DIRTY_MESH_POSITIONS, DIRTY_MESH_SKIN, LIGHT_REFIT_ZERO_AREA,
                               Core, LightRefitPlan, bvh_refit_probe, morph_host, skin_host)
from test_instance_transforms_api import moved_instances
from test_instance_update_gpu import _against_oracle
from test_light_refit import Built, lamp_scene, light_arrays, moved_emitters, transforms_of, with_light_arrays
from test_mesh_positions_api import bend
from test_mesh_refit import boxes_of
from test_mesh_morph import bulge_targets
from test_mesh_refit_gpu import _emissive_mesh
from test_mesh_skin import two_bone_bend, two_bone_weights

pytestmark = pytest.mark.gpu
F, U = np.float32, np.uint32
MOVED_VERTICES = DIRTY_MESH_POSITIONS | DIRTY_LIGHT_POSITIONS
MOVED_INSTANCES = DIRTY_INSTANCE_TRANSFORMS | DIRTY_LIGHT_POSITIONS


def _zoo():
    return scenes.zoo_scene(48, 32, 3)


def _view(host):
    return oracle_lib.with_luts(host.device_scene())


def _core(in_place=0, flavour="exact"):
    core = Core(0)
    core.set_flavour(flavour)
    core.set_mesh_refit_in_place(in_place)
    return core


def _same_arrays(a, b, where, keys=("root", "root_children", "nodes", "table", "bvh_nodes", "bvh_tris")):
    for k in keys:
        x, y = np.ascontiguousarray(a[k]).reshape(-1).view(np.uint8), np.ascontiguousarray(b[k]).reshape(-1).view(np.uint8)
        assert x.size == y.size and np.array_equal(x, y), "%s: %s differs in %d of %d bytes" % (where, k, int((x != y).sum()) if x.size == y.size else -1, x.size)


class Bound:
    """A scene uploaded to a context with its light tree's plan bound, and what the build left on the host."""

    def __init__(self, host, core):
        self.host, self.core = host, core
        core.upload(_view(host))
        self.built = Built(host)
        core.light_refit_bind(self.built.plan)
        self.uploaded = core.light_arrays_probe()

    def check_against_twin(self, twin, where):
        """The device's light structures after a refit against the twin's result `twin` (light_refit_host's dict)."""
        got = self.core.light_arrays_probe()
        n = len(self.built.arrays["handles"])
        assert twin["report"].refitted == 1, where
        assert np.array_equal(got["root"], twin["root"]), "%s: %d root bytes differ from the twin's" % (where, int((got["root"] != twin["root"]).sum()))
        assert np.array_equal(got["root_children"].view(U), twin["root_children"].view(U)), "%s: %d words of the root's float table differ" % (
            where, int((got["root_children"].view(U) != twin["root_children"].view(U)).sum()))
        assert np.array_equal(got["nodes"], twin["nodes"]), "%s: %d node bytes differ from the twin's" % (where, int((got["nodes"] != twin["nodes"]).sum()))
        # the light BVH: the host's refit of the tree the upload built, and bvh_tri of the twin's triangles in its leaf order
        old, new = self.built.arrays["tris"].reshape(n, 3, 4)[:, :, :3], twin["light_bvh_tris"].reshape(n, 3, 4)[:, :, :3]
        r = bvh_refit_probe(boxes_of(old), boxes_of(new), "sah", on_gpu=False)
        assert np.array_equal(r["built"], self.uploaded["bvh_nodes"]), where + ": the probe's tree is the light BVH the upload built"
        assert np.array_equal(got["bvh_nodes"], r["host_refit"]), "%s: %d words of the light BVH's nodes differ from the host's refit" % (where, int((got["bvh_nodes"] != r["host_refit"]).sum()))
        tris = np.zeros((n, 12), U)
        p = new[r["prims"]]
        tris[:, 0:3], tris[:, 4:7], tris[:, 8:11] = p[:, 0].view(U), (p[:, 1] - p[:, 0]).view(U), (p[:, 2] - p[:, 0]).view(U)
        tris[:, 3] = r["prims"]
        assert np.array_equal(got["bvh_tris"][:n], tris), "%s: %d words of the light BVH's triangles differ" % (where, int((got["bvh_tris"][:n] != tris).sum()))
        return got

    def check_table_against_fresh_upload(self, got, view, where):
        """k_light_table's records light by light against a context that was given the moved scene whole (its light order is its own build's)."""
        fresh = _core()
        try:
            fresh.upload(view)
            want = fresh.light_arrays_probe()["table"]
            place = {(int(i), int(t)): k for k, (i, t) in enumerate(light_arrays(view)["handles"])}
            order = [place[(int(i), int(t))] for i, t in self.built.arrays["handles"]]
            assert np.array_equal(got["table"], want[order]), "%s: %d words of the light table differ from a fresh upload's" % (where, int((got["table"] != want[order]).sum()))
        finally:
            fresh.close()


# ---- fails without the feature: bytes after one refit ----
@pytest.mark.parametrize("lights", [2, 9, 129, 1000, "zoo"])
def test_one_refit_leaves_the_twins_bytes_on_the_device(lights):
    host, core = (_zoo() if lights == "zoo" else lamp_scene(lights)), _core()
    try:
        bound = Bound(host, core)
        a = bound.built.arrays
        assert np.array_equal(bound.uploaded["root"], a["root"]) and np.array_equal(bound.uploaded["root_children"].view(U), a["root_children"].view(U)) and np.array_equal(bound.uploaded["nodes"], a["nodes"])
        moved_emitters(host, 0.3)
        view = _view(host)
        core.update(view, MOVED_VERTICES)
        st = core.light_refit_stats()
        print("%s lights: %.3f ms: fragments %.3f, statistics %.3f, nodes %.3f, light BVH %.3f, table %.3f; %d launches, %d bytes down, cost growth %.4f" % (
            lights, 1e3 * st.seconds, 1e3 * st.seconds_fragments, 1e3 * st.seconds_stats, 1e3 * st.seconds_nodes, 1e3 * st.seconds_light_bvh, 1e3 * st.seconds_table, st.last_launches,
            st.last_bytes_downloaded, st.cost_growth))
        assert (st.refits, st.fallbacks, st.last_flags) == (1, 0, 0) and not core.light_refit_needs_rebuild()
        twin = bound.built.refit(light_arrays(view)["vertices"])
        assert st.cost_growth == twin["report"].cost_growth, "the cost is summed from the same (power, variance) in the same order"
        got = bound.check_against_twin(twin, "%s lights" % lights)
        assert not np.array_equal(got["root"], bound.uploaded["root"]), "the move changes the root"
        bound.check_table_against_fresh_upload(got, view, "%s lights" % lights)
    finally:
        core.close(); host.close()


# ---- fails without the feature: every route renders like the oracle given the twin's light arrays ----
def _oracle_view(view, built, twin):
    return with_light_arrays(view, twin["root"], twin["nodes"], built.arrays["handles"], twin["light_bvh_tris"])


@pytest.mark.parametrize("route", ["vertices", "instances", "vertices and instances in place", "pose", "weights"])
def test_a_moved_emitter_renders_like_the_oracle_given_the_twins_light_arrays(route):
    host, core = _zoo(), _core(in_place=1 if "in place" in route else 0)
    other = _zoo() if route in ("pose", "weights") else None
    try:
        stale = _view(host)
        bound = Bound(host, core)
        built = bound.built
        before = _against_oracle(core, stale, route + ": before the move")
        plan, dirty = built.plan, 0
        if route == "pose":  # the device poses the emitting mesh itself; a second host is given the twin's vertices for the oracle's view
            mesh = _emissive_mesh(host)
            rest_p, rest_n = host.get_mesh(mesh)[:2]
            ids, w = two_bone_weights(rest_p)
            core.mesh_skin_bind(mesh, rest_p, rest_n, ids, w, 2)
            bones = two_bone_bend(rest_p, 0.5, 0.2)
            core.mesh_skin_pose(mesh, bones)
            p, n, _ = skin_host(rest_p, rest_n, ids, w, bones)
            other.set_mesh_positions(mesh, p, n)
            core.update(stale, DIRTY_MESH_SKIN | DIRTY_LIGHT_POSITIONS)  # (the view still holds the rest pose: not read)
            view = _view(other)
        elif route == "weights":  # likewise through morph targets
            mesh = _emissive_mesh(host)
            base_p, base_n = host.get_mesh(mesh)[:2]
            morph = bulge_targets(base_p, 2, 0.2)
            weights = np.float32([0.8, -0.4])
            core.mesh_morph_bind(mesh, base_p, base_n, *morph.lists)
            core.mesh_morph_weights(mesh, weights)
            p, n, _ = morph_host(base_p, base_n, *morph.lists, weights)
            other.set_mesh_positions(mesh, p, n)
            core.update(stale, DIRTY_MESH_SKIN | DIRTY_LIGHT_POSITIONS)
            view = _view(other)
        else:
            if "vertices" in route:
                moved_emitters(host, 0.4)
                dirty |= MOVED_VERTICES
            if "instances" in route:
                host.set_instance_transforms(moved_instances(host, 0, every=1))
                f, _, ti, sl = built.plan.arrays()
                plan = LightRefitPlan.from_arrays(f, transforms_of(host, built.plan), ti, sl, built.plan.root_cost)
                core.light_refit_transforms(plan.arrays()[1])
                dirty |= MOVED_INSTANCES
            view = _view(host)
            core.update(view, dirty)
        st = core.light_refit_stats()
        assert (st.refits, st.fallbacks) == (1, 0) and not core.light_refit_needs_rebuild(), route
        assert st.last_bytes_uploaded == (40 * plan.num_transforms if "instances" in route else 0), "no per-light traffic goes up"
        twin = built.refit(light_arrays(view)["vertices"], plan)
        bound.check_against_twin(twin, route)
        after = _against_oracle(core, _oracle_view(view, built, twin), route)
        assert int((after != before).sum()) > 20, "the move must change the image"
    finally:
        core.close(); host.close()
        if other:
            other.close()


# ---- no per-light traffic ----
def test_what_comes_down_does_not_grow_with_the_lights():
    down = {}
    for lights in (9, 1000):
        host, core = lamp_scene(lights), _core()
        try:
            Bound(host, core)
            moved_emitters(host, 0.2)
            core.update(_view(host), MOVED_VERTICES)
            st = core.light_refit_stats()
            assert st.refits == 1 and st.last_bytes_uploaded == 0
            down[lights] = st.last_bytes_downloaded
        finally:
            core.close(); host.close()
    assert down[9] == down[1000] and down[9] <= 4 + 1024 + 24, down


# ---- fallbacks leave the lights alone ----
def test_a_degenerate_triangle_asks_for_a_rebuild_and_touches_nothing():
    host, core = lamp_scene(129), _core()
    try:
        bound = Bound(host, core)
        p = host.get_mesh(1)[0].copy()
        p += F(0.125)
        p[5, 3:6] = p[5, 0:3]
        p[5, 6:9] = p[5, 0:3]
        host.set_mesh_positions(1, p)
        view = _view(host)
        assert view.num_lights == 128, "the host's build drops the collapsed triangle"
        core.update(view, MOVED_VERTICES)
        st = core.light_refit_stats()
        assert core.light_refit_needs_rebuild() and (st.refits, st.fallbacks) == (0, 1) and st.last_flags == LIGHT_REFIT_ZERO_AREA
        _same_arrays(core.light_arrays_probe(), bound.uploaded, "a collapsed triangle")
        core.update(view, DIRTY_LIGHTS)  # the rebuild the caller then asks for: the same arrays as a context that never had a binding
        assert not core.light_refit_needs_rebuild()
        fresh = _core()
        try:
            fresh.upload(view)
            _same_arrays(core.light_arrays_probe(), fresh.light_arrays_probe(), "after the rebuild")
        finally:
            fresh.close()
    finally:
        core.close(); host.close()


def test_a_cost_beyond_the_bound_asks_for_a_rebuild_and_touches_nothing():
    host, core = lamp_scene(129), _core()
    try:
        bound = Bound(host, core)
        core.set_light_refit(1.0 + 1e-3)
        p = host.get_mesh(1)[0]
        host.set_mesh_positions(1, (p * F(2.0)).astype(F))  # twice the size: four times the power, four times the variance
        view = _view(host)
        core.update(view, MOVED_VERTICES)
        st = core.light_refit_stats()
        assert core.light_refit_needs_rebuild() and (st.refits, st.fallbacks, st.last_flags) == (0, 1, 0) and st.cost_growth > 4.0, st.cost_growth
        _same_arrays(core.light_arrays_probe(), bound.uploaded, "beyond the bound")
        core.set_light_refit(0.0)  # never for quality: the same update refits
        core.update(view, MOVED_VERTICES)
        assert not core.light_refit_needs_rebuild() and core.light_refit_stats().refits == 1
        bound.check_against_twin(bound.built.refit(light_arrays(view)["vertices"]), "no bound")
    finally:
        core.close(); host.close()


# ---- the binding's lifetime ----
def test_new_lights_drop_the_binding_and_a_new_one_refits_again():
    host, core = lamp_scene(129), _core()
    try:
        bound = Bound(host, core)
        moved_emitters(host, 0.2)
        view = _view(host)
        core.update(view, MOVED_VERTICES | DIRTY_LIGHTS)  # with new lights the bit is ignored: the host's path, as without it
        st = core.light_refit_stats()
        assert (st.refits, st.fallbacks) == (0, 0) and not core.light_refit_needs_rebuild()
        fresh = _core()
        try:
            fresh.upload(view)
            _same_arrays(core.light_arrays_probe(), fresh.light_arrays_probe(), "LIGHTS with the bit")
        finally:
            fresh.close()
        moved_emitters(host, 0.9)
        view2 = _view(host)
        held = core.light_arrays_probe()
        core.update(view2, MOVED_VERTICES)  # the binding went with the old lights
        assert core.light_refit_needs_rebuild() and core.light_refit_stats().fallbacks == 1
        _same_arrays(core.light_arrays_probe(), held, "without a binding")
        core.update(view2, DIRTY_LIGHTS)
        rebuilt = Built(host)
        core.light_refit_bind(rebuilt.plan)
        bound.built, bound.uploaded = rebuilt, core.light_arrays_probe()
        moved_emitters(host, 1.4)
        view3 = _view(host)
        core.update(view3, MOVED_VERTICES)
        assert not core.light_refit_needs_rebuild() and core.light_refit_stats().refits == 1
        bound.check_against_twin(rebuilt.refit(light_arrays(view3)["vertices"]), "bound again")
        core.upload(view3)  # an upload drops it too
        core.update(view3, MOVED_VERTICES)
        assert core.light_refit_needs_rebuild()
    finally:
        core.close(); host.close()


def test_a_plan_that_is_not_the_scenes_is_refused():
    host, other, core = lamp_scene(129), lamp_scene(9), _core()
    try:
        from luminary_amd.core import CoreError
        core.upload(_view(host))
        with pytest.raises(CoreError):
            core.light_refit_bind(Built(other).plan)
        built = Built(host)
        f, t, ti, sl = built.plan.arrays()
        bad = f.copy()
        bad[3, 2] = 1 << 20  # a triangle the mesh does not have
        with pytest.raises(CoreError):
            core.light_refit_bind(LightRefitPlan.from_arrays(bad, t, ti, sl, 1.0))
        bad = sl.copy()
        bad[130, 1] = 1 << 20
        with pytest.raises(CoreError):
            core.light_refit_bind(LightRefitPlan.from_arrays(f, t, ti, bad, 1.0))
        moved_emitters(host, 0.2)
        core.update(_view(host), MOVED_VERTICES)
        assert core.light_refit_needs_rebuild(), "a refused bind leaves no binding"
    finally:
        core.close(); host.close(); other.close()


# ---- the fast flavour's context holds the same bytes ----
def test_the_fast_flavours_context_holds_the_same_bytes():
    host, core = _zoo(), _core(flavour="fast")
    try:
        bound = Bound(host, core)
        moved_emitters(host, 0.6)
        view = _view(host)
        core.update(view, MOVED_VERTICES)
        assert core.light_refit_stats().refits == 1
        bound.check_against_twin(bound.built.refit(light_arrays(view)["vertices"]), "fast flavour")
    finally:
        core.close(); host.close()


# ---- the host API: the switch, on one and on two device slots ----
def _host_against_oracle(host, where):
    host.render_samples(0, 2, samples_per_pass=2)
    fm, sm = host.accumulators()
    ofm, osm, _ = oracle_lib.render(_view(host), 0, 2)  # (the public view: its light arrays brought up to date by the twin)
    assert np.array_equal(np.asarray(fm).view(U), np.asarray(ofm).view(U)) and np.array_equal(np.asarray(sm).view(U), np.asarray(osm).view(U)), where + ": the host renders like the oracle on its view"
    return np.asarray(fm).copy()


@pytest.mark.parametrize("slots", [1, 2])
def test_the_host_api_refits_on_every_device_slot_and_rebuilds_when_a_device_asks(slots, monkeypatch):
    if slots > 1:
        monkeypatch.setenv("LUM_FAKE_DEVICES", str(slots))
        monkeypatch.setenv("LUM_MAX_DEVICES", "8")
    host, plain = _zoo(), _zoo()
    try:
        assert host.get_device_count() == slots
        host.set_light_refit(1)
        images = [_host_against_oracle(host, "%d slots, as uploaded" % slots)]
        lamp = _emissive_mesh(host)
        rest_p, rest_n = host.get_mesh(lamp)[:2]
        # three poses of an emitting mesh: nothing is posed on the host, every one is a refit
        ids, w = two_bone_weights(rest_p)
        host.bind_mesh_skin(lamp, ids, w, 2)
        for step in range(3):
            host.set_mesh_pose(lamp, two_bone_bend(rest_p, 0.3 + 0.2 * step, 0.1 * step))
            if step < 2:
                host.render_samples(0, 2, samples_per_pass=2)
            else:
                host.render_samples(0, 2, samples_per_pass=2)
                fm_posed = np.asarray(host.accumulators()[0]).copy()
            st = host.light_refit_stats()
            assert host.mesh_skin_stats()["host_materialisations"] == 0, "an emitter's pose stays lazy on the host"
            assert (st["refits"], st["fallbacks"], st["host_rebuilds"], st["last_bytes_uploaded"]) == (step + 1, 0, 0, 0), st
        ofm, _, _ = oracle_lib.render(_view(host), 0, 2)  # (reading the view poses the mesh on the host, and restarts nothing)
        assert np.array_equal(fm_posed.view(U), np.asarray(ofm).view(U)), "%d slots, posed: the host renders like the oracle on its view" % slots
        images.append(fm_posed)
        host.unbind_mesh_skin(lamp)
        # moved vertices, then moved instances
        host.set_mesh_positions(lamp, bend(rest_p, 0.2, 0.7))
        images.append(_host_against_oracle(host, "%d slots, moved vertices" % slots))
        host.set_instance_transforms(moved_instances(host, 1, every=1))
        images.append(_host_against_oracle(host, "%d slots, moved instances" % slots))
        st = host.light_refit_stats()
        assert (st["fallbacks"], st["host_rebuilds"]) == (0, 0) and st["refits"] >= 5 and st["last_bytes_uploaded"] == 40 * host.light_refit_plan().num_transforms, st
        for a, b in zip(images, images[1:]):
            assert int((a != b).sum()) > 20, "every move changes the image"
        # a collapsed triangle: the device asks, the host builds - what a host without the switch produces, byte for byte
        for h in (host, plain):
            if h is plain:
                h.set_instance_transforms(moved_instances(h, 1, every=1))
            p = bend(rest_p, 0.2, 0.7)
            p[3, 3:6] = p[3, 0:3]
            p[3, 6:9] = p[3, 0:3]
            h.set_mesh_positions(lamp, p)
            h.render_samples(0, 2, samples_per_pass=2)
        st = host.light_refit_stats()
        assert st["host_rebuilds"] == 1 and st["last_flags"] == LIGHT_REFIT_ZERO_AREA, st
        (fm, sm), (pfm, psm) = host.accumulators(), plain.accumulators()
        assert np.array_equal(np.asarray(fm).view(U), np.asarray(pfm).view(U)) and np.array_equal(np.asarray(sm).view(U), np.asarray(psm).view(U)), "after the rebuild: the image of a host without the switch"
        a, b = light_arrays(host.device_scene()), light_arrays(plain.device_scene())
        for k in b:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), "after the rebuild: %s of a host without the switch" % k
        # and the next move refits again, over the new binding
        host.set_mesh_positions(lamp, bend(rest_p, 0.2, 0.2))
        _host_against_oracle(host, "%d slots, after the rebuild" % slots)
        st2 = host.light_refit_stats()
        assert st2["refits"] == st["refits"] + 1 and st2["host_rebuilds"] == 1, st2
    finally:
        host.close(); plain.close()



# ---- a context that takes the lights' part from the view while the devices refit gets the tree of the scene as it stands (the view is not read in between) ----
def _images(host):
    host.render_samples(0, 2, samples_per_pass=2)
    fm, sm = host.accumulators()
    return np.asarray(fm).copy(), np.asarray(sm).copy()


def _same_images(a, b, where):
    assert np.array_equal(a[0].view(U), b[0].view(U)) and np.array_equal(a[1].view(U), b[1].view(U)), where


def test_a_pending_lights_update_beside_a_move_uploads_the_tree_of_the_moved_scene():
    host, plain = _zoo(), _zoo()
    try:
        host.set_light_refit(1)      # marks the lights' part for the context
        host.device_scene()          # encodes the scene; the context has still taken nothing
        lamp = _emissive_mesh(host)
        moved = bend(host.get_mesh(lamp)[0], 0.25, 0.3)
        for h in (host, plain):
            h.set_mesh_positions(lamp, moved)
        _same_images(_images(host), _images(plain), "the first render after switch, read and move: the image of a host without the switch")
        st = host.light_refit_stats()
        assert (st["refits"], st["fallbacks"]) == (0, 0), "the context took the lights' part, built from the moved scene"
        host.set_mesh_positions(lamp, bend(moved, 0.1, 0.9))  # and the binding it got then refits
        _host_against_oracle(host, "after the refit")
        assert host.light_refit_stats()["refits"] == 1
    finally:
        host.close(); plain.close()


def test_a_slot_enabled_after_refits_samples_the_tree_the_others_hold(monkeypatch):
    monkeypatch.setenv("LUM_FAKE_DEVICES", "2")
    monkeypatch.setenv("LUM_MAX_DEVICES", "8")
    host, plain = _zoo(), _zoo()
    try:
        assert host.get_device_count() == 2
        host.set_device_enable(1, False)
        host.set_light_refit(1)
        host.render_samples(0, 2, samples_per_pass=2)
        lamp = _emissive_mesh(host)
        rest = host.get_mesh(lamp)[0]
        for step in range(2):  # refit frames on the one enabled device
            host.set_mesh_positions(lamp, bend(rest, 0.2, 0.4 + 0.3 * step))
            host.set_instance_transforms(moved_instances(host, step, every=1))
            host.render_samples(0, 2, samples_per_pass=2)
        assert host.light_refit_stats()["refits"] == 2
        host.set_device_enable(1, True)  # its context takes the whole scene: the tree is built from the scene as it stands, for both
        for step in range(2):
            plain.set_mesh_positions(lamp, bend(rest, 0.2, 0.4 + 0.3 * step))
            plain.set_instance_transforms(moved_instances(plain, step, every=1))
        _same_images(_images(host), _images(plain), "two slots, the second enabled after two refits: the image of a host without the switch")
        assert host.light_refit_stats()["refits"] == 2
        host.set_mesh_positions(lamp, bend(rest, 0.2, 1.3))  # both slots are bound now and refit
        _host_against_oracle(host, "two slots after the enable")
        st = host.light_refit_stats()
        assert (st["refits"], st["fallbacks"], st["host_rebuilds"]) == (3, 0, 0), st
    finally:
        host.close(); plain.close()


# ---- switch off: every array equals the parent's route ----
PARENT_MOVED_VERTICES, PARENT_MOVED_INSTANCES = DIRTY_MESH_POSITIONS | DIRTY_LIGHTS, DIRTY_INSTANCE_TRANSFORMS | DIRTY_LIGHTS


@pytest.mark.parametrize("route", ["vertices", "instances", "vertices and instances in place", "pose", "weights"])
def test_without_the_bit_a_bound_context_takes_the_parents_route_byte_for_byte(route):
    """Two contexts through the same updates with the parent's flags - LUMC_DIRTY_LIGHTS for the moved emitter - one of them with a plan bound and a cost bound set:
    the switch's state must not show. Every light array from the probe and the image."""
    host = _zoo()
    cores = [_core(in_place=1 if "in place" in route else 0), _core(in_place=1 if "in place" in route else 0)]
    try:
        stale = _view(host)
        for core in cores:
            core.upload(stale)
        cores[0].set_light_refit(1.5)
        cores[0].light_refit_bind(Built(host).plan)
        mesh = _emissive_mesh(host)
        base_p, base_n = host.get_mesh(mesh)[:2]
        if route == "pose":
            ids, w = two_bone_weights(base_p)
            bones = two_bone_bend(base_p, 0.5, 0.2)
            p, n, _ = skin_host(base_p, base_n, ids, w, bones)
            for core in cores:
                core.mesh_skin_bind(mesh, base_p, base_n, ids, w, 2)
                core.mesh_skin_pose(mesh, bones)
            host.set_mesh_positions(mesh, p, n)  # the view's light arrays from the posed vertices, as the parent's route asks
            dirty = DIRTY_MESH_SKIN | DIRTY_LIGHTS
        elif route == "weights":
            morph = bulge_targets(base_p, 2, 0.2)
            weights = np.float32([0.8, -0.4])
            p, n, _ = morph_host(base_p, base_n, *morph.lists, weights)
            for core in cores:
                core.mesh_morph_bind(mesh, base_p, base_n, *morph.lists)
                core.mesh_morph_weights(mesh, weights)
            host.set_mesh_positions(mesh, p, n)
            dirty = DIRTY_MESH_SKIN | DIRTY_LIGHTS
        else:
            dirty = 0
            if "vertices" in route:
                moved_emitters(host, 0.4)
                dirty |= PARENT_MOVED_VERTICES
            if "instances" in route:
                host.set_instance_transforms(moved_instances(host, 0, every=1))
                dirty |= PARENT_MOVED_INSTANCES
        view = _view(host)
        for core in cores:
            core.update(view, dirty)
        st = cores[0].light_refit_stats()
        assert (st.refits, st.fallbacks) == (0, 0) and not cores[0].light_refit_needs_rebuild()
        _same_arrays(cores[0].light_arrays_probe(), cores[1].light_arrays_probe(), route)
        _against_oracle(cores[0], view, route + ", bound, without the bit", fresh={"a context that was never bound": cores[1]})
    finally:
        for core in cores:
            core.close()
        host.close()


def test_a_host_switched_on_and_off_again_renders_every_route_like_one_that_never_had_the_switch():
    never, toggled = _zoo(), _zoo()
    try:
        toggled.set_light_refit(1, 1.5)
        lamp = _emissive_mesh(never)
        rest_p = never.get_mesh(lamp)[0]
        ids, w = two_bone_weights(rest_p)
        morph = bulge_targets(rest_p, 2, 0.2)
        steps = [("as uploaded", lambda h: None),
                 ("moved vertices", lambda h: h.set_mesh_positions(lamp, bend(rest_p, 0.2, 0.5))),
                 ("moved instances", lambda h: h.set_instance_transforms(moved_instances(h, 0, every=1))),
                 ("bound", lambda h: h.bind_mesh_skin(lamp, ids, w, 2)),
                 ("posed", lambda h: h.set_mesh_pose(lamp, two_bone_bend(rest_p, 0.4, 0.1))),
                 ("morph bound", lambda h: h.bind_mesh_morph(lamp, len(rest_p), *morph.lists)),
                 ("weights", lambda h: h.set_mesh_weights(lamp, np.float32([0.6, -0.3])))]
        for k, (name, edit) in enumerate(steps):
            for h in (never, toggled):
                edit(h)
            if k == 2:
                toggled.set_light_refit(0)  # off again after a refit frame, with a move pending: from here on the parent's route
            a, b = _images(toggled), _images(never)
            st = toggled.light_refit_stats()
            if k == 1:
                assert st["refits"] == 1, "while it is on the move is a refit"
            if k >= 2:
                _same_images(a, b, name + ": the image of a host that never had the switch")
                assert st["refits"] == 1 and st["host_rebuilds"] == 0, st
        x, y = light_arrays(toggled.device_scene()), light_arrays(never.device_scene())
        for key in y:
            assert np.array_equal(x[key].view(np.uint8), y[key].view(np.uint8)), key
    finally:
        never.close(); toggled.close()
