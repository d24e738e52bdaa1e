"""Deformable meshes on the device: luminary_ext_set_mesh_positions -> LUMC_DIRTY_MESH_POSITIONS -> csrc/host/bvh_refit.hip.

The device's refit is held to the host's (tests/test_mesh_refit.py) byte for byte; what is rendered and traced over refitted trees is held to the CPU oracle
bit for bit, as everything in the exact flavour is - its images do not depend on the trees - and to a fresh upload of the moved geometry."""
import numpy as np
import pytest

import oracle_lib
import ray_truth
from luminary_amd import Host, scenes
from luminary_amd.core import DIRTY_LIGHTS, DIRTY_MESH_POSITIONS, Core, bvh_refit_probe
from test_mesh_positions_api import bend
from test_mesh_refit import SIZES, assert_same_topology, boxes_of, motions, soup
from test_ray_truth import _normalise32, _targets

pytestmark = pytest.mark.gpu
BUILDERS = ["sah", "sah_gpu", "lbvh", "ploc"]
NONE = 0xFFFFFFFF


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: %d of %d values differ" % (what, int((a.view(np.uint32) != b.view(np.uint32)).sum()), a.size)


# ---- 7 ----
@pytest.mark.parametrize("builder", BUILDERS)
def test_the_device_refit_is_the_host_refit_byte_for_byte(builder):
    for n in SIZES:  # 1, 2, 3: a root with a single leaf child, levels of one node
        tris, to = motions(n)
        to = dict(to, identity=tris)
        for name, moved in to.items():
            where = "%s, n = %d, %s" % (builder, n, name)
            r = bvh_refit_probe(boxes_of(tris), boxes_of(moved), builder, on_gpu=True)
            assert r["refit"] is not None and r["host_refit"] is not None, where
            assert r["refit"].tobytes() == r["host_refit"].tobytes(), "%s: %d node words differ" % (where, int((r["refit"] != r["host_refit"]).sum()))
            assert np.float64(r["cost"][1]).tobytes() == np.float64(r["cost"][2]).tobytes(), where
            assert r["valid"] == 1, where
            assert_same_topology(r["built"], r["refit"], where)
            if name == "identity":  # the GPU builders' boxes are the plain union too; where one is not, the refitted box must lie inside the built one
                lo = slice(0, 12); hi = slice(12, 24)
                built, refit = r["built"].view(np.float32), r["refit"].view(np.float32)
                assert (refit[:, lo] >= built[:, lo]).all() and (refit[:, hi] <= built[:, hi]).all(), where
                print("%s: identity refit %s the built nodes" % (where, "equals" if r["built"].tobytes() == r["refit"].tobytes() else "is contained in"))


# ---- 8 ----
def _emissive_mesh(host):
    for m in range(host.get_num_meshes()):
        if any(host.get_material(int(i)).emission_active for i in set(host.get_mesh(m)[3])):
            return m
    raise AssertionError("no emissive mesh")


def _most_instanced_mesh(host):
    count = {}
    for i in range(host.get_num_instances()):
        m = host.get_instance(i).mesh_id
        count[m] = count.get(m, 0) + 1
    return max(count, key=lambda m: (count[m], -m))


def _zoo():
    return scenes.zoo_scene()


def _example():
    return scenes.example_scene(width=64, height=48, sphere_segments=8, ground_res=8, num_objects=8, num_lights=4)


class _MovedScenes:
    """The three successive edits of a scene and, per edit, a host that held the moved geometry before anything was encoded, its view and the oracle's render of it:
    computed once per scene, shared by the builders' cases, and closed with the module (the fixture below)."""

    def __init__(self):
        self._edits, self._steps, self._hosts = {}, {}, []

    def edits(self, which):
        """(mesh, positions) x 3: a plain mesh, an emissive one, then the first - by then refitted - mesh again."""
        if which not in self._edits:
            host = _example() if which == "example" else _zoo()
            try:
                first = _most_instanced_mesh(host) if which == "example" else 0
                lamp = _emissive_mesh(host)
                assert lamp != first
                p0, p1 = host.get_mesh(first)[0], host.get_mesh(lamp)[0]
            finally:
                host.close()
            once = bend(p0, 0.25, 0.0)
            self._edits[which] = [(first, once), (lamp, bend(p1, 0.25, 0.7)), (first, bend(once, 0.2, 1.9))]
        return self._edits[which]

    def steps(self, which):
        if which not in self._steps:
            out = []
            for k in range(3):
                host = _example() if which == "example" else _zoo()
                self._hosts.append(host)
                for mesh, pos in self.edits(which)[:k + 1]:
                    host.set_mesh_positions(mesh, pos)
                view = oracle_lib.with_luts(host.device_scene())
                out.append((view, oracle_lib.render(view, 0, 2)))
            self._steps[which] = out
        return self._steps[which]

    def close(self):
        self._steps.clear()
        for host in self._hosts:
            host.close()
        self._hosts = []


@pytest.fixture(scope="module")
def moved():
    scenes_ = _MovedScenes()
    yield scenes_
    scenes_.close()


def _render(core):
    core.set_pixels(None)
    core.reset_counters()
    core.render(0, 2, samples_per_pass=2)
    fm, sm = core.accumulators()
    return fm, sm, core.query_counters()[:4]


def _render_parity(moved, which, builder):
    make = _example if which == "example" else _zoo
    host = make()
    core, fresh = Core(0), Core(0)
    try:
        for c in (core, fresh):
            c.set_flavour("exact")
            c.set_bvh_builder(builder)
        core.upload(oracle_lib.with_luts(host.device_scene()))
        _render(core)
        for k, (mesh, pos) in enumerate(moved.edits(which)):
            where = "%s, %s, edit %d (mesh %d)" % (which, builder, k, mesh)
            host.set_mesh_positions(mesh, pos)
            core.update(oracle_lib.with_luts(host.device_scene()), DIRTY_MESH_POSITIONS | DIRTY_LIGHTS)
            stats = core.mesh_refit_stats()
            assert stats.last_refits == 1 and stats.last_rebuilds == 0 and stats.refits == k + 1, "%s: %d refits, %d rebuilds" % (where, stats.last_refits, stats.last_rebuilds)
            print("%s: cost growth %.3f, %.2f ms" % (where, stats.max_cost_growth, 1e3 * stats.seconds))
            fm, sm, cnt = _render(core)
            view, (ofm, osm, ocnt) = moved.steps(which)[k]
            _same(fm, ofm, where + ": first moment vs oracle")
            _same(sm, osm, where + ": second moment vs oracle")
            assert cnt == [int(x) for x in ocnt[:4]], "%s: ray counters %s, oracle %s" % (where, cnt, list(ocnt))
            fresh.upload(view)
            ffm, fsm, fcnt = _render(fresh)
            _same(fm, ffm, where + ": first moment vs a fresh upload")
            _same(sm, fsm, where + ": second moment vs a fresh upload")
            assert cnt == fcnt, where
            assert float(fm.max()) > 0.0
        assert not np.array_equal(moved.steps(which)[0][1][0], moved.steps(which)[2][1][0])
    finally:
        core.close(); fresh.close(); host.close()


@pytest.mark.parametrize("builder", BUILDERS)
def test_render_parity_after_three_moves_of_the_zoo(moved, builder):
    _render_parity(moved, "zoo", builder)


def test_render_parity_with_one_moved_mesh_under_several_instances(moved):
    _render_parity(moved, "example", "sah_gpu")


def test_the_host_api_renders_the_moved_scene_and_restarts_the_integration(moved):
    host = _zoo()
    try:
        host.render_samples(0, 2, samples_per_pass=2)
        assert host.is_rendering()[1] == 2
        for k, (mesh, pos) in enumerate(moved.edits("zoo")):
            host.set_mesh_positions(mesh, pos)
            assert host.is_rendering()[1] == 0, "the integration did not restart"
            host.render_samples(0, 2, samples_per_pass=2)
            fm, sm = host.accumulators()
            ofm, osm, _ = moved.steps("zoo")[k][1]
            _same(fm, ofm, "edit %d: first moment vs oracle" % k)
            _same(sm, osm, "edit %d: second moment vs oracle" % k)
            stats = host.mesh_refit_stats()
            assert stats["last_refits"] == 1 and stats["refits"] == k + 1 and stats["rebuilds"] == 0 and stats["max_cost_growth"] > 0.0, stats
    finally:
        host.close()


# ---- 9, 10: a soup as one mesh ----
def _soup_host(tris):
    host = Host()
    scenes.apply_benchmark_settings(host, 16, 16, 2, sky=(0.5, 0.5, 0.5))
    mat = host.add_material(scenes._material((0.6, 0.6, 0.6), 0.6))
    mesh = host.add_mesh(np.asarray(tris, dtype=np.float32).reshape(len(tris), 9), np.full(len(tris), mat, dtype=np.uint16))
    host.new_instance(mesh)
    scenes.set_camera(host, (0.0, 0.0, 30.0), (0.0, 0.0, 0.0))
    return host


def test_ray_queries_after_a_motion_unrelated_to_the_topology():
    n, rays = 7500, 4000
    tris, to = motions(n)
    moved = to["fresh draw"]
    host = _soup_host(tris)
    core = Core(0)
    try:
        core.set_flavour("exact")
        core.upload(oracle_lib.with_luts(host.device_scene()))
        host.set_mesh_positions(0, moved.reshape(n, 9))
        view = oracle_lib.with_luts(host.device_scene())
        core.update(view, DIRTY_MESH_POSITIONS | DIRTY_LIGHTS)
        stats = core.mesh_refit_stats()
        assert stats.last_refits == 1 and stats.last_rebuilds == 0
        rng = np.random.RandomState(9)
        tgt = _targets(rng, moved, rng.randint(0, n, rays))
        d = _normalise32(rng.normal(size=(rays, 3)))
        o = (tgt - rng.uniform(1.0, 20.0, (rays, 1)) * d.astype(np.float64)).astype(np.float32)
        want = oracle_lib.trace_closest(view, o, d, None, use_bvh=False)
        exact = core.trace_closest_host(o, d)
        assert (want[:, 0] != ray_truth.SKY).mean() > 0.9, "the rays must hit what they are aimed at"
        _same(exact, want, "closest hits over the refitted tree (cost x %.2f) vs the oracle's brute force" % stats.max_cost_growth)
        hit = want[:, 0] != ray_truth.SKY
        open_ = hit & (np.arange(rays) % 2 == 0)  # even rays: up to the hit point with the hit triangle as the target; odd rays: 1 % past it, no target - blocked
        t_hit = want[:, 2].copy().view(np.float32)
        dist = np.where(hit, np.where(open_, t_hit, t_hit * np.float32(1.01)), np.float32(50.0)).astype(np.float32)
        ids = np.full((rays, 4), NONE, dtype=np.uint32)
        ids[open_, 0:2] = want[open_, 0:2]
        vis = core.trace_visibility_host(o, d, dist, ids)
        _same(vis, oracle_lib.trace_shadow(view, o, d, dist, ids, use_bvh=False), "visibility of the segments to the hit points vs the oracle's brute force")
        assert (vis == 0.0).all(axis=1).any() and (vis != 0.0).all(axis=1).any(), "both answers must occur"
        core.set_flavour("fast")
        fast = core.trace_closest_host(o, d)
        sol = ray_truth.solve(ray_truth.scene_of_view(view), o, d)
        ok, why = sol.check(fast)
        print("fast flavour over the refitted tree: %d rays, decisive share %.4f, %d rejected" % (rays, sol.decisive.mean(), int((~ok).sum())))
        assert ok.all(), list(why[~ok][:5])
    finally:
        core.close(); host.close()


def test_modes_thresholds_and_the_tree_cache():
    n = 257
    tris, to = motions(n)
    small = bend(tris.reshape(n, 9), 0.02).reshape(n, 3, 3)
    host = _soup_host(tris)
    a, b, fresh = Core(0), Core(0), Core(0)
    try:
        for c in (a, b, fresh):
            c.set_flavour("exact")
            c.set_bvh_builder("sah")
        original = oracle_lib.with_luts(host.device_scene())
        want_original = oracle_lib.render(original, 0, 2)
        a.upload(original)
        b.upload(original)  # takes a's tree from the process's cache
        nodes_original = a.bvh_stats()[0]
        assert b.bvh_stats()[0] == nodes_original

        def move(core, tris_to, mode, growth):
            host.set_mesh_positions(0, np.asarray(tris_to, np.float32).reshape(n, 9))
            view = oracle_lib.with_luts(host.device_scene())
            core.set_mesh_refit(mode, growth)
            core.update(view, DIRTY_MESH_POSITIONS | DIRTY_LIGHTS)
            s = core.mesh_refit_stats()
            fm, sm, cnt = _render(core)
            ofm, osm, ocnt = oracle_lib.render(view, 0, 2)
            _same(fm, ofm, "mode %d, growth %g: first moment vs oracle" % (mode, growth))
            _same(sm, osm, "second moment vs oracle")
            assert cnt == [int(x) for x in ocnt[:4]]
            return view, s

        # mode 0, no threshold: a refit, however bad; the node count cannot change
        view, s = move(a, to["half moved by 1e4"], 0, 0.0)
        assert (s.last_refits, s.last_rebuilds) == (1, 0) and s.max_cost_growth > 1e3 and a.bvh_stats()[0] == nodes_original
        # the other context still renders the original scene from the shared tree, which nobody wrote
        fm, sm, cnt = _render(b)
        _same(fm, want_original[0], "the second context after the first one's refit")
        _same(sm, want_original[1], "second moment")
        # a refitted tree never enters the cache: a fresh upload of the moved vertices builds
        fresh.upload(view)
        nodes_moved = fresh.bvh_stats()[0]
        # ... which the builder itself says, without the cache: the host SAH builder's tree over the moved boxes has another node count than the refitted
        # one (which keeps the original's), so a refitted tree taken from the cache would show here and in the threshold rebuild below
        built_alone = bvh_refit_probe(boxes_of(to["half moved by 1e4"]), boxes_of(to["half moved by 1e4"]), "sah", on_gpu=False)["built"].shape[0]
        print("nodes: %d as built for the original vertices, %d as built for the moved ones (builder alone: %d)" % (nodes_original, nodes_moved, built_alone))
        assert built_alone != nodes_original, "the motion must change the built tree's size, or the next line proves nothing"
        assert nodes_moved == built_alone, "a fresh upload of the moved vertices did not get a built tree"
        # back to the original vertices, threshold 2: the cost falls back to the built tree's - a refit (growth exactly 1: the identity)
        _, s = move(a, tris, 0, 2.0)
        assert (s.last_refits, s.last_rebuilds) == (1, 0) and s.max_cost_growth == 1.0
        # ... a small bend stays a refit, half the triangles 1e4 away is built again
        _, s = move(a, small, 0, 2.0)
        assert (s.last_refits, s.last_rebuilds) == (1, 0) and 0.0 < s.max_cost_growth <= 2.0, s.max_cost_growth
        _, s = move(a, to["half moved by 1e4"], 0, 2.0)
        assert (s.last_refits, s.last_rebuilds) == (0, 1) and s.max_cost_growth > 2.0
        assert a.bvh_stats()[0] == nodes_moved, "the rebuilt tree is the one an upload of these vertices builds"
        # mode 1: always built again
        view, s = move(a, small, 1, 0.0)
        assert (s.last_refits, s.last_rebuilds) == (0, 1) and s.rebuilds == 2 and s.refits == 3
        fresh.upload(view)
        assert a.bvh_stats()[0] == fresh.bvh_stats()[0]
        # a later fresh upload of the original vertices: the original tree
        host.set_mesh_positions(0, tris.reshape(n, 9))
        fresh.upload(oracle_lib.with_luts(host.device_scene()))
        assert fresh.bvh_stats()[0] == nodes_original
        fm, sm, _ = _render(fresh)
        _same(fm, want_original[0], "a fresh upload of the original vertices")
    finally:
        a.close(); b.close(); fresh.close(); host.close()
