"""Deformable meshes refitted where the nodes live: lumc_set_mesh_refit_in_place -> csrc/host/bvh_refit.hip k_refit_level_resident, scene_device.hip refit_in_place.

With the switch on, a LUMC_DIRTY_MESH_POSITIONS update - alone or with LUMC_DIRTY_INSTANCE_TRANSFORMS - rewrites the moved meshes' boxes in [C, C + M) of the resident node
array and rebuilds only the top level: no re-layout, no fallback, a few dozen bytes back. What it leaves in the array is held, byte for byte, to what the long way round
leaves there (the refit in a copy of the tree, the host's assembly, a re-layout), what is rendered over it to the CPU oracle bit for bit, and the host's copies of the
nodes - stale after such a refit - to the updates that read them next."""
import functools
import math

import numpy as np
import pytest

import oracle_lib
from luminary_amd import Host, scenes
from luminary_amd.core import DIRTY_INSTANCE_TRANSFORMS, DIRTY_INSTANCES, DIRTY_LIGHTS, DIRTY_MESH_POSITIONS, Core, CoreError, bvh_refit_probe
from test_instance_transforms_api import moved_instances
from test_instance_update_gpu import _against_oracle, _canonical, _same, _single, _zoo
from test_mesh_positions_api import bend
from test_mesh_refit import boxes_of, soup

pytestmark = pytest.mark.gpu
EMPTY, LEAF = 0xFFFFFFFF, 0x80000000
MOVED = DIRTY_INSTANCE_TRANSFORMS | DIRTY_LIGHTS
BENT = DIRTY_MESH_POSITIONS | DIRTY_LIGHTS
BOTH = DIRTY_MESH_POSITIONS | DIRTY_INSTANCE_TRANSFORMS | DIRTY_LIGHTS


def _small_zoo():
    return _zoo(48, 32, 3)


def _emissive_mesh(host):
    for m in range(host.get_num_meshes()):
        if any(host.get_material(int(i)).emission_active for i in set(host.get_mesh(m)[3])):
            return m
    raise AssertionError("no emissive mesh")


def _view(host):
    return oracle_lib.with_luts(host.device_scene())


def _core(builder=None, in_place=1):
    core = Core(0)
    core.set_flavour("exact")
    if builder:
        core.set_bvh_builder(builder)
    core.set_mesh_refit_in_place(in_place)
    return core


def _widths(nodes, root=0, base=0):
    """Nodes per depth below row `root` of a node array ([nodes, 32] words; an inner child word c names row c - base), and the rows reached."""
    level, out, reached = [root], [], []
    while level:
        out.append(len(level)); reached += level
        level = [int(c) - base for n in level for c in nodes[n, 24:28] if c != EMPTY and not (c & LEAF)]
    return out, reached


def _cost(nodes, rows):
    """bvh_build.cpp bvh4_cost over the rows of a node array, every term as the host computes it, summed exactly (math.fsum)."""
    f = nodes.view(np.float32)[rows].astype(np.float64)
    occupied = nodes[rows, 24:28] != EMPTY
    dx, dy, dz = f[:, 12:16] - f[:, 0:4], f[:, 16:20] - f[:, 4:8], f[:, 20:24] - f[:, 8:12]
    terms = dx * dy + dy * dz + dz * dx
    return math.fsum(terms[occupied].tolist())


def _counts(core):
    i, r = core.instance_update_stats(), core.resident_refit_stats()
    return {"relayouts": i.relayouts, "instance fallbacks": i.fallbacks, "updates": r.updates, "fallbacks": r.fallbacks}


# ---- fails without the feature ----
def test_three_updates_in_place_keep_the_layout_and_render_like_the_oracle():
    host, core = _small_zoo(), _core()
    try:
        core.upload(_view(host))
        host.set_instance_transforms(moved_instances(host, 0))
        core.update(_view(host), MOVED)
        assert _counts(core) == {"relayouts": 1, "instance fallbacks": 0, "updates": 0, "fallbacks": 0}
        n, nm = host.get_num_instances(), host.get_num_meshes()
        a, b = 1, _emissive_mesh(host)
        assert a != b
        pa, pb = host.get_mesh(a)[0], host.get_mesh(b)[0]
        before = core.resident_mesh_nodes_probe()
        roots = core.resident_tree_probe(n, nm)["mesh_root"]
        steps = [("one mesh bent", BENT, {a: bend(pa, 0.2, 0.4)}, None), ("two meshes bent, instances moved", BOTH, {a: bend(pa, 0.25, 1.1), b: bend(pb, 0.2, 0.7)}, 1),
                 ("bent back", BENT, {a: pa, b: pb}, None)]
        images = []
        for k, (where, flags, meshes, move) in enumerate(steps):
            for mesh, positions in meshes.items():
                host.set_mesh_positions(mesh, positions)
            if move is not None:
                host.set_instance_transforms(moved_instances(host, move))
            view = _view(host)
            core.update(view, flags)
            stats, refit = core.resident_refit_stats(), core.mesh_refit_stats()
            print("%s: %d meshes, %d launches, %d bytes back, growth %.4f | %.3f ms: upload %.3f, hashes %.3f, refit %.3f, cost %.3f, top level %.3f" % (
                where, stats.last_meshes, stats.last_launches, stats.last_bytes_downloaded, refit.max_cost_growth, 1e3 * stats.seconds, 1e3 * stats.seconds_upload,
                1e3 * stats.seconds_hash, 1e3 * stats.seconds_refit, 1e3 * stats.seconds_cost, 1e3 * stats.seconds_top_level))
            assert _counts(core) == {"relayouts": 1, "instance fallbacks": 0, "updates": k + 1, "fallbacks": 0}, where
            assert stats.last_meshes == len(meshes) and refit.last_refits == len(meshes) and refit.last_rebuilds == 0, where
            assert 0 < stats.last_bytes_downloaded < 1024 and stats.last_launches <= len(meshes) + 27 + 3, where
            probe = core.resident_tree_probe(n, nm)
            assert np.array_equal(probe["mesh_root"], roots), where
            images.append(_against_oracle(core, view, where))
        assert not np.array_equal(images[0], images[2]) and not np.array_equal(images[0], images[1])
        after = core.resident_mesh_nodes_probe()
        assert after.tobytes() == before.tobytes(), "bent back: %d node words differ from those before the first bend" % int((after != before).sum())
    finally:
        core.close(); host.close()


# ---- same bytes as the long way round ----
def _same_layout(a, b, host, where):
    n, nm = host.get_num_instances(), host.get_num_meshes()
    pa, pb = a.resident_tree_probe(n, nm), b.resident_tree_probe(n, nm)
    assert (pa["C"], pa["M"], pa["T"], pa["depth"]) == (pb["C"], pb["M"], pb["T"], pb["depth"]), where
    assert np.array_equal(pa["mesh_root"], pb["mesh_root"]), where
    na, nb = a.resident_mesh_nodes_probe(), b.resident_mesh_nodes_probe()
    assert na.tobytes() == nb.tobytes(), "%s: %d words of [C, C + M) differ, in nodes %s" % (where, int((na != nb).sum()), np.nonzero((na != nb).any(axis=1))[0][:8])
    assert pa["leaves"].tobytes() == pb["leaves"].tobytes(), where + ": leaf records"
    ca, cb = _canonical(pa["top"][:pa["T"]]), _canonical(pb["top"][:pb["T"]])  # (a level's nodes are numbered through atomics: compared as trees)
    assert ca[1] == cb[1] and np.array_equal(ca[0], cb[0]), where + ": top level"
    return pa, na


def _both_ways(host, builder, edits, where):
    """`edits`: [(flags, {mesh: positions}, step of moved_instances or None)]. One context takes them in place, its twin the long way round; then both take one
    moved-instances update (the twin re-lays out) and must hold the same bytes. Returns the in-place context's probe and mesh nodes; closes both."""
    a, b = _core(builder, 1), _core(builder, 0)
    try:
        first = _view(host)
        a.upload(first); b.upload(first)  # (the shared tree cache gives both contexts one topology)
        host.set_instance_transforms(moved_instances(host, 0))
        view = _view(host)
        a.update(view, MOVED); b.update(view, MOVED)
        for flags, meshes, move in edits:
            for mesh, positions in meshes.items():
                host.set_mesh_positions(mesh, positions)
            if move is not None:
                host.set_instance_transforms(moved_instances(host, move))
            view = _view(host)
            a.update(view, flags); b.update(view, flags)
        ra, rb = a.mesh_refit_stats(), b.mesh_refit_stats()
        assert (ra.refits, ra.rebuilds) == (rb.refits, rb.rebuilds) and ra.rebuilds == 0, where
        assert _counts(a) == {"relayouts": 1, "instance fallbacks": 0, "updates": len(edits), "fallbacks": 0}, (where, _counts(a))
        assert _counts(b)["updates"] == 0 and _counts(b)["fallbacks"] == 0, where
        _against_oracle(a, view, where, {"the long way round": b})
        host.set_instance_transforms(moved_instances(host, 2))
        view = _view(host)
        a.update(view, MOVED); b.update(view, MOVED)
        assert _counts(a)["relayouts"] == 1 and _counts(b)["relayouts"] == 2, where  # (the twin's layout went with the first moved vertices)
        return _same_layout(a, b, host, where)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("builder", ["sah", None])
def test_same_bytes_as_the_long_way_round(builder):
    host = _small_zoo()
    try:
        m0, m1 = 1, _emissive_mesh(host)
        p0, p1 = host.get_mesh(m0)[0], host.get_mesh(m1)[0]
        edits = [(BENT, {m0: bend(p0, 0.2, 0.4)}, None), (BOTH, {m0: bend(p0, 0.25, 1.1), m1: bend(p1, 0.2, 0.7)}, 1), (BENT, {m0: bend(p0, 0.1, 2.0)}, None)]
        _both_ways(host, builder, edits, "zoo, builder %s" % (builder or "default"))
    finally:
        host.close()


# ---- shapes ----
@functools.lru_cache(maxsize=None)
def _soup_of_width(width):
    """A soup whose host-built tree has `width` nodes at its widest depth (found by a search over seeds; the host builder is deterministic)."""
    for seed in range(400):
        tris = soup(np.random.RandomState(100000 + seed), 3000 + seed % 60)
        if max(_widths(bvh_refit_probe(boxes_of(tris), boxes_of(tris), "sah")["built"])[0]) == width:
            return tris
    raise AssertionError("no soup whose widest depth has %d nodes" % width)


def _soups_host(soups, unused):
    host = Host()
    scenes.apply_benchmark_settings(host, 48, 32, 2, sky=(0.5, 0.5, 0.5))
    mat = host.add_material(scenes._material((0.6, 0.6, 0.6), 0.6))
    for k, tris in enumerate(soups):
        mesh = host.add_mesh(np.asarray(tris, dtype=np.float32).reshape(len(tris), 9), np.full(len(tris), mat, dtype=np.uint16))
        if k not in unused:
            host.new_instance(mesh, position=(1.5 * k - 4.0, 0.5 * (k % 3), -0.7 * k), rotation=(0.1 * k, 0.2, 0.0), scale=(1.0, 1.0 + 0.05 * k, 1.0))
    scenes.set_camera(host, (0.0, 0.0, 34.0), (0.0, 0.0, 0.0))
    return host


def test_shapes_of_meshes_in_one_update():
    """One node; two nodes one below the other; widest depths of 255, 256 and 257 nodes (either side of a workgroup of 256); 30 000 triangles, whose slots are
    split between the tops of all meshes and the rest; a mesh no instance uses. All seven move in one update: every depth launch covers meshes of other depths."""
    rng = np.random.RandomState(3)
    soups = [soup(rng, 2), soup(np.random.RandomState(9), 9), _soup_of_width(255), _soup_of_width(256), _soup_of_width(257), soup(rng, 30000), soup(rng, 300)]
    host = _soups_host(soups, unused={6})
    try:
        moved = {m: bend(host.get_mesh(m)[0], 0.15, 0.3 * m) for m in range(len(soups))}
        probe, nodes = _both_ways(host, "sah", [(BENT, moved, None)], "soups")
        C, roots = probe["C"], probe["mesh_root"]
        widths, slots = zip(*[_widths(nodes, int(r) - C, C) for r in roots])
        print("nodes per depth: %s" % [list(w) if len(w) < 4 else "%d depths, widest %d" % (len(w), max(w)) for w in widths])
        assert widths[0] == [1] and widths[1] == [1, 1] and [max(w) for w in widths[2:5]] == [255, 256, 257]
        assert len({len(w) for w in widths}) >= 4, "meshes of different depths in one update"
        big = np.sort(np.array(slots[5]))
        assert big[-1] - big[0] + 1 > len(big) and big[0] < 4096 - C <= big[-1], "the large mesh's slots are one range: the split case did not occur"
        assert sum(len(s) for s in slots) == probe["M"]
    finally:
        host.close()


# ---- host copies ----
def test_stale_host_copies_are_brought_back_before_they_are_read():
    host, core = _small_zoo(), _core()
    try:
        core.upload(_view(host))
        host.set_instance_transforms(moved_instances(host, 0))
        view = _view(host)
        core.update(view, MOVED)
        unbent = _against_oracle(core, view, "before the bend")
        mesh = 1
        host.set_mesh_positions(mesh, bend(host.get_mesh(mesh)[0], 0.6, 0.4))
        view = _view(host)
        core.update(view, BENT)
        assert _counts(core) == {"relayouts": 1, "instance fallbacks": 0, "updates": 1, "fallbacks": 0}
        bent = _against_oracle(core, view, "bent in place")
        assert int((bent != unbent).sum()) > 20, "the bend must change the image, or stale boxes would not show"
        # a new instance of the bent mesh: the host assembles the scene tree from its copies of the nodes
        host.new_instance(mesh, position=(0.3, 1.4, -0.2), rotation=(0.1, 0.7, 0.0), scale=(0.8, 0.8, 0.8))
        view = _view(host)
        core.update(view, DIRTY_INSTANCES | DIRTY_LIGHTS)
        with pytest.raises(CoreError):
            core.resident_tree_probe(view.num_instances, view.num_meshes)
        _against_oracle(core, view, "a new instance after a refit in place")
        # the switch off, another bend: the other path refits the tree it holds
        core.set_mesh_refit_in_place(0)
        host.set_mesh_positions(mesh, bend(host.get_mesh(mesh)[0], 0.3, 1.3))
        view = _view(host)
        core.update(view, BENT)
        stats = core.mesh_refit_stats()
        assert (stats.last_refits, stats.last_rebuilds) == (1, 0) and core.resident_refit_stats().updates == 1
        _against_oracle(core, view, "the switch off, bent again")
        # ... and on again with the nodes stale when the switch goes off: the other path reads them
        core.set_mesh_refit_in_place(1)
        host.set_mesh_positions(mesh, bend(host.get_mesh(mesh)[0], 0.4, 2.2))
        view = _view(host)
        core.update(view, BENT)
        assert core.resident_refit_stats().updates == 2
        core.set_mesh_refit_in_place(0)
        host.set_mesh_positions(mesh, bend(host.get_mesh(mesh)[0], 0.2, 0.1))
        view = _view(host)
        core.update(view, BENT)
        assert core.mesh_refit_stats().last_refits == 1
        _against_oracle(core, view, "stale nodes read by the other path's refit")
    finally:
        core.close(); host.close()


# ---- cost and fallback ----
def test_the_device_s_cost_and_the_fallback_beyond_the_threshold():
    host, core = _small_zoo(), _core()
    try:
        core.upload(_view(host))
        host.set_instance_transforms(moved_instances(host, 0))
        core.update(_view(host), MOVED)
        n, nm = host.get_num_instances(), host.get_num_meshes()
        mesh = 1
        original = host.get_mesh(mesh)[0]
        moved = bend(original, 0.5, 0.4)
        probe = core.resident_tree_probe(n, nm)
        rows = _widths(core.resident_mesh_nodes_probe(), int(probe["mesh_root"][mesh]) - probe["C"], probe["C"])[1]
        built = _cost(core.resident_mesh_nodes_probe(), rows)
        host.set_mesh_positions(mesh, moved)
        core.update(_view(host), BENT)
        growth = core.mesh_refit_stats().max_cost_growth
        want = _cost(core.resident_mesh_nodes_probe(), rows) / built
        bound = 2.0 * len(rows) * 2.0 ** -53
        print("mesh %d, %d nodes: growth on the device %.17g, from the probed nodes %.17g, relative difference %.3g, bound %.3g" % (mesh, len(rows), growth, want, abs(growth / want - 1.0), bound))
        assert growth > 1.05, "the bend must grow the cost for the threshold below"
        assert abs(growth / want - 1.0) <= bound
        # back (the built boxes again: growth 1 up to the order of the additions), then the same bend under a threshold it exceeds
        host.set_mesh_positions(mesh, original)
        core.update(_view(host), BENT)
        assert abs(core.mesh_refit_stats().max_cost_growth - 1.0) <= bound and _counts(core) == {"relayouts": 1, "instance fallbacks": 0, "updates": 2, "fallbacks": 0}
        core.set_mesh_refit(0, 0.5 * (1.0 + growth))
        host.set_mesh_positions(mesh, moved)
        view = _view(host)
        core.update(view, BENT)
        stats = core.mesh_refit_stats()
        assert (stats.last_refits, stats.last_rebuilds) == (0, 1) and stats.max_cost_growth > 0.5 * (1.0 + growth)
        assert _counts(core) == {"relayouts": 1, "instance fallbacks": 0, "updates": 2, "fallbacks": 1}
        with pytest.raises(CoreError):
            core.resident_tree_probe(n, nm)
        _against_oracle(core, view, "the fallback")
        # the next update runs in place again, after one re-layout
        core.set_mesh_refit(0, 0.0)
        host.set_mesh_positions(mesh, bend(original, 0.2, 1.0))
        view = _view(host)
        core.update(view, BENT)
        assert _counts(core) == {"relayouts": 2, "instance fallbacks": 0, "updates": 3, "fallbacks": 1}
        core.resident_tree_probe(n, nm)
        _against_oracle(core, view, "in place again")
    finally:
        core.close(); host.close()


# ---- public API ----
def test_the_host_api_moves_vertices_and_instances_in_one_frame():
    host = _small_zoo()
    try:
        host.set_mesh_refit_in_place(1)
        host.render_samples(0, 2, samples_per_pass=2)
        assert host.is_rendering()[1] == 2
        mesh = 1
        original = host.get_mesh(mesh)[0]
        for step in range(2):
            host.set_mesh_positions(mesh, bend(original, 0.25, 0.5 * step))
            host.set_instance_transforms(moved_instances(host, step))
            assert host.is_rendering()[1] == 0, "the integration did not restart"
            host.render_samples(0, 2, samples_per_pass=2)
            fm, sm = host.accumulators()
            ofm, osm, _ = oracle_lib.render(_view(host), 0, 2)
            _same(fm, ofm, "frame %d: first moment vs oracle" % step)
            _same(sm, osm, "frame %d: second moment vs oracle" % step)
            stats = host.resident_refit_stats()
            assert (stats["updates"], stats["fallbacks"], stats["last_meshes"]) == (step + 1, 0, 1), stats
            assert host.instance_update_stats()["relayouts"] == 1 and host.mesh_refit_stats()["refits"] == step + 1
    finally:
        host.close()


# ---- refusals ----
def test_refusals():
    host, other, core = _small_zoo(), _single(), _core()
    try:
        with pytest.raises(CoreError, match="lumc_set_mesh_refit_in_place"):
            core.set_mesh_refit_in_place(2)
        core.upload(_view(host))
        with pytest.raises(CoreError, match="no resident layout"):
            core.resident_mesh_nodes_probe()
        with pytest.raises(CoreError, match="LUMC_DIRTY_MESH_POSITIONS with other meshes or triangle counts"):
            core.update(_view(other), BENT)
    finally:
        core.close(); host.close(); other.close()
