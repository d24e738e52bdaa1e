"""Moving instances on the device: luminary_ext_set_instance_transforms -> LUMC_DIRTY_INSTANCE_TRANSFORMS -> csrc/host/instance_update.hip.

The device's rows and world boxes are held to the host's functions byte for byte; the top level it builds into the resident node array is checked in numpy - and,
where no two instance centroids coincide, held to the host builder's tree; what is rendered and traced over it is held to the CPU oracle bit for bit, as everything
in the exact flavour is - its images do not depend on the trees -, to a fresh upload of the moved scene and to the float64 truth of
tests/ray_truth.py. The GPU builders number a level's nodes through atomics, so two trees are compared as trees: both renumbered breadth first, child slot by
child slot, from the root - the boxes, the child words and the leaf order then have to agree bit for bit."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import ray_truth
from luminary_amd import DeviceSceneView, Host, Vec3, scenes
from luminary_amd.core import DIRTY_INSTANCE_TRANSFORMS, DIRTY_INSTANCES, DIRTY_LIGHTS, DIRTY_MESH_POSITIONS, Core, CoreError, host_bvh_nodes_probe, instance_boxes_probe
from test_instance_transforms_api import moved_instances
from test_mesh_positions_api import bend
from test_ray_truth import _axis_parallel_rays, _instance_world, _normalise32, _targets

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
EMPTY, LEAF = 0xFFFFFFFF, 0x80000000
FLT_MAX = np.float32(3.4028234663852886e38)
MOVED = DIRTY_INSTANCE_TRANSFORMS | DIRTY_LIGHTS


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: %d of %d values differ" % (what, int((a.view(np.uint32) != b.view(np.uint32)).sum()), a.size)


# ---- rows and boxes, byte for byte ----
def _quaternion_words(rng, identity=False):
    q = np.array([0.0, 0.0, 0.0, 1.0]) if identity else rng.normal(size=4)
    q /= np.linalg.norm(q)
    w = np.round((q + 1.0) * 0x7FFF).astype(np.uint32)
    return np.array([w[0] | (w[1] << 16), w[2] | (w[3] << 16)], dtype=np.uint32)


KINDS = ["identity", "rotated", "scaled", "negative scale", "zero scale", "far away", "empty mesh", "mesh id out of range", "no mesh"]
NOT_HITTABLE = {"zero scale", "empty mesh", "mesh id out of range", "no mesh"}


def _probe_view(n, shift):
    """A view of n instances over three meshes (the third empty), instance i of kind KINDS[(i + shift) % 9]; returns (view, mesh boxes, kinds)."""
    rng = np.random.RandomState(1000 * n + shift)
    offsets = np.array([0, 10, 30, 30], dtype=np.uint32)
    mesh_boxes = np.float32([[-1.0, -0.5, -2.0, 1.5, 0.75, 2.0], [3.0, -4.0, 0.0, 3.5, 9.0, 0.25], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    ids = np.zeros(n, dtype=np.uint32)
    t = np.zeros((n, 8), dtype=np.float32)
    kinds = []
    for i in range(n):
        kind = KINDS[(i + shift) % len(KINDS)]
        kinds.append(kind)
        ids[i] = rng.randint(0, 2)
        pos, scale, words = rng.uniform(-20.0, 20.0, 3), np.ones(3), _quaternion_words(rng, kind == "identity")
        if kind == "identity":
            pos = np.zeros(3)
        elif kind == "scaled":
            scale = 10.0 ** rng.uniform(-3.0, 3.0, 3)
            scale[rng.randint(0, 3)] = [1e-3, 1e3][i % 2]
        elif kind == "negative scale":
            scale = rng.uniform(0.5, 2.0, 3) * [1.0, -1.0, 1.0]
        elif kind == "zero scale":
            scale[rng.randint(0, 3)] = 0.0
        elif kind == "far away":
            pos = rng.choice([-1e6, 1e6], 3) + rng.uniform(-1.0, 1.0, 3)
        elif kind == "empty mesh":
            ids[i] = 2
        elif kind == "mesh id out of range":
            ids[i] = 3 + rng.randint(0, 5)
        elif kind == "no mesh":
            ids[i] = NONE
        t[i, 0:3], t[i, 3:6] = pos, scale
        t[i, 6:8] = words.view(np.float32)
    view = DeviceSceneView()
    view.num_meshes, view.num_instances = 3, n
    view.mesh_tri_offset, view.instance_mesh_ids, view.instance_transforms = offsets.ctypes.data, ids.ctypes.data, t.ctypes.data
    view._keep = (offsets, ids, t)
    return view, mesh_boxes, kinds


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_rows_and_boxes_of_the_kernel_are_the_host_functions_byte_for_byte(n):
    seen = set()
    for shift in (range(len(KINDS)) if n < len(KINDS) else (0, 4)):
        view, mesh_boxes, kinds = _probe_view(n, shift)
        h_rows, h_boxes, h_flags = instance_boxes_probe(view, mesh_boxes, on_gpu=False)
        d_rows, d_boxes, d_flags = instance_boxes_probe(view, mesh_boxes, on_gpu=True)
        where = "n = %d, shift %d" % (n, shift)
        assert np.array_equal(h_flags, d_flags), "%s: flags differ at %s" % (where, np.nonzero(h_flags != d_flags)[0][:8])
        _same(d_rows, h_rows, where + ": rows")
        _same(d_boxes, h_boxes, where + ": boxes")
        for i, kind in enumerate(kinds):
            assert bool(h_flags[i]) == (kind not in NOT_HITTABLE), "%s: instance %d (%s) flagged %d" % (where, i, kind, h_flags[i])
        hit = h_flags.astype(bool)
        assert np.isfinite(h_boxes[hit]).all() and (h_boxes[hit, :3] < h_boxes[hit, 3:]).all() and not h_boxes[~hit].any()
        seen |= set(kinds)
    assert seen == set(KINDS)


# ---- the tree ----
def _zoo(width=96, height=64, bounces=8):
    return scenes.zoo_scene(width, height, bounces)


def _example():
    return scenes.example_scene(width=96, height=64, sphere_segments=6, ground_res=8)


def _single():
    rng = np.random.RandomState(12)
    host = Host()
    scenes.apply_benchmark_settings(host, 16, 16, 2, sky=(0.5, 0.5, 0.5))
    mat = host.add_material(scenes._material((0.6, 0.6, 0.6), 0.6))
    tris = (rng.uniform(-3.0, 3.0, (60, 1, 3)) + rng.normal(size=(60, 3, 3)) * 0.5).astype(np.float32)
    host.new_instance(host.add_mesh(tris.reshape(60, 9), np.full(60, mat, dtype=np.uint16)))
    scenes.set_camera(host, (0.0, 0.0, 12.0), (0.0, 0.0, 0.0))
    return host


MAKE = {"zoo": _zoo, "example": _example, "single": _single}


def _mesh_boxes(host):
    out = np.zeros((host.get_num_meshes(), 6), np.float32)
    for m in range(host.get_num_meshes()):
        p = host.get_mesh(m)[0].reshape(-1, 3)
        if len(p):
            out[m] = np.concatenate([p.min(axis=0), p.max(axis=0)])
    return out


def _canonical(nodes):
    """The tree of a node array ([nodes, 32] words) renumbered breadth first from node 0: ([reached nodes, 28] words with renumbered inner children, depth)."""
    order, index, depth = [0], {0: 0}, 0
    level = [0]
    while level:
        depth += 1
        nxt = []
        for n in level:
            for c in nodes[n, 24:28]:
                c = int(c)
                if c != EMPTY and not (c & LEAF):
                    assert c < len(nodes) and c not in index, "inner child %d out of range or reached twice" % c
                    index[c] = len(order); order.append(c); nxt.append(c)
        level = nxt
    out = nodes[order, :28].copy()
    for row in out:
        for k in range(24, 28):
            c = int(row[k])
            if c != EMPTY and not (c & LEAF):
                row[k] = index[c]
    return out, depth


def _check_tree(core, host, view, where, mesh_boxes):
    n, nm = view.num_instances, view.num_meshes
    probe = core.resident_tree_probe(n, nm)
    stats = core.instance_update_stats()
    rows, boxes, hittable = instance_boxes_probe(view, mesh_boxes, on_gpu=False)
    mesh_ids = oracle_lib.view_arrays(view)["instance_mesh_ids"]
    ids = np.nonzero(hittable)[0]
    h, T, cap = len(ids), probe["T"], probe["C"]
    assert cap == max(1, n - 1) and 1 <= T <= cap and stats.tlas_nodes == T and stats.tlas_capacity == cap and stats.hittable == h and stats.tlas_depth == probe["depth"], where
    assert core.bvh_stats()[2] == T and core.bvh_stats()[0] == probe["M"]
    # the leaf records: every instance that can be hit exactly once, its rows, the root of its mesh; one record of padding
    leaves = probe["leaves"]
    assert leaves.shape[0] == h + 1 and not leaves[h].any(), where
    order = leaves[:h, 3, 0]
    assert sorted(order.tolist()) == ids.tolist(), "%s: the leaves do not hold every instance that can be hit exactly once" % where
    _same(leaves[:h, 0:3, :], rows[order].view(np.uint32), where + ": leaf rows")
    assert np.array_equal(leaves[:h, 3, 1], probe["mesh_root"][mesh_ids[order]]) and not leaves[:h, 3, 2:].any(), where
    assert (probe["mesh_root"] >= cap).all() and (probe["mesh_root"] < cap + max(probe["M"], 1)).all(), where
    # the nodes [0, T): every leaf once, inner children < T and reached once, boxes hold what is below them
    top = probe["top"]
    canon, depth = _canonical(top[:T])
    assert len(canon) == T, "%s: %d of %d top-level nodes are reached from the root" % (where, len(canon), T)
    assert depth <= 16 and depth == probe["depth"], where
    f = top.view(np.float32)
    below = {}
    def box_below(node):
        if node in below:
            return below[node]
        all_lo, all_hi = np.full(3, np.inf), np.full(3, -np.inf)
        for k in range(4):
            c = int(top[node, 24 + k])
            if c == EMPTY:
                assert (f[node, [k, 4 + k, 8 + k]] == FLT_MAX).all() and (f[node, [12 + k, 16 + k, 20 + k]] == -FLT_MAX).all(), "%s: empty slot with a box" % where
                continue
            if c & LEAF:
                assert (c >> 28) & 7 == 0 and (c & 0x0FFFFFFF) < h, "%s: leaf word %#x" % (where, c)
                seen_leaves.append(c & 0x0FFFFFFF)
                b = boxes[order[c & 0x0FFFFFFF]].astype(np.float64)
                lo, hi = b[:3], b[3:]
            else:
                assert c < T
                lo, hi = box_below(c)
            clo, chi = f[node, [k, 4 + k, 8 + k]].astype(np.float64), f[node, [12 + k, 16 + k, 20 + k]].astype(np.float64)
            assert (clo <= lo).all() and (chi >= hi).all(), "%s: node %d slot %d does not hold what is below it" % (where, node, k)
            all_lo, all_hi = np.minimum(all_lo, lo), np.maximum(all_hi, hi)
        below[node] = (all_lo, all_hi)
        return below[node]
    seen_leaves = []
    box_below(0)
    assert sorted(seen_leaves) == list(range(h)), "%s: the nodes do not reach every leaf exactly once" % where
    # slots [T, C) are empty
    assert (top[T:, 24:28] == EMPTY).all() and (f[T:, 0:12] == FLT_MAX).all() and (f[T:, 12:24] == -FLT_MAX).all(), "%s: a slot behind the top level is not empty" % where
    # the host builder's tree over the same boxes
    centres = (boxes[ids, :3] + boxes[ids, 3:]) * np.float32(0.5)
    if len(np.unique(centres, axis=0)) == h:
        want_nodes, want_prims, want_depth = host_bvh_nodes_probe(boxes[ids], 1, 16)
        want, _ = _canonical(want_nodes)
        assert want_depth == depth and len(want) == T, "%s: %d nodes in %d levels, the host builder makes %d in %d" % (where, T, depth, len(want), want_depth)
        assert np.array_equal(ids[want_prims], order), "%s: the leaf order is not the host builder's" % where
        assert np.array_equal(canon, want), "%s: %d words of the top level differ from the host builder's tree" % (where, int((canon != want).sum()))
    else:
        print("%s: coincident centroids, the host builder's tree is not compared" % where)
    return probe


@pytest.mark.parametrize("which", ["zoo", "example"])
def test_the_top_level_in_the_resident_array(which):
    host, core = MAKE[which](), Core(0)
    try:
        core.set_flavour("exact")
        core.upload(oracle_lib.with_luts(host.device_scene()))
        mesh_boxes = _mesh_boxes(host)
        first = None
        for step in range(3):
            host.set_instance_transforms(moved_instances(host, step))
            view = oracle_lib.with_luts(host.device_scene())
            core.update(view, MOVED)
            stats = core.instance_update_stats()
            assert (stats.device_updates, stats.fallbacks, stats.relayouts) == (step + 1, 0, 1), "%s, update %d: %d device updates, %d fallbacks, %d re-layouts" % (
                which, step, stats.device_updates, stats.fallbacks, stats.relayouts)
            probe = _check_tree(core, host, view, "%s, update %d" % (which, step), mesh_boxes)
            print("%s, update %d: T = %d of C = %d, M = %d, depth %d | %.3f ms: re-layout %.3f, upload %.3f, boxes %.3f, build %.3f, leaves %.3f" % (
                which, step, probe["T"], probe["C"], probe["M"], probe["depth"], 1e3 * stats.seconds, 1e3 * stats.seconds_relayout, 1e3 * stats.seconds_upload,
                1e3 * stats.seconds_boxes, 1e3 * stats.seconds_build, 1e3 * stats.seconds_leaves))
            first = first or probe
            assert (probe["C"], probe["M"], probe["mesh_hash"]) == (first["C"], first["M"], first["mesh_hash"]), "%s: the mesh part of the node array changed" % which
            assert np.array_equal(probe["mesh_root"], first["mesh_root"])
    finally:
        core.close(); host.close()


def _render(core):
    core.set_pixels(None)
    core.reset_counters()
    core.render(0, 2, samples_per_pass=2)
    fm, sm = core.accumulators()
    return fm, sm, core.query_counters()[:4]


def _against_oracle(core, view, where, fresh=None):
    fm, sm, cnt = _render(core)
    ofm, osm, ocnt = oracle_lib.render(view, 0, 2)
    _same(fm, ofm, where + ": first moment vs oracle")
    _same(sm, osm, where + ": second moment vs oracle")
    assert cnt == [int(x) for x in ocnt[:4]], "%s: ray counters %s, oracle %s" % (where, cnt, list(ocnt))
    assert float(fm.max()) > 0.0
    for name, other in (fresh or {}).items():
        ffm, fsm, fcnt = _render(other)
        _same(fm, ffm, "%s: first moment vs %s" % (where, name))
        _same(sm, fsm, "%s: second moment vs %s" % (where, name))
        assert cnt == fcnt, where
    return fm


def test_one_instance_falls_back_to_the_host_path():
    host, core = _single(), Core(0)
    try:
        core.set_flavour("exact")
        core.upload(oracle_lib.with_luts(host.device_scene()))
        inst = host.get_instance(0)
        inst.position, inst.rotation = Vec3(0.5, -0.25, 1.0), Vec3(0.3, 0.2, 0.1)
        host.set_instance_transforms([inst])
        view = oracle_lib.with_luts(host.device_scene())
        core.update(view, MOVED)
        stats = core.instance_update_stats()
        assert (stats.device_updates, stats.fallbacks) == (0, 1)
        with pytest.raises(CoreError):
            core.resident_tree_probe(1, 1)
        _against_oracle(core, view, "one instance, fallback")
    finally:
        core.close(); host.close()


# ---- render parity ----
@pytest.mark.parametrize("which", ["zoo", "example"])
def test_render_parity_after_three_updates(which):
    host = MAKE[which]()
    core, host_path, fresh = Core(0), Core(0), Core(0)
    try:
        for c in (core, host_path, fresh):
            c.set_flavour("exact")
        host_path.set_instance_update(1)
        first = oracle_lib.with_luts(host.device_scene())
        core.upload(first); host_path.upload(first)
        images = []
        for step in range(3):
            host.set_instance_transforms(moved_instances(host, step))
            view = oracle_lib.with_luts(host.device_scene())
            core.update(view, MOVED); host_path.update(view, MOVED)
            fresh.upload(view)
            images.append(_against_oracle(core, view, "%s, update %d" % (which, step), {"mode 1": host_path, "a fresh upload": fresh}))
        a, b = core.instance_update_stats(), host_path.instance_update_stats()
        assert (a.device_updates, a.fallbacks, a.relayouts) == (3, 0, 1) and (b.device_updates, b.fallbacks, b.relayouts) == (0, 0, 0)
        with pytest.raises(CoreError):
            host_path.resident_tree_probe(view.num_instances, view.num_meshes)
        assert not np.array_equal(images[0], images[2])
    finally:
        core.close(); host_path.close(); fresh.close(); host.close()


def _is_emissive(host, i):
    return any(host.get_material(int(k)).emission_active for k in set(host.get_mesh(host.get_instance(i).mesh_id)[3]))


def _emissive_instance(host):
    for i in range(host.get_num_instances()):
        if _is_emissive(host, i):
            return i
    raise AssertionError("no emissive instance")


def test_degenerate_emissive_and_the_updates_that_drop_the_layout():
    host, core = _zoo(48, 32, 3), Core(0)
    try:
        core.set_flavour("exact")
        core.upload(oracle_lib.with_luts(host.device_scene()))
        n = host.get_num_instances()
        mesh_boxes = _mesh_boxes(host)
        def update(instances, where, hittable):
            host.set_instance_transforms(instances)
            view = oracle_lib.with_luts(host.device_scene())
            core.update(view, MOVED)
            assert core.instance_update_stats().hittable == hittable, where
            _check_tree(core, host, view, where, _mesh_boxes(host))
            return _against_oracle(core, view, where)
        lamp = _emissive_instance(host)
        plain = next(i for i in range(n) if not _is_emissive(host, i))
        # an instance turns degenerate and comes back
        original = host.get_instance(plain)
        flat = host.get_instance(plain)
        flat.scale = Vec3(flat.scale.x, 0.0, flat.scale.z)
        before = _against_oracle(core, oracle_lib.with_luts(host.device_scene()), "as uploaded")
        gone = update([flat], "one instance degenerate", n - 1)
        back = update([original], "the instance restored", n)
        _same(back, before, "restored vs as uploaded")
        assert not np.array_equal(gone, before)
        # an emissive instance moves: the light table follows
        light = host.get_instance(lamp)
        light.position = Vec3(light.position.x + 0.4, light.position.y - 0.2, light.position.z + 0.3)
        light.rotation = Vec3(light.rotation.x + 0.5, light.rotation.y, light.rotation.z - 0.3)
        lit = update([light], "an emissive instance moved", n)
        assert not np.array_equal(lit, before)
        assert core.instance_update_stats().relayouts == 1 and core.instance_update_stats().device_updates == 3
        # a new instance (the host path drops the resident layout), then moved instances again: one more re-layout
        new = host.new_instance(host.get_instance(plain).mesh_id, position=(0.3, 0.4, -0.2), rotation=(0.1, 0.7, 0.0), scale=(0.5, 0.5, 0.5))
        view = oracle_lib.with_luts(host.device_scene())
        core.update(view, DIRTY_INSTANCES | DIRTY_LIGHTS)
        with pytest.raises(CoreError):
            core.resident_tree_probe(n + 1, view.num_meshes)
        _against_oracle(core, view, "a new instance")
        moved = host.get_instance(new)
        moved.position = Vec3(-0.3, 0.5, 0.1)
        update([moved], "the new instance moved", n + 1)
        assert core.instance_update_stats().relayouts == 2 and core.instance_update_stats().device_updates == 4
        # moved vertices after a resident update, then moved instances over the refitted mesh
        mesh = host.get_instance(plain).mesh_id
        host.set_mesh_positions(mesh, bend(host.get_mesh(mesh)[0], 0.2, 0.4))
        view = oracle_lib.with_luts(host.device_scene())
        core.update(view, DIRTY_MESH_POSITIONS | DIRTY_LIGHTS)
        assert core.mesh_refit_stats().last_refits == 1
        _against_oracle(core, view, "moved vertices after a resident update")
        update([original], "moved instances over the refitted mesh", n + 1)
        assert core.instance_update_stats().relayouts == 3 and core.instance_update_stats().fallbacks == 0
        # an update that names other instances than the scene on the device is refused, by name
        host.new_instance(mesh)
        with pytest.raises(CoreError, match="LUMC_DIRTY_INSTANCE_TRANSFORMS"):
            core.update(oracle_lib.with_luts(host.device_scene()), MOVED)
    finally:
        core.close(); host.close()


def test_the_host_api_renders_the_moved_scene_and_restarts_the_integration():
    host = _zoo(48, 32, 3)
    try:
        host.render_samples(0, 2, samples_per_pass=2)
        assert host.is_rendering()[1] == 2
        for step in range(2):
            host.set_instance_transforms(moved_instances(host, step))
            assert host.is_rendering()[1] == 0, "the integration did not restart"
            host.render_samples(0, 2, samples_per_pass=2)
            fm, sm = host.accumulators()
            ofm, osm, _ = oracle_lib.render(oracle_lib.with_luts(host.device_scene()), 0, 2)
            _same(fm, ofm, "update %d: first moment vs oracle" % step)
            _same(sm, osm, "update %d: second moment vs oracle" % step)
            stats = host.instance_update_stats()
            assert (stats["device_updates"], stats["fallbacks"], stats["relayouts"]) == (step + 1, 0, 1), stats
        host.set_instance_update(1)
        host.set_instance_transforms(moved_instances(host, 2))
        host.render_samples(0, 2, samples_per_pass=2)
        assert host.instance_update_stats()["device_updates"] == 2
        ofm, _, _ = oracle_lib.render(oracle_lib.with_luts(host.device_scene()), 0, 2)
        _same(host.accumulators()[0], ofm, "mode 1 through the host: first moment vs oracle")
    finally:
        host.close()


# ---- hostile rays over the resident layout: tests/ray_truth.py, with the acceptance rules of test_ray_truth.py, test_visibility_truth.py, test_light_query_truth.py ----
def test_ray_queries_over_the_resident_layout_against_the_truth():
    host, core = _zoo(), Core(0)
    try:
        core.set_flavour("exact")
        core.upload(oracle_lib.with_luts(host.device_scene()))
        host.set_instance_transforms(moved_instances(host, 0) + moved_instances(host, 1))
        view = oracle_lib.with_luts(host.device_scene())
        core.update(view, MOVED)
        assert core.instance_update_stats().device_updates == 1
        core.resident_tree_probe(view.num_instances, view.num_meshes)  # (the layout is resident: the queries below walk it)
        rng = np.random.RandomState(21)
        words = oracle_lib.view_arrays(view)["instance_transforms"].reshape(-1, 8)
        world = np.concatenate([_instance_world(words[i], host.get_mesh(host.get_instance(i).mesh_id)[0].reshape(-1, 3, 3)) for i in range(view.num_instances)])
        n = 2500
        tgt = _targets(rng, world, rng.randint(0, len(world), n), 0.2, 0.7)
        o = (tgt + rng.uniform(-6.0, 6.0, (n, 3))).astype(np.float32)
        d = _normalise32(tgt - o.astype(np.float64))
        o2, d2, _ = _axis_parallel_rays(rng, world, 500, 0.2, 0.7)
        o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
        rays = len(o)
        scene = ray_truth.scene_of_view(view)
        # closest hits (test_ray_truth.py test_gpu_closest_hits_against_the_truth)
        sol = ray_truth.solve(scene, o, d, None)
        want = oracle_lib.trace_closest(view, o, d, None, use_bvh=False)
        exact = core.trace_closest_host(o, d)
        core.set_flavour("fast")
        fast = core.trace_closest_host(o, d)
        ok_e, why_e = sol.check(exact)
        ok_f, why_f = sol.check(fast)
        same = (exact == want).all(axis=1)
        dec = sol.decisive
        agree = (fast[:, 0] == exact[:, 0]) & (fast[:, 1] == exact[:, 1])
        print("closest: %d rays, decisive share %.4f | exact: %d differ from the brute force, %d rejected | fast: %d rejected, %d decisive rays on another triangle" % (
            rays, dec.mean(), int((~same).sum()), int((~ok_e).sum()), int((~ok_f).sum()), int((dec & ~agree).sum())))
        assert (want[:, 0] != ray_truth.SKY).mean() > 0.9, "the rays must hit what they are aimed at"
        assert same.all(), "the exact flavour differs from the oracle's brute force on %d rays" % int((~same).sum())
        assert ok_e.all(), list(why_e[~ok_e][:5])
        assert ok_f.all(), list(why_f[~ok_f][:5])
        assert (agree | ~dec).all()
        # visibility (test_visibility_truth.py test_gpu_visibility_against_the_truth): even rays to the hit point with the hit triangle as the target, odd rays past it
        hit = want[:, 0] != ray_truth.SKY
        open_ = hit & (np.arange(rays) % 2 == 0)
        t_hit = want[:, 2].copy().view(np.float32)
        dist = np.where(hit, np.where(open_, t_hit, t_hit * np.float32(1.01)), np.float32(50.0)).astype(np.float32)
        ids = np.full((rays, 4), NONE, dtype=np.uint32)
        ids[open_, 0:2] = want[open_, 0:2]
        kind, factor = ray_truth.surface_factors(view)
        vsol = ray_truth.solve_visibility(scene, kind, factor, o, d, dist, ids)
        vwant = oracle_lib.trace_shadow(view, o, d, dist, ids, use_bvh=False)
        core.set_flavour("exact")
        vexact = core.trace_visibility_host(o, d, dist, ids)
        core.set_flavour("fast")
        vfast = core.trace_visibility_host(o, d, dist, ids)
        vsame = (vexact.view(np.uint32) == vwant.view(np.uint32)).all(axis=1)
        vok_e, vwhy_e = vsol.check(vexact)
        vok_f, vwhy_f = vsol.check(vfast, fast=True)
        vdec = vsol.decisive
        blocked_e, blocked_f = np.all(vexact == 0.0, axis=1), np.all(vfast == 0.0, axis=1)
        ku = np.maximum(vsol.k_certain - 1, 0) * ray_truth.U
        bound = (ku / (1.0 - ku))[:, None] * np.abs(vexact.astype(np.float64))
        close = (np.abs(vfast.astype(np.float64) - vexact.astype(np.float64)) <= bound).all(axis=1)
        print("visibility: decisive share %.4f | exact: %d differ from the brute force, %d rejected | fast: %d rejected, %d decisive rays blocked differently, %d products outside the bound" % (
            vdec.mean(), int((~vsame).sum()), int((~vok_e).sum()), int((~vok_f).sum()), int((vdec & (blocked_e != blocked_f)).sum()), int((vdec & ~close).sum())))
        assert not np.isnan(vexact).any() and not np.isnan(vfast).any(), "a ray nobody answered"
        assert vsame.all() and vok_e.all() and vok_f.all(), (list(vwhy_e[~vok_e][:5]), list(vwhy_f[~vok_f][:5]))
        assert not (vdec & (blocked_e != blocked_f)).any() and not (vdec & ~close).any()
        assert blocked_e.any() and (~blocked_e).any(), "both answers must occur"
        # light queries (test_light_query_truth.py test_gpu_light_queries_against_the_truth)
        handles = np.full((rays, 2), NONE, dtype=np.uint32)
        randoms = rng.uniform(0.0, 1.0, rays).astype(np.float32)
        lsol = ray_truth.solve_lights(view, o, d, handles, randoms)
        l_ids, l_hits = oracle_lib.trace_light_bvh(view, o, d, handles, randoms, use_bvh=False)
        core.set_flavour("exact")
        e_ids, e_hits = core.light_query_host(o, d, handles, randoms)
        core.set_flavour("fast")
        f_ids, f_hits = core.light_query_host(o, d, handles, randoms)
        lok_e, lwhy_e = lsol.check(e_ids, e_hits)
        lok_f, lwhy_f = lsol.check(f_ids, f_hits)
        want_ids, want_hits = lsol.expected()
        ldec = lsol.decisive
        print("light queries over %d lights: decisive share %.4f, %d rays cross a light | exact: %d rejected | fast: %d rejected" % (
            view.num_lights, ldec.mean(), int((l_hits > 0).sum()), int((~lok_e).sum()), int((~lok_f).sum())))
        assert ((e_ids == l_ids) & (e_hits == l_hits)).all(), "the exact flavour differs from the oracle's brute force"
        assert lok_e.all() and lok_f.all(), (list(lwhy_e[~lok_e][:5]), list(lwhy_f[~lok_f][:5]))
        assert (((e_ids == want_ids) & (e_hits == want_hits)) | ~ldec).all() and (((f_ids == want_ids) & (f_hits == want_hits)) | ~ldec).all()
        assert (l_hits > 0).any(), "some rays must cross a light"
    finally:
        core.close(); host.close()
