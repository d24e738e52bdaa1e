"""The scene's tree as the upload assembles it on the host (csrc/host/bvh_build.cpp assemble_scene_tree, through lumc_scene_tree_probe; no GPU): the top level
over the instances, every mesh's tree behind it in one node array, renumbered breadth first so that the ray kernels can stage "node index < K" in LDS; the
top-level leaf records, the rows by instance id, the traversal triangles. The GPU parity suites see an error here only as a wrong image."""
import ctypes as C
from collections import deque

import numpy as np
import pytest

import luminary_amd

EMPTY, LEAF = 0xFFFFFFFF, 0x80000000
TOP_BUDGET = 4096  # nodes the renumbering orders (the most the ray kernels could stage)
NODE = np.dtype([("box", np.float32, (6, 4)), ("child", np.uint32, 4), ("pad", np.uint32, 4)])  # lo_x[4] lo_y lo_z hi_x hi_y hi_z
TRI = np.dtype([("p0", np.float32, 3), ("id", np.uint32), ("e1", np.float32, 3), ("scene_index", np.uint32), ("e2", np.float32, 3), ("albedo_tex", np.uint32)])
assert NODE.itemsize == 128 and TRI.itemsize == 48


def _transform(pos, scale=(1.0, 1.0, 1.0), quat=(0.0, 0.0, 0.0, 1.0)):
    """32 bytes of an instance: translation, scale, the rotation as four 16-bit words (csrc/host/scene.cpp)."""
    q = np.asarray(quat, np.float64) / np.linalg.norm(quat)
    w16 = [int((1.0 - q[0]) * 0x7FFF + 0.5), int((1.0 - q[1]) * 0x7FFF + 0.5), int((1.0 - q[2]) * 0x7FFF + 0.5), int((1.0 + q[3]) * 0x7FFF + 0.5)]
    out = np.zeros(8, np.float32)
    out[0:3], out[3:6] = pos, scale
    out[6:8] = np.array([w16[0] | (w16[1] << 16), w16[2] | (w16[3] << 16)], np.uint32).view(np.float32)
    return out


def _world_to_object(transform):
    """The linear part of an instance's world -> object map in float64, on its own: q v q* of the quaternion the 16-bit words hold (not exactly of length
    one, hence the homogeneous form of the rotation matrix) applied to v / scale."""
    w = transform[6:8].view(np.uint32)
    x, y, z = (1.0 - float(h) / 0x7FFF for h in (int(w[0]) & 0xFFFF, int(w[0]) >> 16, int(w[1]) & 0xFFFF))
    s = float(int(w[1]) >> 16) / 0x7FFF - 1.0
    r = np.array([[s * s + x * x - y * y - z * z, 2 * (x * y - s * z), 2 * (x * z + s * y)],
                  [2 * (x * y + s * z), s * s - x * x + y * y - z * z, 2 * (y * z - s * x)],
                  [2 * (x * z - s * y), 2 * (y * z + s * x), s * s - x * x - y * y + z * z]])
    return r / transform[3:6].astype(np.float64)[None, :]


def _triangles(corners):
    """[n, 3, 3] corner positions -> [n, 12] floats (3 x float4, w = 1)."""
    v = np.ones((len(corners), 3, 4), np.float32)
    v[:, :, :3] = corners
    return v.reshape(len(corners), 12)


def _box_mesh():
    c = np.array([[x, y, z] for x in (-1.0, 1.5) for y in (-0.5, 0.75) for z in (-2.0, 1.0)], np.float32)  # corner index = 4 x + 2 y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return _triangles(np.array([[c[a], c[b], c[d]] for a, b, d, e in quads] + [[c[a], c[d], c[e]] for a, b, d, e in quads]))


def _grid_mesh(nx, nz):
    x, z = np.meshgrid(np.arange(nx + 1, dtype=np.float64), np.arange(nz + 1, dtype=np.float64), indexing="ij")
    p = np.stack([0.1 * x, 0.3 * np.sin(0.07 * x) * np.cos(0.05 * z), 0.1 * z], -1).astype(np.float32)
    a, b, c, d = p[:-1, :-1], p[1:, :-1], p[:-1, 1:], p[1:, 1:]
    return _triangles(np.concatenate([np.stack([a, b, c], 2).reshape(-1, 3, 3), np.stack([d, c, b], 2).reshape(-1, 3, 3)]))


def _scene_small():
    """Three meshes (a 12-triangle box, one triangle, no triangle) and seven instances, four of which exercise the skip paths and the shared mesh root."""
    meshes = [_box_mesh(), _triangles(np.array([[[0.0, 0.0, 0.0], [2.0, 0.25, 0.0], [0.5, 3.0, -1.0]]])), np.zeros((0, 12), np.float32)]
    instances = [(0, _transform((0.0, 0.0, 0.0))),
                 (0, _transform((5.0, -2.0, 1.0), (0.25, 1.0, 4.0), (0.3, -0.2, 0.5, 0.78))),
                 (1, _transform((-3.0, 1.0, 2.0), quat=(0.0, 0.6, 0.0, 0.8))),
                 (2, _transform((1.0, 1.0, 1.0))),                     # the empty mesh
                 (7, _transform((2.0, 2.0, 2.0))),                     # a mesh id out of range
                 (0, _transform((0.0, 9.0, 0.0), (1.0, 0.0, 1.0))),    # a zero scale component: no inverse
                 (0, _transform((-8.0, 0.5, -4.0), (2.0, 2.0, 2.0)))]  # the box a second time
    return meshes, instances, [0, 1, 2, 6]


def _scene_grid():
    return [_grid_mesh(200, 100)], [(0, _transform((1.0, 2.0, 3.0), quat=(0.1, 0.2, -0.1, 0.95)))], [0]


def _probe(meshes, instances):
    lib = luminary_amd._lib()
    lib.lumc_scene_tree_probe.restype = C.c_int
    lib.lumc_scene_tree_probe.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)] + [C.c_void_p] * 6
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in meshes])]).astype(np.uint32)
    vertices = np.ascontiguousarray(np.concatenate(meshes), np.float32)
    mesh_ids = np.array([m for m, _ in instances], np.uint32)
    transforms = np.ascontiguousarray(np.stack([t for _, t in instances]), np.float32)
    view = luminary_amd.DeviceSceneView()
    view.num_meshes, view.num_instances = len(meshes), len(instances)
    view.mesh_tri_offset, view.vertices = offsets.ctypes.data, vertices.ctypes.data
    view.instance_mesh_ids, view.instance_transforms = mesh_ids.ctypes.data, transforms.ctypes.data
    sizes = (C.c_uint64 * 4)()
    assert lib.lumc_scene_tree_probe(C.addressof(view), sizes, None, None, None, None, None, None) == 0
    out = {"nodes": np.zeros(sizes[0], NODE), "tris": np.zeros(sizes[3], TRI), "leaves": np.zeros((sizes[2], 4, 4), np.float32),
           "rows": np.zeros((len(instances) + 1, 3, 4), np.float32), "mesh_root": np.zeros(len(meshes) + 1, np.uint32), "bounds": np.zeros((2, 3), np.float32)}
    again = (C.c_uint64 * 4)()
    assert lib.lumc_scene_tree_probe(C.addressof(view), again, *[out[k].ctypes.data for k in ("nodes", "tris", "leaves", "rows", "mesh_root", "bounds")]) == 0
    assert list(again) == list(sizes)
    out.update(tlas_num_nodes=int(sizes[1]), offsets=offsets, vertices=vertices.reshape(-1, 3, 4)[:, :, :3], mesh_ids=mesh_ids, transforms=transforms)
    return out


_SCENES = {}


def _tree(name):
    """Built once per scene and read by every test."""
    if name not in _SCENES:
        meshes, instances, survivors = _scene_small() if name == "small" else _scene_grid()
        _SCENES[name] = (_probe(meshes, instances), survivors)
    return _SCENES[name]


def _leaf_range(c):
    return int(c & 0x0FFFFFFF), int((c >> 28) & 7) + 1


def _walk(t, start, top):
    """Breadth first from `start`; a leaf of a top-level node continues into the root of its instance's mesh. -> [(node, is a top-level node)] in visit order."""
    child = t["nodes"]["child"]
    n = len(child)
    seen = np.zeros(n, bool)
    seen[start] = True
    order, queue = [(start, top)], deque([(start, top)])
    while queue:
        node, is_top = queue.popleft()
        for c in child[node]:
            if c == EMPTY:
                continue
            if c & LEAF:
                if not is_top:
                    continue
                first, count = _leaf_range(c)
                assert count == 1 and first < len(t["leaves"]) - 1, "one instance per top-level leaf, never the padding record"
                inst = int(t["leaves"][first, 3].view(np.uint32)[0])
                nxt, nxt_top = int(t["mesh_root"][t["mesh_ids"][inst]]), False
            else:
                nxt, nxt_top = int(c), is_top
            assert nxt < n, "child index in range"
            if not seen[nxt]:
                seen[nxt] = True
                order.append((nxt, nxt_top))
                queue.append((nxt, nxt_top))
    return order


@pytest.mark.parametrize("name", ["small", "grid"])
def test_the_nodes_are_numbered_breadth_first_and_all_reachable(name):
    t, survivors = _tree(name)
    n = len(t["nodes"])
    if name == "grid":  # 40 000 triangles in leaves of at most two under nodes of at most four children: at least 5000 nodes
        assert luminary_amd._lib().lumc_leaf_max_triangles() <= 2 and n > TOP_BUDGET, n
    inner = t["nodes"]["child"][(t["nodes"]["child"] != EMPTY) & ((t["nodes"]["child"] & LEAF) == 0)]
    assert inner.size == 0 or inner.max() < n
    from_root = _walk(t, 0, True)
    # (the tree of a mesh that no surviving instance names is never reached from node 0: it stays behind the ordered part)
    ordered = min(n, TOP_BUDGET, len(from_root))
    assert [i for i, _ in from_root[:ordered]] == list(range(ordered)), "a breadth-first walk meets the nodes in the order of their indices"
    top_level = {i for i, is_top in from_root if is_top}
    assert len(top_level) == t["tlas_num_nodes"]
    # every node is reachable: from node 0, or - such a mesh keeps its tree in the array for the next instance edit - from its mesh's root
    by_mesh = [{i for i, _ in _walk(t, int(t["mesh_root"][m]), False)} for m in range(len(t["offsets"]) - 1)]
    assert top_level.union(*by_mesh) == set(range(n))
    assert {i for i, _ in from_root} == top_level.union(*[by_mesh[int(t["mesh_ids"][i])] for i in survivors])


@pytest.mark.parametrize("name", ["small", "grid"])
def test_the_top_level_leaves_name_the_instances_that_can_be_hit(name):
    t, survivors = _tree(name)
    leaves, words = t["leaves"], t["leaves"][:, 3].view(np.uint32)
    assert len(leaves) == len(survivors) + 1, "one record per surviving instance and one of padding"
    assert sorted(int(w[0]) for w in words[:-1]) == survivors
    referenced = []
    for node, is_top in _walk(t, 0, True):
        if not is_top:
            continue
        for k, c in enumerate(t["nodes"]["child"][node]):
            if c == EMPTY or not (c & LEAF):
                continue
            rec = _leaf_range(c)[0]
            referenced.append(rec)
            inst = int(words[rec, 0])
            mesh = int(t["mesh_ids"][inst])
            assert int(words[rec, 1]) == int(t["mesh_root"][mesh]) and tuple(words[rec, 2:]) == (0, 0)
            assert np.array_equal(leaves[rec, :3, 3], t["transforms"][inst, :3]), "the rows' .w are the translation"
            assert np.array_equal(leaves[rec, :3].view(np.uint32), t["rows"][inst].view(np.uint32)), "the record holds the rows kept by instance id"
            # the rows against the float64 matrix: the float32 code rounds the four decoded numbers (2 roundings each, entering an entry of the
            # rotation with a factor of at most 4 |q|) and then about eight more times per entry, every term at most 1 / scale: 32 ulp of 1 / min scale
            want = _world_to_object(t["transforms"][inst])
            assert np.abs(leaves[rec, :3, :3] - want).max() <= 32 * 2.0 ** -24 / np.abs(t["transforms"][inst, 3:6]).min(), (inst, leaves[rec, :3, :3], want)
            # the leaf's box around the mesh where the kernels' ray mapping (x -> M (x - t)) puts it: world = M^-1 v + t, in float64
            m64, tr = leaves[rec, :3, :3].astype(np.float64), leaves[rec, :3, 3].astype(np.float64)
            v = t["vertices"][t["offsets"][mesh]:t["offsets"][mesh + 1]].reshape(-1, 3).astype(np.float64)
            world = v @ np.linalg.inv(m64).T + tr
            box = t["nodes"]["box"][node][:, k].astype(np.float64)
            assert np.all(box[:3] <= world.min(0)) and np.all(box[3:] >= world.max(0)), (inst, box, world.min(0), world.max(0))
            assert np.all(t["bounds"][0] <= world.min(0)) and np.all(t["bounds"][1] >= world.max(0))
    assert sorted(referenced) == list(range(len(survivors))), "every record hangs in exactly one leaf"


@pytest.mark.parametrize("name", ["small", "grid"])
def test_every_mesh_tree_tiles_its_triangles_and_bounds_them(name):
    t, _ = _tree(name)
    nodes, tris, verts = t["nodes"], t["tris"], t["vertices"]
    assert len(tris) == t["offsets"][-1] + 1, "one traversal triangle per triangle and one of padding"
    for m in range(len(t["offsets"]) - 1):
        t0, t1 = int(t["offsets"][m]), int(t["offsets"][m + 1])
        covered = np.zeros(t1 - t0, np.int64)
        below = {}
        for node, _ in reversed(_walk(t, int(t["mesh_root"][m]), False)):  # children before their parents
            lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
            for k, c in enumerate(nodes["child"][node]):
                if c == EMPTY:
                    continue
                if c & LEAF:
                    first, count = _leaf_range(c)
                    assert t0 <= first and first + count <= t1, "leaf ranges index the scene's traversal triangles"
                    covered[first - t0:first - t0 + count] += 1
                    p = verts[tris["scene_index"][first:first + count]].reshape(-1, 3).astype(np.float64)
                    clo, chi = p.min(0), p.max(0)
                else:
                    clo, chi = below[int(c)]
                box = nodes["box"][node][:, k].astype(np.float64)
                assert np.all(box[:3] <= clo) and np.all(box[3:] >= chi), (m, node, k)
                lo, hi = np.minimum(lo, clo), np.maximum(hi, chi)
            below[node] = (lo, hi)
        assert np.all(covered == 1), "the leaves under the mesh's root tile [t0, t0 + nt) exactly once"
        mine = tris[t0:t1]
        assert np.array_equal(np.sort(mine["scene_index"]), np.arange(t0, t1)) and np.array_equal(mine["id"], mine["scene_index"] - t0)
        v = verts[mine["scene_index"]]  # float32: the edges are single float subtractions
        assert np.array_equal(mine["p0"], v[:, 0]) and np.array_equal(mine["e1"], v[:, 1] - v[:, 0]) and np.array_equal(mine["e2"], v[:, 2] - v[:, 0])
