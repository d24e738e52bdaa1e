"""A host walk of the scene's node array as the single-level closest-hit kernel walks it (csrc/device/dev_trace.h trace_items<Q, true>, visit_node /
enter_children, ClosestState::on_tris), for tests that need to know WHICH nodes a ray visits and in what order: tests/test_coherent_first_hits.py builds waves
whose two halves share a given number of visits.

The tree comes from lumc_scene_tree_probe - what lumc_scene_upload assembles with the host builder, no device needed. The walk follows the kernel's rules: the
near / far planes by the signs of the reciprocal direction, entry distance max(ax, ay, max(az, 0)), exit min(bx, by, min(bz, tmax)), accepted when
tn <= tf * 1.000004 + 1e-30, the five-comparator network on (entry distance, child) with a swap only where the second key is smaller, the far children pushed
far to near, a pop dropping what lies beyond the nearest hit so far, a leaf's triangles tested in order with tmax shrinking. Arithmetic is float64 on float32
inputs, not the device's fma / v_rcp sequence, so the walk also returns its MARGIN: the smallest relative distance of any decision it took (a box accepted or
refused, two sort keys ordered, a pop kept or dropped, a triangle's barycentrics and distance) from the other outcome. A caller takes a walk for the device's
only where the margin is far above the arithmetic's differences (1e-6); `textured` says that a triangle with an albedo texture was crossed, whose alpha cut-out
the walk does not evaluate."""
import ctypes as C

import numpy as np

import luminary_amd

EMPTY, LEAF, FLT_MAX = 0xFFFFFFFF, 0x80000000, float(np.finfo(np.float32).max)
NODE = np.dtype([("box", np.float32, (6, 4)), ("child", np.uint32, 4), ("pad", np.uint32, 4)])  # lo_x[4] lo_y lo_z hi_x hi_y hi_z
TRI = np.dtype([("p0", np.float32, 3), ("id", np.uint32), ("e1", np.float32, 3), ("scene_index", np.uint32), ("e2", np.float32, 3), ("albedo_tex", np.uint32)])


def scene_tree(view):
    """(nodes, tris, root of the one instance's mesh tree) of a single-level scene"""
    lib = luminary_amd._lib()
    lib.lumc_scene_tree_probe.restype = C.c_int
    lib.lumc_scene_tree_probe.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)] + [C.c_void_p] * 6
    sizes = (C.c_uint64 * 4)()
    assert lib.lumc_scene_tree_probe(C.addressof(view), sizes, None, None, None, None, None, None) == 0
    assert sizes[1] == 1 and sizes[2] == 2, "one top-level node, the instance's leaf record and the padding record: a single-level scene"
    nodes, tris, leaves = np.zeros(sizes[0], NODE), np.zeros(sizes[3], TRI), np.zeros((sizes[2], 4, 4), np.float32)
    assert lib.lumc_scene_tree_probe(C.addressof(view), sizes, nodes.ctypes.data, tris.ctypes.data, leaves.ctypes.data, None, None, None) == 0
    assert np.array_equal(leaves[0, :3, :3], np.eye(3, dtype=np.float32)) and not leaves[0, :3, 3].any(), "the walk is in world space: the instance sits under the identity"
    return nodes, tris, int(leaves[0, 3].view(np.uint32)[1])


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-30)


def walk(tree, origin, direction, num_textures=0):
    """(sequence of `cur` values - inner nodes and leaves - in the order of the kernel's turns, margin, textured, (triangle id, t) of the hit or None)"""
    nodes, tris, root = tree
    o, d = [float(np.float32(x)) for x in origin], [float(np.float32(x)) for x in direction]
    inv = [float(np.float32(1.0 / x)) for x in d]
    noi = [float(np.float32(-(o[k] * inv[k]))) for k in range(3)]
    near = [3 if inv[k] < 0.0 else 0 for k in range(3)]  # row offset of the near plane: hi (3 + axis) for a negative direction
    seq, stack, margin, textured = [], [], float("inf"), False
    cur, tmax, best = root, FLT_MAX, None
    while True:
        seq.append(cur)
        if cur & LEAF:
            first, count = cur & 0x0FFFFFFF, ((cur >> 28) & 7) + 1
            for t_ in tris[first:first + count]:
                p0, e1, e2 = t_["p0"].astype(np.float64), t_["e1"].astype(np.float64), t_["e2"].astype(np.float64)
                h = np.cross(d, e2)
                a = float(np.dot(e1, h))
                if a == 0.0:
                    margin = 0.0
                    continue
                f, s = 1.0 / a, np.asarray(o) - p0
                u = f * float(np.dot(s, h))
                q = np.cross(s, e1)
                v = f * float(np.dot(d, q))
                margin = min(margin, abs(u), abs(v), abs(1.0 - u - v))
                if v < 0.0 or u < 0.0 or not (u + v <= 1.0):
                    continue
                t = f * float(np.dot(e2, q))
                margin = min(margin, abs(t), _rel(t, tmax))
                if t >= 0.0 and t < tmax:
                    textured |= int(t_["albedo_tex"]) < num_textures
                    best, tmax = (int(t_["id"]), t), float(np.float32(t))
            cur = EMPTY
        else:
            box, child = nodes[cur]["box"].astype(np.float64), nodes[cur]["child"]
            keys = []
            for c in range(4):
                a = [box[near[k] + k][c] * inv[k] + noi[k] for k in range(3)]
                b = [box[3 - near[k] + k][c] * inv[k] + noi[k] for k in range(3)]
                tn, tf = max(a[0], a[1], max(a[2], 0.0)), min(b[0], b[1], min(b[2], tmax))
                bound = tf * 1.000004 + 1e-30
                if child[c] != EMPTY:
                    margin = min(margin, _rel(tn, bound))
                keys.append((tn if tn <= bound and child[c] != EMPTY else float("inf"), int(child[c])))
            for i, j in ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2)):  # cswap: swapped only where the second key is smaller
                ki, kj = keys[i][0], keys[j][0]
                if ki != float("inf") and kj != float("inf") and not (ki == 0.0 and kj == 0.0):  # (two zeros: both origins inside, exact on the device too)
                    margin = min(margin, _rel(ki, kj))
                if kj < ki:
                    keys[i], keys[j] = keys[j], keys[i]
            for k, c in reversed(keys[1:]):  # far to near, the real ones only
                if k < float("inf"):
                    stack.append((c, k))
            cur = keys[0][1] if keys[0][0] < float("inf") else EMPTY
        if cur == EMPTY:
            while stack:
                c, k = stack.pop()
                bound = tmax * 1.000004 + 1e-30
                if tmax < FLT_MAX:
                    margin = min(margin, _rel(k, bound))
                if k <= bound:
                    cur = c
                    break
            if cur == EMPTY:
                return seq, margin, textured, best


def shared_visits(seq_a, seq_b):
    """inner-node visits two walks share before their sequences part: the turns two lanes make as one"""
    n = 0
    for a, b in zip(seq_a, seq_b):
        if a != b:
            break
        n += 0 if a & LEAF else 1
    return n
