"""A float64 brute force for particle queries: every triangle of every one of the 25^3 lattice cells, with the disc cut-out in barycentric space
(optix_common.cuh:67-74). Test infrastructure only; nothing here is taken from what a device or the oracle returned."""
import ctypes as C

import numpy as np

NO_TRIANGLE = 0xFFFFFFFF


def particle_triangles(view):
    """The unit cell's triangles of a DeviceSceneView as float64 [2 * count, 3, 3]."""
    n = 2 * int(view.particles_count)
    return np.ctypeslib.as_array(C.cast(view.particle_vertices, C.POINTER(C.c_float)), shape=(n, 3, 4))[..., :3].astype(np.float64)


def brute_force(tris, pos, d, tmax):
    """The nearest admissible hit of every ray (pos in [0, 1)^3, d = direction / particles_scale, tmax; float32 [n, ...]): (triangle index [n], NO_TRIANGLE for
    a miss; distance [n] float64)."""
    g = np.arange(-12, 13, dtype=np.float64)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    p0, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    best_tri, best_t = np.full(len(pos), NO_TRIANGLE, dtype=np.int64), np.full(len(pos), np.inf)
    for r in range(len(pos)):
        o = pos[r].astype(np.float64)[None, None, :] - cells[:, None, :]     # [cell, 1, 3]
        dd = d[r].astype(np.float64)
        h = np.cross(dd, e2)                                                   # [tri, 3]
        a = (e1 * h).sum(axis=1)
        s = o - p0[None, :, :]                                                 # [cell, tri, 3]
        u = (s * h[None]).sum(axis=2) / a
        q = np.cross(s, e1[None])
        v = (q * dd).sum(axis=2) / a
        t = (q * e2[None]).sum(axis=2) / a
        ok = (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t < tmax[r]) & ((u - 0.5) ** 2 + (v - 0.5) ** 2 <= 0.25)
        if ok.any():
            tt = np.where(ok, t, np.inf)
            best = np.unravel_index(np.argmin(tt), tt.shape)
            best_tri[r], best_t[r] = best[1], tt[best]
    return best_tri, best_t


def check_against_brute_force(truth, out_t, out_tri, per_particle=False):
    """Asserts that (out_t, out_tri) - the distance and the triangle index, NO_TRIANGLE for a miss - are what brute_force found (`truth`). per_particle:
    out_tri holds the particle (triangle index >> 1, what a path's hit id keeps). Returns the number of rays that hit."""
    best_tri, best_t = truth
    hits = 0
    for r in range(len(best_tri)):
        if best_tri[r] != NO_TRIANGLE:
            assert out_tri[r] == (best_tri[r] >> 1 if per_particle else best_tri[r]), (r, out_tri[r], best_tri[r])
            assert abs(out_t[r] - best_t[r]) < 1e-4 * max(1.0, best_t[r])
            hits += 1
        else:
            assert out_tri[r] == NO_TRIANGLE, (r, out_tri[r])
    return hits
