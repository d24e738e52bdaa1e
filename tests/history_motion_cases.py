"""What tests/test_history_motion.py and tests/test_history_motion_gpu.py share: a numpy restatement of the motion part of csrc/host/history.h written from the
header's text - binary64 for the instance record, binary32 for the pixel, every operation one at a time in the header's order -, the worlds (a wall and the sky
with a box instance in front, walked in float64) and the families of moves. Not a test file."""
import numpy as np

import history_cases as H
from luminary_amd import core

F, U, D = np.float32, np.uint32, np.float64
SAME, MOVED, VOID = core.HISTORY_MOTION_SAME, core.HISTORY_MOTION_MOVED, core.HISTORY_MOTION_VOID
EMPTY, MISS, OCEAN, PARTICLE = core.MATTE_ID_EMPTY, core.MATTE_ID_MISS, core.MATTE_ID_OCEAN, core.MATTE_ID_PARTICLE
RESERVED = 0xFFFFFFFC
CAP = 8.0  # motion_max_history of the cases
COUNTS = (1, 3, 65, 300)  # one record; a few; a wave and one; several waves and a tail


# ---- the record, restated ----
def words(translation, scale, quat):
    """the 8 words of a transform as the scene view holds them (scene.cpp encode_transform): translation, scale, the quaternion (x, y, z, w) in 4 x 16 bits"""
    q = [float(c) for c in quat]
    enc = lambda v: int((v * 0x7FFF) + 0.5) & 0xFFFF
    x, y, z, w = enc(1.0 - q[0]), enc(1.0 - q[1]), enc(1.0 - q[2]), enc(1.0 + q[3])
    out = np.zeros(8, F)
    out[:3], out[3:6] = translation, scale
    out[6:8] = np.array([x | (y << 16), z | (w << 16)], U).view(F)
    return out


def instance_matrix(p):
    """the world->object matrix of the header (instance_inverse_rows) in binary32, returned in binary64; None: a translation or scale word is not finite"""
    p = np.asarray(p, F)
    if not H.finite(p[:6]).all():
        return None
    a, b = (int(v) for v in p[6:8].view(U))
    c = F(1) / F(32767)
    ax, ay, az, aw = F(a & 0xFFFF) * c, F(a >> 16) * c, F(b & 0xFFFF) * c, F(b >> 16) * c
    u = (F(1) - ax, F(1) - ay, F(1) - az)
    s = aw - F(1)
    with np.errstate(all="ignore"):
        i = (F(1) / p[3], F(1) / p[4], F(1) / p[5])
        duu = H.dot(u, u)
        k1 = s * s - duu
        k2 = F(2) * s
        M = np.zeros((3, 3), D)
        for j in range(3):
            v = tuple(F(1.0 if j == k else 0.0) * i[k] for k in range(3))
            duv = H.dot(u, v)
            cr = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
            k0 = F(2) * duv
            for k in range(3):
                M[k][j] = D((u[k] * k0 + v[k] * k1) + cr[k] * k2)
    return M


def inverse3(m):
    """by cofactors over the determinant, in binary64; None: the determinant is zero or not finite"""
    with np.errstate(all="ignore"):
        sub2 = lambda a, b, c, d: a * b - c * d
        c0, c1, c2 = sub2(m[1][1], m[2][2], m[1][2], m[2][1]), sub2(m[1][0], m[2][2], m[1][2], m[2][0]), sub2(m[1][0], m[2][1], m[1][1], m[2][0])
        det = (m[0][0] * c0 - m[0][1] * c1) + m[0][2] * c2
        if not (abs(det) > 0.0) or not np.isfinite(det):
            return None
        f = np.zeros((3, 3), D)
        f[0][0] = c0 / det
        f[0][1] = sub2(m[0][2], m[2][1], m[0][1], m[2][2]) / det
        f[0][2] = sub2(m[0][1], m[1][2], m[0][2], m[1][1]) / det
        f[1][0] = sub2(m[1][2], m[2][0], m[1][0], m[2][2]) / det
        f[1][1] = sub2(m[0][0], m[2][2], m[0][2], m[2][0]) / det
        f[1][2] = sub2(m[0][2], m[1][0], m[0][0], m[1][2]) / det
        f[2][0] = c2 / det
        f[2][1] = sub2(m[0][1], m[2][0], m[0][0], m[2][1]) / det
        f[2][2] = sub2(m[0][0], m[1][1], m[0][1], m[1][0]) / det
    return f


def mul3(a, b, i, j):
    return (a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j]


def motion_record(old8, new8):
    r = np.zeros((), core.HISTORY_MOTION_RECORD)
    old8, new8 = np.asarray(old8, F), np.asarray(new8, F)
    if np.array_equal(old8.view(U), new8.view(U)):
        r["cls"] = SAME
        return r
    r["cls"] = VOID
    Mo, Mn = instance_matrix(old8), instance_matrix(new8)
    if Mo is None or Mn is None:
        return r
    Fo, Fn = inverse3(Mo), inverse3(Mn)
    if Fo is None or Fn is None:
        return r
    with np.errstate(all="ignore"):
        L = np.array([F(mul3(Fo, Mn, i, j)) for i in range(3) for j in range(3)], F)
        NL = np.array([F(mul3(Fn, Mo, j, i)) for i in range(3) for j in range(3)], F)
    if not (H.finite(L).all() and H.finite(NL).all()):
        return r
    r["cls"], r["t_new"], r["t_old"], r["L"], r["NL"] = MOVED, new8[:3], old8[:3], L, NL
    return r


def motion_records(old8, new8):
    old8, new8 = np.asarray(old8, F).reshape(-1, 8), np.asarray(new8, F).reshape(-1, 8)
    rec = np.zeros(len(old8), core.HISTORY_MOTION_RECORD)
    for i in range(len(old8)):
        rec[i] = motion_record(old8[i], new8[i])
    cls = rec["cls"]
    return rec, (int((cls == MOVED).sum()), int((cls == SAME).sum()), int((cls == VOID).sum()))


# ---- the pixel, restated ----
def owner_class(o, records):
    count = len(records)
    o = np.asarray(o, U)
    cls = records["cls"][np.where(o < count, o, 0)] if count else np.zeros(o.shape, U)
    return np.where(o >= U(RESERVED), U(SAME), np.where(o >= U(count), U(VOID), cls)).astype(U)


def row_apply(a, b, c, v):
    return (a * v[0] + b * v[1]) + c * v[2]


def reproject_motion(now, old, st, cap, normal, depth, old_shown, old_weight, old_normal, old_depth, owner, old_owner, records):
    """-> carried [3, P], carried_weight [P], (carried, rejected, off, owner moved, owner moved and carried), info: what the branch-coverage assertions read"""
    w, h, ow, oh = now.width, now.height, old.width, old.height
    P, count = w * h, len(records)
    normal, depth = np.asarray(normal, F).reshape(3, P), np.asarray(depth, F).reshape(P)
    old_shown, old_weight = np.asarray(old_shown, F).reshape(3, ow * oh), np.asarray(old_weight, F).reshape(ow * oh)
    old_normal, old_depth = np.asarray(old_normal, F).reshape(3, ow * oh), np.asarray(old_depth, F).reshape(ow * oh)
    owner, old_owner = np.asarray(owner, U).reshape(P), np.asarray(old_owner, U).reshape(ow * oh)
    py, px = np.divmod(np.arange(P), w)
    c = owner_class(owner, records)
    void, moved = c == VOID, c == MOVED
    rec = records[np.where(moved, owner, 0)] if count else np.zeros(P, core.HISTORY_MOTION_RECORD)
    with np.errstate(all="ignore"):
        d = H.centre_ray(now, px.astype(F), py.astype(F))
        surface = depth >= F(0)
        X = tuple(F(now.pos[i]) + d[i] * depth for i in range(3))
        # step 1, the moved form
        dd = tuple(X[i] - rec["t_new"][:, i] for i in range(3))
        Ld = tuple(row_apply(rec["L"][:, 3 * i], rec["L"][:, 3 * i + 1], rec["L"][:, 3 * i + 2], dd) for i in range(3))
        Xo = tuple(rec["t_old"][:, i] + Ld[i] for i in range(3))
        nn = tuple(row_apply(rec["NL"][:, 3 * i], rec["NL"][:, 3 * i + 1], rec["NL"][:, 3 * i + 2], normal) for i in range(3))
        l = np.sqrt(H.dot(nn, nn))
        use = moved & surface
        bad_normal = use & ~((l > F(0)) & H.finite(l))
        n_cmp = tuple(np.where(use, nn[i] / l, normal[i]) for i in range(3))
        X = tuple(np.where(use, Xo[i], X[i]) for i in range(3))
        vs = tuple(X[i] - F(old.pos[i]) for i in range(3))
        v = tuple(np.where(surface, vs[i], d[i]) for i in range(3))
        r = np.where(surface, np.sqrt(H.dot(v, v)), F(0))
        alive = ~void & ~bad_normal
        valid, fx, fy = H.project(old, v)
        on = alive & valid & (fx >= F(-1)) & (fx < F(ow)) & (fy >= F(-1)) & (fy < F(oh))
        fx, fy = np.where(on, fx, F(0)), np.where(on, fy, F(0))
        x0f, y0f = np.floor(fx), np.floor(fy)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        tx, ty = fx - x0f, fy - y0f
        ux, uy = F(1) - tx, F(1) - ty
        tol = F(st.depth_tolerance) * r
        ws, sw = np.zeros(P, F), np.zeros(P, F)
        s = [np.zeros(P, F) for _ in range(3)]
        refused_by_owner = np.zeros(P, np.int64)
        for k in range(4):
            x, y = x0 + (k & 1), y0 + (k >> 1)
            wt = (tx if k & 1 else ux) * (ty if k >> 1 else uy)
            inside = on & (x >= 0) & (y >= 0) & (x < ow) & (y < oh)
            q = np.where(inside, y * ow + x, 0)
            gn, gd = old_normal[:, q], old_depth[q]
            dlt = gd - r
            ad = np.where(dlt < F(0), -dlt, dlt)
            geo = np.where(surface, (gd >= F(0)) & (ad <= tol) & (H.dot(n_cmp, gn) >= F(st.normal_threshold)), gd < F(0))
            oo = old_owner[q]
            own = (oo == owner) | ((c == SAME) & (owner_class(oo, records) == SAME))
            refused_by_owner += (inside & geo & ~own)
            sh, swt = old_shown[:, q], old_weight[q]
            ok = inside & geo & own & H.finite(sh[0]) & H.finite(sh[1]) & H.finite(sh[2]) & H.finite(swt) & (swt > F(0))
            ws = np.where(ok, ws + wt, ws)
            for ch in range(3):
                s[ch] = np.where(ok, s[ch] + wt * sh[ch], s[ch])
            sw = np.where(ok, sw + wt * swt, sw)
        got = on & (ws > F(0))
        qw = sw / ws
        limit = np.where(moved, F(cap), F(st.max_history)).astype(F)
        m = np.where(qw < limit, qw, limit)
        carried = np.stack([np.where(got, s[ch] / ws, F(0)) for ch in range(3)]).astype(F)
        weight = np.where(got, m * ws, F(0)).astype(F)
    rejected = ~alive | (on & ~got)
    off = alive & ~on
    stats = (int(got.sum()), int(rejected.sum()), int(off.sum()), int(moved.sum()), int((moved & got).sum()))
    info = {"refused_by_owner": refused_by_owner, "class": np.where(got, 0, np.where(off, 2, 1)), "moved": moved, "void": void, "carried": got}
    return carried, weight, stats, info


# ---- the worlds: a wall and the sky (history_cases), a unit box under an instance transform in front, walked in float64 ----
def matrix64(p):
    """the same formula on the same quantised quaternion in binary64 throughout: what a float64 tracer maps a ray with"""
    p = np.asarray(p, F)
    a, b = (int(v) for v in p[6:8].view(U))
    u = np.array([1.0 - (a & 0xFFFF) / 32767.0, 1.0 - (a >> 16) / 32767.0, 1.0 - (b & 0xFFFF) / 32767.0])
    s = (b >> 16) / 32767.0 - 1.0
    M = np.zeros((3, 3))
    with np.errstate(all="ignore"):
        for j in range(3):
            v = np.zeros(3)
            v[j] = D(1.0) / D(p[3 + j])
            M[:, j] = 2.0 * np.dot(u, v) * u + (s * s - np.dot(u, u)) * v + 2.0 * s * np.cross(u, v)
    return M


def world_guides(key, box8, box_id, wall_id):
    """first hits of the centre rays: normal [3, P], depth [P], owner [P]. The box is [-1/2, 1/2]^3 in object space; box8 None or a transform that cannot be hit: no box."""
    normal, depth = H.guides_of(key)
    P = key.width * key.height
    owner = np.where(depth >= 0, U(wall_id), U(MISS)).astype(U)
    if box8 is None:
        return normal, depth, owner
    M = matrix64(box8)
    if not np.isfinite(M).all() or not np.isfinite(np.asarray(box8, F)[:3]).all() or abs(np.linalg.det(M)) == 0.0:
        return normal, depth, owner
    py, px = np.divmod(np.arange(P), key.width)
    dirs = np.stack(H.centre_ray(key, px.astype(F), py.astype(F))).astype(D)
    o = M @ (np.array(list(key.pos), D) - np.asarray(box8, F)[:3].astype(D))
    dd = M @ dirs
    with np.errstate(all="ignore"):
        t1, t2 = (-0.5 - o[:, None]) / dd, (0.5 - o[:, None]) / dd
        near, far = np.minimum(t1, t2), np.maximum(t1, t2)
        tn, tf = near.max(axis=0), far.min(axis=0)
        axis = near.argmax(axis=0)
    hit = (tn <= tf) & (tn > 0) & ((depth < 0) | (tn < depth))
    face = np.zeros((3, P))
    face[axis, np.arange(P)] = -np.sign(dd[axis, np.arange(P)])
    nw = M.T @ face
    nw /= np.maximum(np.sqrt((nw * nw).sum(axis=0, keepdims=True)), 1e-300)
    normal, depth = normal.copy(), depth.copy()
    normal[:, hit] = nw[:, hit].astype(F)
    depth[hit] = tn[hit].astype(F)
    owner[hit] = U(box_id)
    return normal, depth, owner


def quat(axis, angle):
    a = np.asarray(axis, D) / np.linalg.norm(axis)
    return tuple(a * np.sin(angle / 2)) + (float(np.cos(angle / 2)),)


# The box is a plate lying almost on the wall: its front face is 0.08 in front of it at a depth near 6.9, inside the default depth tolerance of 2 %, and nearly
# parallel to it. So depth and normal agree between the plate and the wall around it, and only the owners tell them apart: what the motion form adds is what decides.
BOX_Z, BOX_DEPTH = -5.95, 6.92
BASE_SCALE, BASE_QUAT = (1.8, 1.3, 0.06), quat((0, 1, 0), 0.05)
FAMILIES = ("t0.3", "t3", "t40", "rotated", "sheared", "rescaled", "both", "leaving", "void_scale", "void_nan", "foreign", "reserved")
# what a family has to show, from the restatement alone: carried pixels of the mover, taps refused by their owner, rejected pixels, pixels off the old frame
CLAIMS = {name: ("mover_carried", "refused", "rejected") for name in FAMILIES}
CLAIMS.update({"void_scale": ("mover_void", "rejected"), "void_nan": ("mover_void", "rejected"), "foreign": ("mover_void", "rejected")})


def family(name, width, height, count):
    """-> dict: old / now keys, old8 / new8 [count, 8], mover and wall ids, every plane the twins and the kernels take"""
    base, _ = H.keys(width, height)["identical"]
    old_key, now_key = base, base
    pixel = 2.0 * H.FOV / width * BOX_DEPTH  # world units per pixel at the box
    mover = count - 1
    wall = OCEAN if count == 1 or name == "reserved" else (7 if count > 7 else 0)
    cx, cy = H.BASE_POS[0], H.BASE_POS[1]
    t_new, t_old, s_new, s_old, q_new, q_old = [cx, cy, BOX_Z], [cx, cy, BOX_Z], BASE_SCALE, BASE_SCALE, BASE_QUAT, BASE_QUAT
    if name in ("t0.3", "t3", "t40", "reserved", "void_scale", "void_nan", "foreign"):
        shift = {"t0.3": 0.3, "t40": 40.0}.get(name, 3.0) * pixel
        if name == "t40":
            t_new[0] = cx + (0.35 * width) * pixel
        t_old[0] = t_new[0] - shift
        t_old[1] = t_new[1] - 0.2 * shift
    elif name == "rotated":
        q_new = quat((0.05, 0.1, 1), 0.4)
    elif name == "sheared":
        s_old = s_new = (2.4, 1.0, 0.06)
        q_old, q_new = quat((0, 0.3, 1), 0.5), quat((0, 0.3, 1), 0.9)
    elif name == "rescaled":
        s_new = (2.3, 1.0, 0.06)
    elif name == "both":
        now_key = H.keys(width, height)["translated"][1]
        t_old[0], q_new = t_new[0] - 3.0 * pixel, quat((0, 0.1, 1), 0.3)
    elif name == "leaving":
        t_new[0] = cx + H.FOV * BOX_DEPTH  # the box's centre on the frame's edge
        t_old[0] = t_new[0] - 1.0
    if name == "void_scale":
        s_old = (0.0, 1.3, 0.06)
    if name == "void_nan":
        t_old[0] = np.nan
    rng = np.random.default_rng(width + 1000 * FAMILIES.index(name) + count)
    old8, new8 = np.zeros((count, 8), F), np.zeros((count, 8), F)
    for i in range(count):  # the crowd: instances nobody sees, of every class
        old8[i] = words(rng.uniform(-40, 40, 3), rng.uniform(0.2, 3.0, 3), quat(rng.normal(size=3), rng.uniform(0, 3)))
        new8[i] = old8[i]
        kind = rng.integers(0, 4)
        if kind == 1:
            new8[i] = words(rng.uniform(-40, 40, 3), rng.uniform(0.2, 3.0, 3), quat(rng.normal(size=3), rng.uniform(0, 3)))
        elif kind == 2 and i % 5 == 0:
            new8[i][3 + i % 3] = [0.0, np.inf, np.nan][i % 3]
    if count > 1 and wall < count:
        new8[wall] = old8[wall]  # the wall stands
    old8[mover], new8[mover] = words(t_old, s_old, q_old), words(t_new, s_new, q_new)
    on, od, oo = world_guides(old_key, old8[mover], mover, wall)
    nn, nd, no = world_guides(now_key, new8[mover], mover, wall)
    if name == "foreign":
        no = np.where(no == U(mover), U(count + 5), no).astype(U)
    P, Q = width * height, width * height
    if name == "reserved":  # particles, and pixels without a path, scattered over both planes
        for plane, n in ((oo, Q), (no, P)):
            plane[rng.random(n) < 0.05] = U(PARTICLE)
            plane[rng.random(n) < 0.03] = U(EMPTY)
    old_shown = rng.gamma(2.0, 0.5, size=(3, Q)).astype(F)
    old_weight = rng.integers(1, 65, Q).astype(F)
    old_weight[rng.random(Q) < 0.03] = 0.0
    old_shown[rng.integers(0, 3), rng.integers(0, Q, max(Q // 60, 1))] = np.nan
    return {"old": old_key, "now": now_key, "old8": old8, "new8": new8, "mover": mover, "wall": wall, "normal": nn, "depth": nd, "owner": no, "old_normal": on, "old_depth": od,
            "old_owner": oo, "old_shown": old_shown, "old_weight": old_weight}


def check_claims(name, case, stats, info):
    """a family that silently carries nothing cannot pass"""
    mover_px = np.asarray(case["owner"], U) == U(case["mover"] if name != "foreign" else len(case["old8"]) + 5)
    for claim in CLAIMS[name]:
        if claim == "mover_carried":
            if name == "t40" and case["now"].width < 40:
                assert stats[2] > 0, (name, "forty pixels are more than this frame: the mover's pixels come from off the old frame")
            else:
                assert mover_px.any() and (info["carried"] & info["moved"] & mover_px).any(), (name, claim)
        elif claim == "refused":
            assert info["refused_by_owner"].sum() > 0, (name, claim)
        elif claim == "rejected":
            assert stats[1] > 0, (name, claim)
        elif claim == "mover_void":
            assert mover_px.any() and info["void"][mover_px].all() and not info["carried"][mover_px].any(), (name, claim)
