"""What tests/test_history.py and tests/test_history_gpu.py share: a numpy float32 restatement of csrc/host/history.h written from the header's text (every
operation on float32 arrays, one at a time, in the header's order), the camera keys and the synthetic planes. Not a test file."""
import numpy as np

from luminary_amd import core

F, U = np.float32, np.uint32
FRAMES = ((7, 5), (50, 31), (64, 64))  # less than a wave; a part-empty last wave and workgroup; exact 32 x 8 tiles
FOV = 0.6


# ---- the definition, restated ----
def dot(a, b):
    tx = a[0] * b[0]
    ty = a[1] * b[1]
    tz = a[2] * b[2]
    s = tx + ty
    return s + tz


def rotate(q, v):
    qx, qy, qz, qw = (F(c) for c in q)
    u = (qx, qy, qz)
    duv, duu = dot(u, v), dot(u, u)
    cr = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
    t = F(2) * duv
    k = qw * qw - duu
    m = F(2) * qw
    return tuple((u[i] * t + v[i] * k) + cr[i] * m for i in range(3))


def frame(key):
    step = F(2) * (F(key.fov) / F(key.width))
    return step, (step * F(key.height)) * F(0.5)


def centre_ray(key, px, py):
    """px, py: float32 arrays of pixel coordinates"""
    step, vfov = frame(key)
    sx = F(key.fov) - step * (px + F(0.5))
    sy = step * (py + F(0.5)) - vfov
    c = (-sx, -sy, np.full_like(sx, F(-1)))
    l = np.sqrt(dot(c, c))
    return rotate(tuple(key.rotation), (c[0] / l, c[1] / l, c[2] / l))


def project(key, v):
    q = tuple(key.rotation)
    dc = rotate((-F(q[0]), -F(q[1]), -F(q[2]), F(q[3])), v)
    step, vfov = frame(key)
    with np.errstate(all="ignore"):
        valid = dc[2] < F(0)
        fx = (F(key.fov) - dc[0] / dc[2]) / step - F(0.5)
        fy = (dc[1] / dc[2] + vfov) / step - F(0.5)
    return valid, fx, fy


def finite(a):
    return (a.view(U) & U(0x7F800000)) != U(0x7F800000)


def reproject(now, old, st, normal, depth, old_shown, old_weight, old_normal, old_depth):
    """-> carried [3, P], carried_weight [P], (carried, rejected, off)"""
    w, h, ow, oh = now.width, now.height, old.width, old.height
    P = w * h
    normal, depth = np.asarray(normal, F).reshape(3, P), np.asarray(depth, F).reshape(P)
    old_shown, old_weight = np.asarray(old_shown, F).reshape(3, ow * oh), np.asarray(old_weight, F).reshape(ow * oh)
    old_normal, old_depth = np.asarray(old_normal, F).reshape(3, ow * oh), np.asarray(old_depth, F).reshape(ow * oh)
    py, px = np.divmod(np.arange(P), w)
    with np.errstate(all="ignore"):
        d = centre_ray(now, px.astype(F), py.astype(F))
        surface = depth >= F(0)
        X = tuple(F(now.pos[i]) + d[i] * depth for i in range(3))
        vs = tuple(X[i] - F(old.pos[i]) for i in range(3))
        v = tuple(np.where(surface, vs[i], d[i]) for i in range(3))
        r = np.where(surface, np.sqrt(dot(v, v)), F(0))
        valid, fx, fy = project(old, v)
        on = valid & (fx >= F(-1)) & (fx < F(ow)) & (fy >= F(-1)) & (fy < F(oh))
        fx, fy = np.where(on, fx, F(0)), np.where(on, fy, F(0))
        x0f, y0f = np.floor(fx), np.floor(fy)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        tx, ty = fx - x0f, fy - y0f
        ux, uy = F(1) - tx, F(1) - ty
        tol = F(st.depth_tolerance) * r
        ws, sw = np.zeros(P, F), np.zeros(P, F)
        s = [np.zeros(P, F) for _ in range(3)]
        for k in range(4):
            x, y = x0 + (k & 1), y0 + (k >> 1)
            wt = (tx if k & 1 else ux) * (ty if k >> 1 else uy)
            inside = on & (x >= 0) & (y >= 0) & (x < ow) & (y < oh)
            q = np.where(inside, y * ow + x, 0)
            gn, gd = old_normal[:, q], old_depth[q]
            dd = gd - r
            ad = np.where(dd < F(0), -dd, dd)
            geo = np.where(surface, (gd >= F(0)) & (ad <= tol) & (dot(normal, gn) >= F(st.normal_threshold)), gd < F(0))
            sh, swt = old_shown[:, q], old_weight[q]
            ok = inside & geo & finite(sh[0]) & finite(sh[1]) & finite(sh[2]) & finite(swt) & (swt > F(0))
            ws = np.where(ok, ws + wt, ws)
            for c in range(3):
                s[c] = np.where(ok, s[c] + wt * sh[c], s[c])
            sw = np.where(ok, sw + wt * swt, sw)
        got = on & (ws > F(0))
        qw = sw / ws
        m = np.where(qw < F(st.max_history), qw, F(st.max_history))
        carried = np.stack([np.where(got, s[c] / ws, F(0)) for c in range(3)]).astype(F)
        weight = np.where(got, m * ws, F(0)).astype(F)
    return carried, weight, (int(got.sum()), int((on & ~got).sum()), int((~on).sum()))


def blend(st, width, height, samples, image, carried=None, carried_weight=None):
    """-> image after the blend [3, P], shown [3, P], weight [P]"""
    P = width * height
    cur = np.asarray(image, F).reshape(3, P)
    C = np.zeros((3, P), F) if carried is None else np.asarray(carried, F).reshape(3, P)
    W = np.zeros(P, F) if carried_weight is None else np.asarray(carried_weight, F).reshape(P)
    N = F(samples)
    y, x = np.divmod(np.arange(P), width)
    fin = finite(cur[0]) & finite(cur[1]) & finite(cur[2])
    with np.errstate(all="ignore"):
        mix = fin & (W > F(0))
        c = [C[ch].copy() for ch in range(3)]
        if st.clamp_sigma > 0:
            taps = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
            exists = [(x + dx >= 0) & (x + dx < width) & (y + dy >= 0) & (y + dy < height) for dx, dy in taps]
            index = [np.where(e, (y + dy) * width + (x + dx), 0) for e, (dx, dy) in zip(exists, taps)]
            k = sum(e.astype(np.int64) for e in exists).astype(F)
            for ch in range(3):
                s = np.zeros(P, F)
                for e, i in zip(exists, index):
                    s = np.where(e, s + cur[ch][i], s)
                mean = s / k
                q = np.zeros(P, F)
                for e, i in zip(exists, index):
                    dlt = cur[ch][i] - mean
                    q = np.where(e, q + dlt * dlt, q)
                sigma = np.sqrt(q / k)
                ext = F(st.clamp_sigma) * sigma
                lo, hi = mean - ext, mean + ext
                c[ch] = np.where(c[ch] < lo, lo, np.where(c[ch] > hi, hi, c[ch]))
        den = W + N
        shown = np.stack([np.where(mix, (W * c[ch] + N * cur[ch]) / den, cur[ch]) for ch in range(3)]).astype(F)
        weight = np.where(fin, np.where(mix, den, N), F(0)).astype(F)
    return shown.copy(), shown, weight


# ---- keys ----
def quat_y(angle):
    return (0.0, float(np.sin(angle / 2)), 0.0, float(np.cos(angle / 2)))


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return (aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz)


BASE_POS, BASE_ROT = (0.25, 0.5, 1.0), quat_mul(quat_y(0.05), (float(np.sin(-0.04)), 0.0, 0.0, float(np.cos(-0.04))))


def keys(width, height):
    """{name: (old key, new key)}: every pair the issue lists"""
    base = core.history_key(BASE_POS, BASE_ROT, FOV, width, height)
    k = lambda pos=BASE_POS, rot=BASE_ROT, fov=FOV: core.history_key(pos, rot, fov, width, height)
    return {"identical": (base, k()), "translated": (base, k(pos=(0.45, 0.4, 1.3))), "rotated": (base, k(rot=quat_mul(quat_y(0.12), BASE_ROT))), "fov": (base, k(fov=0.5)),
            "turned": (base, k(rot=quat_mul(quat_y(np.pi), BASE_ROT))), "half_off": (base, k(pos=(BASE_POS[0] + 4.2, BASE_POS[1], BASE_POS[2])))}


# ---- planes ----
WALL_Z, WALL_X, WALL_Y = -6.0, 5.0, (-3.0, 1.6)  # a wall facing +z; beyond its edges the sky


def guides_of(key):
    """first-hit guides of the wall world seen from `key`, by a float64 walk of the centre rays: normal [3, P], depth [P] (depth -1, normal 0: sky)"""
    w, h = key.width, key.height
    py, px = np.divmod(np.arange(w * h), w)
    d = np.stack(centre_ray(key, px.astype(F), py.astype(F))).astype(np.float64)
    pos = np.array(list(key.pos), np.float64)
    with np.errstate(all="ignore"):
        t = (WALL_Z - pos[2]) / d[2]
        hx, hy = pos[0] + t * d[0], pos[1] + t * d[1]
    hit = (d[2] < 0) & (t > 0) & (np.abs(hx) < WALL_X) & (hy > WALL_Y[0]) & (hy < WALL_Y[1])
    depth = np.where(hit, t, -1.0).astype(F)
    normal = np.zeros((3, w * h), F)
    normal[2] = np.where(hit, 1.0, 0.0)
    return normal, depth


def planes(old, now, seed, hostile=True, random_guides=False):
    """a dict of everything the twins and the kernels take: the new guides, the old state, a new image"""
    rng = np.random.default_rng(seed)
    P, Q = now.width * now.height, old.width * old.height
    normal, depth = guides_of(now)
    old_normal, old_depth = guides_of(old)
    if random_guides:  # no geometry at all: every branch of the tap test at random
        normal = rng.normal(size=(3, P)).astype(F)
        normal /= np.sqrt((normal * normal).sum(axis=0, keepdims=True))
        depth = np.where(rng.random(P) < 0.25, -1.0, rng.uniform(0.0, 12.0, P)).astype(F)
        old_normal = rng.normal(size=(3, Q)).astype(F)
        old_depth = np.where(rng.random(Q) < 0.25, -1.0, rng.uniform(0.0, 12.0, Q)).astype(F)
    old_shown = rng.gamma(2.0, 0.5, size=(3, Q)).astype(F)
    old_weight = rng.integers(1, 65, Q).astype(F)
    image = rng.gamma(2.0, 0.5, size=(3, P)).astype(F)
    if hostile:
        flip = rng.random(Q) < 0.06  # an edge: the old normal turned away
        old_normal[:, flip] = -old_normal[:, flip]
        old_depth[rng.random(Q) < 0.04] *= F(1.5)  # a depth step
        old_weight[rng.random(Q) < 0.08] = 0.0
        for bad in (np.nan, np.inf, -np.inf):
            old_shown[rng.integers(0, 3), rng.integers(0, Q, max(Q // 40, 1))] = bad
            image[rng.integers(0, 3), rng.integers(0, P, max(P // 50, 1))] = bad
        old_weight[rng.integers(0, Q, 2)] = np.inf
        depth[rng.integers(0, P, 2)] = np.nan
    return {"normal": normal, "depth": depth, "old_shown": old_shown, "old_weight": old_weight, "old_normal": old_normal, "old_depth": old_depth, "image": image}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(U), b.view(U))
