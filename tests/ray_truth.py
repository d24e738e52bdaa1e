"""A float64 truth for closest-hit ray queries, and an acceptor for what a float32 implementation may answer. Test infrastructure only.

The truth walks no tree: every (instance, triangle) pair of the scene is intersected with every ray in float64 (Moeller-Trumbore, the sequence of
dev_math.h intersect_triangle on the object-space ray of dev_trace.h). Next to every value it carries a forward error bound for what a float32
evaluation of the same sequence can return, in the standard model: every + - * returns the exact result times (1 + delta), |delta| <= 2^-24; the
reciprocal f = 1 / a may be a hardware reciprocal of 1 ulp, |delta| <= 2^-23; a result below the normal range may be flushed (2^-126 absolute).
The bound is a running error analysis: with x^ = x + ex, y^ = y + ey,
    x^ (+-) y^ = (x +- y) + [ex + ey]            and its rounding adds at most 2^-24 (|x +- y| + ex + ey),
    x^ * y^    = x y + [|x| ey + |y| ex + ex ey] and its rounding adds at most 2^-24 (|x y| + the bracket),
    1 / a^     = 1 / a + [ea / (|a| (|a| - ea))] and the reciprocal's own error is at most 2^-23 / (|a| - ea),
i.e. sums of absolute values of float64 quantities, divided by |a| where the sequence divides. Operations that IEEE arithmetic performs without
rounding are charged nothing: adding an exact zero, multiplying by an exact zero or power of two (an identity instance maps a ray exactly, and a
ray in the plane of an axis-aligned triangle gives a = 0 in float32 too). A contracted multiply-add rounds once instead of twice, so the same
bound covers code built with contraction. Nothing here is taken from what a device or the oracle returned.

Geometry is taken as the device sees it (oracle_lib.view_arrays): three float32 positions per triangle, of which the edges e1 = p1 - p0,
e2 = p2 - p0 are formed once, in float32, when the triangle is stored for the ray kernels; the instance transform is (translation, scale, quat16)
as dev_math.h documents, and the rows of the world -> object matrix are the twelve float32 numbers column j = xf_rel_inv(e_j) in dev_math.h's
operation order. Those float32 numbers are the scene; they are promoted to float64 and the rounding of the mapping itself (mat_row_apply on
origin - T and on the direction) enters the bounds like every other operation.
"""
import numpy as np

U = 2.0 ** -24          # unit roundoff of binary32: + - * and a correctly rounded /
U_RCP = 2.0 ** -23      # a hardware reciprocal (1 ulp)
ETA = 2.0 ** -126       # a result below the normal range may be flushed to zero
SKY = 0xFFFFFFFE        # instance word of "nothing hit" (dev_trace.h kHitSky)
NO_HANDLE = 0xFFFFFFFF

HIT, MISS, AMBIGUOUS = 1, -1, 0


# ---- (value, error bound) arithmetic on float64 arrays ----
def _exact(v):
    v = np.asarray(v, dtype=np.float64)
    return v, np.zeros_like(v)


def _round(v, prop, exact=False):
    """Bound after rounding a result whose exact value is v and whose inputs' errors propagate to `prop`; where `exact`, the operation rounds nothing."""
    mag = np.abs(v) + prop
    return prop + np.where(exact, 0.0, U * mag + ETA * (mag != 0.0))


def _is_zero(x):
    return (x[0] == 0.0) & (x[1] == 0.0)


def _is_power_of_two(x):  # an exactly known 0 or +-2^k: multiplying by it is exact (it is how an identity instance maps a ray)
    return (x[1] == 0.0) & ((x[0] == 0.0) | (np.abs(np.frexp(x[0])[0]) == 0.5))


def _add(x, y):
    v = x[0] + y[0]
    return v, _round(v, x[1] + y[1], _is_zero(x) | _is_zero(y))


def _sub(x, y):
    v = x[0] - y[0]
    return v, _round(v, x[1] + y[1], _is_zero(x) | _is_zero(y))


def _mul(x, y):
    v = x[0] * y[0]
    return v, _round(v, np.abs(x[0]) * y[1] + np.abs(y[0]) * x[1] + x[1] * y[1], _is_power_of_two(x) | _is_power_of_two(y))


def _dot(a, b):  # dev_math.h dot: (a.x * b.x + a.y * b.y) + a.z * b.z
    return _add(_add(_mul(a[0], b[0]), _mul(a[1], b[1])), _mul(a[2], b[2]))


def _cross(a, b):
    return (_sub(_mul(a[1], b[2]), _mul(a[2], b[1])), _sub(_mul(a[2], b[0]), _mul(a[0], b[2])), _sub(_mul(a[0], b[1]), _mul(a[1], b[0])))


# ---- the scene as the device sees it ----
def _f32(words):
    return np.ascontiguousarray(words, dtype=np.uint32).view(np.float32)


def _inverse_rows(transform_words):
    """Rows of the world -> object matrix of one instance, float32, in the operation order of dev_math.h: column j = xf_rel_inv(e_j) =
    qapply(quat16_inv(t), e_j * vinv(t.scale)). Returns (rows [3, 3] float32, translation [3] float32)."""
    f = np.float32
    w = np.ascontiguousarray(transform_words, dtype=np.uint32)
    p = w.view(np.float32)
    a, b = int(w[6]), int(w[7])
    k = f(1.0) / f(0x7FFF)
    ux, uy = f(1.0) - f(a & 0xFFFF) * k, f(1.0) - f(a >> 16) * k
    uz, s = f(1.0) - f(b & 0xFFFF) * k, f(b >> 16) * k - f(1.0)
    inv_scale = [f(1.0) / p[3], f(1.0) / p[4], f(1.0) / p[5]]
    rows = np.zeros((3, 3), dtype=np.float32)
    for j in range(3):
        vx, vy, vz = [f(1.0 if i == j else 0.0) * inv_scale[i] for i in range(3)]
        duv = ux * vx + uy * vy + uz * vz
        duu = ux * ux + uy * uy + uz * uz
        cx, cy, cz = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
        k0, k1, k2 = f(2.0) * duv, s * s - duu, f(2.0) * s
        rows[0, j] = (ux * k0 + vx * k1) + cx * k2
        rows[1, j] = (uy * k0 + vy * k1) + cy * k2
        rows[2, j] = (uz * k0 + vz * k1) + cz * k2
    return rows, p[0:3].copy()


class Scene:
    """Triangles and instances read from a DeviceSceneView; every pair (instance, triangle of its mesh) has an index."""

    def __init__(self, arrays):
        off = np.asarray(arrays["mesh_tri_offset"], dtype=np.int64)
        v = _f32(arrays["vertices"]).reshape(-1, 3, 4)[:, :, 0:3]
        self.p0 = v[:, 0, :].astype(np.float64)
        self.e1 = (v[:, 1, :] - v[:, 0, :]).astype(np.float64)  # float32 subtraction: rounded once, as stored for the ray kernels
        self.e2 = (v[:, 2, :] - v[:, 0, :]).astype(np.float64)
        mesh_ids = np.asarray(arrays["instance_mesh_ids"], dtype=np.uint32)
        tf = np.asarray(arrays["instance_transforms"], dtype=np.uint32).reshape(-1, 8)
        self.instances = []  # (instance id, first triangle, triangle count, rows float64, translation float64, first pair)
        self.pair_base = {}
        pairs = 0
        for i, m in enumerate(mesh_ids):
            if int(m) + 1 >= off.size:
                continue  # inactive instance
            first, count = int(off[m]), int(off[m + 1] - off[m])
            if count == 0:
                continue
            with np.errstate(all="ignore"):
                rows, tr = _inverse_rows(tf[i])
            if not np.all(np.isfinite(rows)):
                continue
            self.instances.append((i, first, count, rows.astype(np.float64), tr.astype(np.float64), pairs))
            self.pair_base[i] = (pairs, first, count)
            pairs += count
        self.num_pairs = pairs

    def pair_of(self, inst, tri):
        """Pair index of the handles (arrays); -1 where they name nothing."""
        inst = np.asarray(inst, dtype=np.int64)
        tri = np.asarray(tri, dtype=np.int64)
        out = np.full(inst.shape, -1, dtype=np.int64)
        for i, (base, _, count) in self.pair_base.items():
            sel = (inst == i) & (tri < count)
            out[sel] = base + tri[sel]
        return out

    def handle_of(self, pair):
        pair = np.asarray(pair, dtype=np.int64)
        inst = np.full(pair.shape, SKY, dtype=np.uint32)
        tri = np.zeros(pair.shape, dtype=np.uint32)
        for i, (base, _, count) in self.pair_base.items():
            sel = (pair >= base) & (pair < base + count)
            inst[sel] = i
            tri[sel] = (pair[sel] - base).astype(np.uint32)
        return inst, tri


def scene_of_view(view):
    import oracle_lib
    return Scene(oracle_lib.view_arrays(view))


# ---- one block of pairs ----
def _object_ray(rows, tr, o, d):
    """World ray [R, 3] -> object-space origin and direction as three (value, bound) components [R, 1] each."""
    p = [_sub(_exact(o[:, k:k + 1]), _exact(tr[k])) for k in range(3)]
    dd = [_exact(d[:, k:k + 1]) for k in range(3)]

    def row(r, x):  # mat_row_apply: (a * x + b * y) + c * z
        return _add(_add(_mul(_exact(r[0]), x[0]), _mul(_exact(r[1]), x[1])), _mul(_exact(r[2]), x[2]))
    return [row(rows[k], p) for k in range(3)], [row(rows[k], dd) for k in range(3)]


def _intersect(oo, od, p0, e1, e2):
    """intersect_triangle on object rays (lists of three (value, bound), shape [R, 1] or [R]) against triangles ([1, T, 3] -> components [1, T], or [R, 3]).
    Returns (cls, t, bt): the class of every pair, its float64 distance and the bound of a float32 distance (inf where `a` cannot be trusted)."""
    V = [_exact(p0[..., k]) for k in range(3)]
    E1 = [_exact(e1[..., k]) for k in range(3)]
    E2 = [_exact(e2[..., k]) for k in range(3)]
    with np.errstate(all="ignore"):
        h = _cross(od, E2)
        a = _dot(E1, h)
        s = [_sub(oo[k], V[k]) for k in range(3)]
        nu = _dot(s, h)
        q = _cross(s, E1)
        nv = _dot(od, q)
        nt = _dot(E2, q)
        a_ok = np.abs(a[0]) > a[1]
        room = np.where(a_ok, np.abs(a[0]) - a[1], 1.0)
        safe_a = np.where(a_ok, a[0], 1.0)
        f = (1.0 / safe_a, a[1] / (np.abs(safe_a) * room) + U_RCP / room + ETA)
        u, v, t = _mul(f, nu), _mul(f, nv), _mul(f, nt)
        bsum = u[1] + v[1] + 2.0 * U  # u + v is rounded once more before it is compared with 1
        hit = a_ok & (u[0] >= u[1]) & (v[0] >= v[1]) & (u[0] + v[0] <= 1.0 - (u[1] + v[1])) & (t[0] >= t[1])
        miss = a_ok & ((u[0] < -u[1]) | (v[0] < -v[1]) | (u[0] + v[0] > 1.0 + bsum) | (t[0] < -t[1]))
        # `a` within its bound of zero: f^ may be anything finite or an infinity, of either sign - but of one sign for u, v and t. Two numerators of
        # certainly opposite signs make one of u^, v^, t^ negative (or minus infinity): a miss. An `a` that is exactly zero in float32 too (every
        # term a product with an exact zero: a ray in the plane of an axis-aligned triangle) gives infinities or NaN, which the comparisons reject.
        sg = [np.where(n[0] > n[1], 1, np.where(n[0] < -n[1], -1, 0)) for n in (nu, nv, nt)]
        opposite = (sg[0] * sg[1] < 0) | (sg[0] * sg[2] < 0) | (sg[1] * sg[2] < 0)
        miss |= ~a_ok & (opposite | ((a[0] == 0.0) & (a[1] == 0.0)))
    cls = np.where(hit, HIT, np.where(miss, MISS, AMBIGUOUS)).astype(np.int8)
    return cls, np.where(a_ok, t[0], 0.0), np.where(a_ok, t[1], np.inf)


class Solution:
    """What the truth knows about a set of rays. `check` is the acceptor."""

    def __init__(self, scene, o, d, ignore_pair, nearest_upper, num_acceptable, the_acceptable, farther_hit):
        self.scene, self.o, self.d, self.ignore_pair = scene, o, d, ignore_pair
        self.nearest_upper = nearest_upper      # min over certain hits of t + bt (inf: none)
        self.num_acceptable = num_acceptable    # pairs that may be answered
        self.the_acceptable = the_acceptable    # one of them (-1: none)
        self.farther_hit = farther_hit          # a certain hit that is certainly farther than the nearest one (-1: none)
        self.has_certain_hit = np.isfinite(nearest_upper)
        self.decisive = np.where(self.has_certain_hit, num_acceptable == 1, num_acceptable == 0)

    def expected(self):
        """The one acceptable (instance, triangle) of every decisive ray ((SKY, 0) for a miss); meaningless elsewhere."""
        pair = np.where(self.has_certain_hit, self.the_acceptable, -1)
        return self.scene.handle_of(pair)

    def pair_values(self, pair):
        """(class, t, bt) of one pair per ray (pair < 0: MISS)."""
        sc = self.scene
        cls = np.full(pair.shape, MISS, dtype=np.int8)
        t = np.zeros(pair.shape)
        bt = np.full(pair.shape, np.inf)
        for (_, first, count, rows, tr, base) in sc.instances:
            sel = np.nonzero((pair >= base) & (pair < base + count))[0]
            if sel.size == 0:
                continue
            g = first + (pair[sel] - base)
            oo, od = _object_ray(rows, tr, self.o[sel], self.d[sel])
            oo = [(x[0][:, 0], x[1][:, 0]) for x in oo]
            od = [(x[0][:, 0], x[1][:, 0]) for x in od]
            cls[sel], t[sel], bt[sel] = _intersect(oo, od, sc.p0[g], sc.e1[g], sc.e2[g])
        return cls, t, bt

    def check(self, answers):
        """answers [R, 3] uint32 (instance, triangle, t bits) as trace_closest_host returns them. Returns (ok [R] bool, reason [R] of str or None).
        Sky is acceptable iff no pair is a certain hit. A hit on pair k is acceptable iff k is not ignored and not a certain miss, the distance lies
        within bt_k of t_k, and no certain hit lies certainly nearer (t_j + bt_j < t_k - bt_k)."""
        answers = np.ascontiguousarray(answers, dtype=np.uint32)
        n = answers.shape[0]
        ok = np.zeros(n, dtype=bool)
        reason = np.full(n, None, dtype=object)
        sky = answers[:, 0] == SKY
        ok[sky] = ~self.has_certain_hit[sky]
        reason[sky & ~ok] = "sky, but a triangle is certainly hit"
        idx = np.nonzero(~sky)[0]
        if idx.size:
            pair = np.full(n, -1, dtype=np.int64)
            pair[idx] = self.scene.pair_of(answers[idx, 0], answers[idx, 1])
            cls, t, bt = self.pair_values(pair)
            t_dev = answers[:, 2].copy().view(np.float32).astype(np.float64)
            for i in idx:
                if pair[i] < 0:
                    reason[i] = "no such (instance, triangle)"
                elif pair[i] == self.ignore_pair[i]:
                    reason[i] = "the ignored triangle"
                elif cls[i] == MISS:
                    reason[i] = "a triangle the ray certainly misses"
                elif not abs(t_dev[i] - t[i]) <= bt[i]:
                    reason[i] = "t = %.9g, truth %.17g +- %.3g" % (t_dev[i], t[i], bt[i])
                elif self.nearest_upper[i] < t[i] - bt[i]:
                    reason[i] = "a certain hit lies nearer (below %.9g; this one %.9g - %.3g)" % (self.nearest_upper[i], t[i], bt[i])
                else:
                    ok[i] = True
        return ok, reason

    def describe(self, i, answer=None):
        """One ray, the truth's pair and (optionally) an answer, for failure messages."""
        inst, tri = self.scene.handle_of(np.array([self.the_acceptable[i]]))
        one = Solution(self.scene, self.o[i:i + 1], self.d[i:i + 1], self.ignore_pair[i:i + 1], self.nearest_upper[i:i + 1], self.num_acceptable[i:i + 1],
                       self.the_acceptable[i:i + 1], self.farther_hit[i:i + 1])
        cls, t, bt = one.pair_values(self.the_acceptable[i:i + 1])
        s = "ray %d o=%s d=%s | truth: %d acceptable pair(s), certain hit %s, one of them (inst %d, tri %d) t=%.17g bt=%.3g" % (
            i, [float(x) for x in self.o[i]], [float(x) for x in self.d[i]], int(self.num_acceptable[i]), bool(self.has_certain_hit[i]), int(inst[0]), int(tri[0]),
            float(t[0]), float(bt[0]))
        if answer is not None:
            a = np.ascontiguousarray(answer, dtype=np.uint32)
            s += " | answer (inst %d, tri %d) t=%.9g" % (int(a[0]), int(a[1]), float(a[2:3].view(np.float32)[0]))
        return s


def solve(scene, origins, dirs, ignore=None, block=400_000):
    """Brute force over every pair, in blocks of about `block` pairs."""
    o = np.ascontiguousarray(origins, dtype=np.float32).astype(np.float64)
    d = np.ascontiguousarray(dirs, dtype=np.float32).astype(np.float64)
    n = o.shape[0]
    ignore_pair = np.full(n, -1, dtype=np.int64)
    if ignore is not None:
        ignore = np.ascontiguousarray(ignore, dtype=np.uint32)
        ignore_pair = scene.pair_of(ignore[:, 0], ignore[:, 1])
    nearest_upper = np.full(n, np.inf)
    num_acc = np.zeros(n, dtype=np.int64)
    the_acc = np.full(n, -1, dtype=np.int64)
    farther = np.full(n, -1, dtype=np.int64)
    step = max(1, block // max(scene.num_pairs, 1))
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        blocks = []
        for (_, first, count, rows, tr, base) in scene.instances:
            oo, od = _object_ray(rows, tr, o[r0:r1], d[r0:r1])
            sl = slice(first, first + count)
            cls, t, bt = _intersect(oo, od, scene.p0[None, sl], scene.e1[None, sl], scene.e2[None, sl])
            ig = ignore_pair[r0:r1, None] == (base + np.arange(count))[None, :]
            cls = np.where(ig, MISS, cls)  # an ignore handle excludes the pair outright
            blocks.append((base, cls, t, bt))
        upper = np.full(r1 - r0, np.inf)
        for (_, cls, t, bt) in blocks:
            upper = np.minimum(upper, np.where(cls == HIT, t + bt, np.inf).min(axis=1))
        nearest_upper[r0:r1] = upper
        far_t = np.full(r1 - r0, np.inf)
        for (base, cls, t, bt) in blocks:
            acc = (cls != MISS) & ~(upper[:, None] < t - bt)
            num_acc[r0:r1] += acc.sum(axis=1)
            any_acc = acc.any(axis=1)
            first_acc = base + acc.argmax(axis=1)
            the_acc[r0:r1] = np.where(any_acc & (the_acc[r0:r1] < 0), first_acc, the_acc[r0:r1])
            far = (cls == HIT) & (upper[:, None] < t - bt)
            ft = np.where(far, t, np.inf)
            j = ft.argmin(axis=1)
            best = ft[np.arange(r1 - r0), j]
            better = best < far_t
            farther[r0:r1] = np.where(better, base + j, farther[r0:r1])
            far_t = np.where(better, best, far_t)
    return Solution(scene, o, d, ignore_pair, nearest_upper, num_acc, the_acc, farther)
