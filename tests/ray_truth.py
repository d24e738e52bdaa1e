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


# ---- visibility rays: what a segment (eps, dist) certainly crosses, and which transparency products a float32 implementation may answer ----
# The pairs are classified with _object_ray and _intersect as they stand, nothing added to their bounds. With the float64 distance t, its float32 bound bt,
# eps = kEps and the float32 dist of the ray, a pair that is neither the target nor self is
#   certainly crossed      class HIT and t - bt > eps and t + bt < dist,
#   certainly not crossed  class MISS, or t + bt <= eps, or t - bt >= dist,
#   ambiguous              otherwise.
# The factor of a pair is what ShadowState::on_tris (dev_trace.h) multiplies in, restated in float32 on the material words the device reads: alpha 1 is
# opaque, alpha 0 uncoloured is absent, otherwise 1 - alpha, times the albedo where the material has coloured transparency. A textured material is supported
# only where every texel of its texture is the same (and its gamma is 1): the bilinear fetch then returns that texel whatever uv is.
# NOT covered: uv-dependent textured alpha, the ambient-reuse equivalence (a closest-hit ray answering a visibility question), the particle tree.
K_EPS = float(np.float32(1.1920928955078125e-7))  # dev_math.h kEps
ABSENT, FACTOR, OPAQUE = 0, 1, 2
MAX_AMBIGUOUS = 6   # subsets are enumerated up to 2^6 per ray; a ray with more ambiguous pairs is undecided
MAX_FACTORS = 12    # with factors >= 2^-6 nothing underflows
DMAT_COLOURED = 0x10


def _unorm16(d):
    return np.asarray(d, dtype=np.uint32).astype(np.float32) * (np.float32(1.0) / np.float32(0xFFFF))


def surface_factors(view):
    """(kind [T] of ABSENT / FACTOR / OPAQUE, factor [T, 3] float32) per scene triangle, from the material words and the textures of a DeviceSceneView."""
    import ctypes as C
    import oracle_lib
    a = oracle_lib.view_arrays(view)
    m = a["materials"].reshape(-1, 16).astype(np.uint32)
    coloured = (m[:, 0] & DMAT_COLOURED) != 0
    albedo, alpha = _unorm16(m[:, 4:7]), _unorm16(m[:, 7])
    ntex = int(view.num_textures)
    table = oracle_lib._array(view.texture_table, C.c_uint32, 4 * ntex).reshape(-1, 4)
    texels = oracle_lib._array(view.texels, C.c_uint32, int((table[:, 0] + table[:, 1] * table[:, 2]).max()) if ntex else 0)
    for i in range(len(m)):
        tex = int(m[i, 12])
        if tex == 0xFFFF:
            continue
        if tex >= ntex:
            albedo[i], alpha[i] = np.float32(0.9), np.float32(1.0)
            continue
        first, w, h, gamma = [int(x) for x in table[tex]]
        tx = texels[first:first + w * h]
        assert (tx == tx[0]).all() and np.uint32(gamma).view(np.float32) == 1.0, "the truth supports constant-texel textures of gamma 1 only"
        c = np.array([tx[0] & 0xFF, (tx[0] >> 8) & 0xFF, (tx[0] >> 16) & 0xFF, tx[0] >> 24], dtype=np.uint32).astype(np.float32) * (np.float32(1.0) / np.float32(255.0))
        albedo[i], alpha[i] = c[0:3], c[3]
    tp = np.float32(1.0) - alpha
    f = np.where(coloured[:, None], albedo * tp[:, None], np.repeat(tp[:, None], 3, axis=1)).astype(np.float32)
    kind = np.where(alpha == 1.0, OPAQUE, np.where((alpha == 0.0) & ~coloured, ABSENT, FACTOR)).astype(np.int8)
    mat = a["tri_tex"].reshape(-1, 4)[:, 3] & 0xFFFF
    return kind[mat], f[mat]


def _half_ulp32(p):
    """Half a float32 ulp at the magnitude of the float64 values p (normal range)."""
    _, e = np.frexp(np.abs(p))
    return np.where(p == 0.0, 0.0, np.ldexp(1.0, e - 25))


class VisibilitySolution:
    """What the truth knows about a set of visibility rays. `check` is the acceptor."""

    def __init__(self, finite, must_block, may_block, product, k_certain, amb_factors, num_ambiguous, one_factor):
        self.finite = finite                # the ray's origin and direction are finite (a non-finite ray crosses nothing: (1, 1, 1))
        self.must_block = must_block        # an opaque pair is certainly crossed
        self.may_block = may_block          # an opaque pair is ambiguous
        self.product = product              # [R, 3] longdouble: product of the certainly crossed factors
        self.k_certain = k_certain          # their number
        self.amb_factors = amb_factors      # per ray: list of float32 [3] factors of the ambiguous non-opaque pairs
        self.num_ambiguous = num_ambiguous  # ambiguous pairs, the opaque ones included
        self.one_factor = one_factor        # [R, 3] float32: one of the certainly crossed factors (1 where there is none), for mutation tests
        self.undecided = num_ambiguous > MAX_AMBIGUOUS
        self.decisive = (num_ambiguous == 0) | ~finite

    def expected(self):
        """The one acceptable answer of every decisive ray: the product rounded once ([R, 3] float32; 0 where blocked)."""
        p = np.where(self.must_block[:, None], 0.0, self.product.astype(np.float64)).astype(np.float32)
        p[~self.finite] = 1.0
        return p

    def check(self, answers, fast=False):
        """answers [R, 3] float32. Returns (ok [R], reason [R]). Zero is required where an opaque pair is certainly crossed and allowed where one is ambiguous;
        otherwise all three channels must be the certainly crossed product times the factors of ONE subset of the ambiguous pairs: within half a float32 ulp plus
        2^-50 relative (the exact flavour: a binary64 product rounded once), or within (k - 1) u / (1 - (k - 1) u), u = 2^-24, for k factors (`fast`: a binary32
        product in any order)."""
        ans = np.ascontiguousarray(answers, dtype=np.float32).astype(np.float64)
        n = len(ans)
        ok = np.zeros(n, dtype=bool)
        reason = np.full(n, None, dtype=object)
        for i in range(n):
            a = ans[i]
            if not np.all(np.isfinite(a)):
                reason[i] = "not a number: %s (a ray nobody answered keeps the NaN pattern)" % a
                continue
            if not self.finite[i]:
                ok[i] = bool(np.all(a == 1.0))
                reason[i] = None if ok[i] else "a non-finite ray crosses nothing: (1, 1, 1), not %s" % a
                continue
            if self.undecided[i]:
                ok[i] = True
                continue
            zero = bool(np.all(a == 0.0))
            if self.must_block[i]:
                ok[i] = zero
                reason[i] = None if zero else "an opaque surface is certainly crossed, answer %s" % a
                continue
            if zero and self.may_block[i]:
                ok[i] = True
                continue
            fs = self.amb_factors[i]
            best = None
            for subset in range(1 << len(fs)):
                p = self.product[i].copy()
                k = int(self.k_certain[i])
                for j in range(len(fs)):
                    if subset >> j & 1:
                        p = p * fs[j].astype(np.longdouble)
                        k += 1
                p = p.astype(np.float64)
                if fast:
                    ku = max(k - 1, 0) * U
                    tol = np.abs(p) * (ku / (1.0 - ku))
                else:
                    tol = _half_ulp32(p) + np.abs(p) * 2.0 ** -50
                err = np.abs(a - p)
                if np.all(err <= tol):
                    ok[i] = True
                    break
                if best is None or err.max() < best[0]:
                    best = (err.max(), p, tol, k)
            if not ok[i]:
                reason[i] = "answer %s; nearest admissible product %s (k = %d, tolerance %s), %d ambiguous pair(s)%s" % (
                    a, best[1], best[3], best[2], int(self.num_ambiguous[i]), ", zero only if blocked" if zero else "")
        return ok, reason


def solve_visibility(scene, kind, factor, origins, dirs, dist, ids, block=400_000):
    """Brute force over every pair, like solve. kind / factor: surface_factors; dist [R] float32; ids [R, 4]: target and self handles."""
    o32, d32 = np.ascontiguousarray(origins, dtype=np.float32), np.ascontiguousarray(dirs, dtype=np.float32)
    finite = np.isfinite(o32).all(axis=1) & np.isfinite(d32).all(axis=1)
    o = np.where(finite[:, None], o32, 0.0).astype(np.float64)
    d = np.where(finite[:, None], d32, 1.0).astype(np.float64)
    dist = np.ascontiguousarray(dist, dtype=np.float32).astype(np.float64)
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    n = o.shape[0]
    tgt, slf = scene.pair_of(ids[:, 0], ids[:, 1]), scene.pair_of(ids[:, 2], ids[:, 3])
    must = np.zeros(n, dtype=bool)
    may = np.zeros(n, dtype=bool)
    product = np.ones((n, 3), dtype=np.longdouble)
    k_certain = np.zeros(n, dtype=np.int64)
    num_amb = np.zeros(n, dtype=np.int64)
    amb = [[] for _ in range(n)]
    one = np.ones((n, 3), dtype=np.float32)
    step = max(1, block // max(scene.num_pairs, 1))
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        for (_, first, count, rows, tr, base) in scene.instances:
            oo, od = _object_ray(rows, tr, o[r0:r1], d[r0:r1])
            sl = slice(first, first + count)
            cls, t, bt = _intersect(oo, od, scene.p0[None, sl], scene.e1[None, sl], scene.e2[None, sl])
            pair = (base + np.arange(count))[None, :]
            skipped = (tgt[r0:r1, None] == pair) | (slf[r0:r1, None] == pair) | (kind[sl] == ABSENT)[None, :] | ~finite[r0:r1, None]
            dd = dist[r0:r1, None]
            with np.errstate(invalid="ignore"):
                crossed = (cls == HIT) & (t - bt > K_EPS) & (t + bt < dd) & ~skipped
                out = (cls == MISS) | (t + bt <= K_EPS) | (t - bt >= dd) | skipped
            ambiguous = ~crossed & ~out
            opaque = (kind[sl] == OPAQUE)[None, :]
            must[r0:r1] |= (crossed & opaque).any(axis=1)
            may[r0:r1] |= (ambiguous & opaque).any(axis=1)
            fc = crossed & ~opaque
            take = fc.any(axis=1) & (k_certain[r0:r1] == 0)
            one[r0:r1][take] = factor[sl][fc.argmax(axis=1)[take]]
            k_certain[r0:r1] += fc.sum(axis=1)
            for ch in range(3):
                product[r0:r1, ch] *= np.where(fc, factor[sl, ch][None, :].astype(np.longdouble), np.longdouble(1.0)).prod(axis=1)
            num_amb[r0:r1] += ambiguous.sum(axis=1)
            for (r, j) in zip(*np.nonzero(ambiguous & ~opaque)):
                if len(amb[r0 + r]) <= MAX_AMBIGUOUS:
                    amb[r0 + r].append(factor[first + j])
    return VisibilitySolution(finite, must, may, product, k_certain, amb, num_amb, one)


# ---- light queries: which lights the reservoir of light_query (dev_trace.h) may count, and which one it may pick ----
# The light triangles are world-space (light_bvh_tris, no instance map): the ray enters _intersect as it is. A light that is neither `self` nor fully
# transparent and uncoloured is certainly hit (class HIT, t - bt > eps), certainly not (class MISS or t + bt <= eps) or ambiguous. The opaque ones bracket
# t*, the distance of the nearest opaque light: t* <= hi = min (t + bt) over the certainly hit opaque lights, t* >= lo = min (t - bt) over the possibly hit
# ones. A transparent light is certainly a candidate (t <= t*) where it is certainly hit with t + bt < lo, possibly one where it is possibly hit with
# t - bt <= hi. An opaque light is a candidate only as THE nearest opaque one: possibly where t - bt <= hi, certainly where it is certainly hit and no
# other opaque light is possibly that near. NOT covered: uv-dependent textured alpha, the particle tree.
LIGHT_INVALID = 0xFFFFFFFF


def squares32(key, counter):
    """dev_sampler.h squares32 on uint32 arrays."""
    key, counter = np.uint64(key), np.asarray(counter, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)

    def swap(a):
        return ((a >> np.uint64(16)) | (a << np.uint64(16))) & m
    x = (counter * key) & m
    y = x
    z = (y + key) & m
    x = swap((x * x + y) & m)
    x = swap((x * x + z) & m)
    x = swap((x * x + y) & m)
    x = (x * x + z) & m
    t = x
    x = swap(x)
    return (t ^ ((x * x + y) & m)).astype(np.uint32)


def light_pick(ids, random_bits):
    """The light the reservoir keeps among `ids`: the minimum of squares32(0xfcbd6e15, 0x9E3779B9 * id + bits(random)), ties to the lower id."""
    ids = np.sort(np.asarray(ids, dtype=np.uint64))
    keys = squares32(0xfcbd6e15, (np.uint64(0x9E3779B9) * ids + np.uint64(random_bits)) & np.uint64(0xFFFFFFFF))
    return int(ids[np.argmin(keys)])  # argmin returns the first minimum: the lower id


class LightSolution:
    def __init__(self, finite, certain, possible, randoms):
        self.finite, self.certain, self.possible = finite, certain, possible  # [R, L] bool
        self.random_bits = np.ascontiguousarray(randoms, dtype=np.float32).view(np.uint32)
        self.decisive = (certain == possible).all(axis=1)

    def expected(self):
        """(id, num_hits) of every decisive ray; meaningless elsewhere."""
        n = len(self.finite)
        ids, hits = np.full(n, LIGHT_INVALID, dtype=np.uint32), self.certain.sum(axis=1).astype(np.uint32)
        for i in np.nonzero(hits)[0]:
            ids[i] = light_pick(np.nonzero(self.certain[i])[0], self.random_bits[i])
        return ids, hits

    def check(self, ids, hits):
        """num_hits must lie in [|certain|, |possible|]; the id must be a possible candidate, or invalid only where no candidate is certain. On decisive rays
        both are determined: the hash pick is restated here."""
        ids, hits = np.asarray(ids, dtype=np.uint32), np.asarray(hits, dtype=np.uint32)
        n = len(ids)
        ok = np.zeros(n, dtype=bool)
        reason = np.full(n, None, dtype=object)
        lo, hi = self.certain.sum(axis=1), self.possible.sum(axis=1)
        want_ids, _ = self.expected()
        for i in range(n):
            if not (lo[i] <= hits[i] <= hi[i]):
                reason[i] = "num_hits %d outside [%d, %d]" % (hits[i], lo[i], hi[i])
            elif ids[i] == LIGHT_INVALID:
                if lo[i] > 0 or hits[i] > 0:
                    reason[i] = "no light picked although %d are counted (%d certain)" % (hits[i], lo[i])
                else:
                    ok[i] = True
            elif ids[i] >= self.possible.shape[1] or not self.possible[i, ids[i]]:
                reason[i] = "light %d is no possible candidate" % ids[i]
            elif hits[i] == 0:
                reason[i] = "light %d picked from none" % ids[i]
            elif self.decisive[i] and ids[i] != want_ids[i]:
                reason[i] = "light %d picked, the hash picks %d of %s" % (ids[i], want_ids[i], list(np.nonzero(self.certain[i])[0]))
            else:
                ok[i] = True
        return ok, reason


def solve_lights(view, origins, dirs, self_handles, randoms):
    import oracle_lib
    a = oracle_lib.view_arrays(view)
    kind_tri, _ = surface_factors(view)
    handles = a["light_tri_handles"].reshape(-1, 2).astype(np.int64)
    v = _f32(a["light_bvh_tris"]).reshape(-1, 3, 4)[:, :, 0:3]
    p0 = v[:, 0, :].astype(np.float64)[None]
    e1, e2 = (v[:, 1, :] - v[:, 0, :]).astype(np.float64)[None], (v[:, 2, :] - v[:, 0, :]).astype(np.float64)[None]
    mesh = np.asarray(a["instance_mesh_ids"], dtype=np.int64)[handles[:, 0]]
    kind = kind_tri[np.asarray(a["mesh_tri_offset"], dtype=np.int64)[mesh] + handles[:, 1]]
    o32, d32 = np.ascontiguousarray(origins, dtype=np.float32), np.ascontiguousarray(dirs, dtype=np.float32)
    finite = np.isfinite(o32).all(axis=1) & np.isfinite(d32).all(axis=1)
    o = np.where(finite[:, None], o32, 0.0).astype(np.float64)
    d = np.where(finite[:, None], d32, 1.0).astype(np.float64)
    oo, od = [_exact(o[:, k:k + 1]) for k in range(3)], [_exact(d[:, k:k + 1]) for k in range(3)]
    cls, t, bt = _intersect(oo, od, p0, e1, e2)
    sh = np.ascontiguousarray(self_handles, dtype=np.uint32).astype(np.int64)
    skipped = ((sh[:, 0:1] == handles[None, :, 0]) & (sh[:, 1:2] == handles[None, :, 1])) | (kind == ABSENT)[None, :] | ~finite[:, None]
    with np.errstate(invalid="ignore"):
        hit = (cls == HIT) & (t - bt > K_EPS) & ~skipped
        maybe = ~((cls == MISS) | (t + bt <= K_EPS) | skipped)
        opaque = (kind == OPAQUE)[None, :]
        hi = np.where(hit & opaque, t + bt, np.inf).min(axis=1, keepdims=True)
        lo = np.where(maybe & opaque, t - bt, np.inf).min(axis=1, keepdims=True)
        near_opaque = maybe & opaque & (t - bt <= hi)   # the opaque lights that may be the nearest one
        only = near_opaque.sum(axis=1, keepdims=True) == 1
        certain = np.where(opaque, near_opaque & hit & only, hit & (t + bt < lo))
        possible = np.where(opaque, near_opaque, maybe & (t - bt <= hi))
    return LightSolution(finite, certain, possible, randoms)
