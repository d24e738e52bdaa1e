"""A float64 truth for the sampled-light half of next-event estimation (csrc/device/dev_light.h sample_light), and an acceptor for what a binary32 implementation
of it may answer. Test infrastructure only; plain numpy, nothing here is taken from what a device or the oracle returned.

The scene is read as the device sees it (oracle_lib.view_arrays): the light tree's root header and child blocks and its nodes, dequantised in float64 (mean = byte * 2^e
+ base, sigma = byte * 2^e_sigma, power = the integer: exact in binary32 and so the same numbers), the lights' float32 vertices through their instance transform (the
families use an identity instance, which is asserted), the material words of the emitters. The per-light table the device derives at upload (light_tri_table) is NOT
read: a table kernel that wrote a wrong line shows as a wrong stage.

Error bounds are ray_truth.py's (value, bound) arithmetic: every + - * rounds to 2^-24 relative, a hardware reciprocal, square root or reciprocal square root to one ulp
(U_RSQ = 2^-23, as U_RCP); the fast flavour's 1 / x = rsq(x)^2 (tree_importance_pair) is charged two of them and the product's rounding. A vertex normal is normalised
on the device from the caller's float32 vector: the truth normalises in float64 and gives each component 6 * 2^-24 of itself (three roundings of the squared length,
halved by the root; the root or rsq; the reciprocal or division; the product).

The resampling scans (root pass over <= 128 children with eight lanes, Reservoir::add in the descent and over the eight candidates). Reference form, per child with
importance w, running sum W, p = w / W and lane random r:
    accept = r < p;   r' = accept ? r / p : (r - p) / (1 - p)
With absolute bounds er on r and ep on p (ep = (ew + p eW) / (W - eW) + 2^-22 p: the quotient's inputs and a division that may be a reciprocal and a product):
    accepted:  er' = (er + ep) / (p - ep) + 4u          (d(r / p) = er / p + r ep / p^2 <= (er + ep) / p; the reciprocal's and the product's roundings, r' < 1)
    rejected:  er' = (er + 2 ep + 2u) / (1 - p - ep - u) + 2u
and a decision is DECIDED when |r - p| > er + ep + (1 - r) eW / W + 4u. A lane is decisive when every decision of its scan is decided; a child whose importance is not
certainly positive or certainly zero (0 < w <= ew) while it would open the scan makes the vertex's lanes undecided.

The fast flavour's threshold form (LUM_ROOT_THRESHOLD) obeys the same recurrence. It keeps t = (1 - r0) / W0 per lane, constant between two accepted children, and
accepts child c when excess = t W_c - 1 > 0. For the lane's reference random r before child c (after the rejections since the last accepted child, which telescope:
1 - r = (1 - r0) W_{c-1} / W0 = t W_{c-1}):  t W_c - 1 = (1 - r) W_c / W_{c-1} - 1 = (1 - r) / (1 - p) - 1 = (p - r) / (1 - p), so excess = (p - r) / (1 - p): the
same decision, and a relative error dt of t moves it like an absolute error (1 - r) dt of r. A rejection leaves t alone and 1 - r' = (1 - r) / (1 - p): the equivalent
error grows by 1 / (1 - p) as above (without the rounding the reference form adds). An accepted child makes t' = excess * W_{c-1} / (w_c W_c), whose relative error is
that of excess, (dt + dW)(1 + excess) / excess = (dt + dW)(1 - r) / (p - r), plus the step's (that of p, and three roundings); with 1 - r' = (p - r) / p the equivalent
error is (1 - r') dt' = ((1 - r) dt + (1 - r) dW) / p + (1 - r') (ep / p + 3u) <= (er + ep) / (p - ep) + 4u once the running sum's error (1 - r) eW / W is part of
the decision's margin, as it is above. So one recurrence bounds both forms, and the 7-bit key (LUM_ROOT_KEY) changes no decision: it only drops the picked
importance's seven lowest mantissa bits before the probability is quantised (2^-16 of it at most).
"""
import numpy as np

import ray_truth
from ray_truth import U, U_RCP, _add, _dot, _exact, _mul, _sub

U_RSQ = 2.0 ** -23      # v_rsq_f32 / v_sqrt_f32: one ulp
LANES = 8
INVALID = 0xFFFFFFFF
HI = float(np.frombuffer(np.uint32(0x3F7FFFFF).tobytes(), np.float32)[0])
NO_PICK, SELF, REFUSED, MISSED, EVALUATED = 0, 1, 2, 3, 4
# oracle/o_rng.h random targets
RT_RAY, RT_RESAMPLING, RT_PREPASS, RT_POSTPASS = 367, 384, 387, 404
TRANSLUCENT = 1
HEAD, LANE_WORDS, WORDS = 18, 17, 154


def _bfloat(h):
    return (np.asarray(h, dtype=np.uint32) << 16).view(np.float32).astype(np.float64)


def _s8(b):
    return np.asarray(b, dtype=np.uint8).view(np.int8).astype(np.float64)


class LightScene:
    def __init__(self, arrays):
        root = np.asarray(arrays["light_tree_root"], dtype=np.uint8)
        h16 = root[:10].copy().view(np.uint16)
        self.num_root_lights = int(h16[3])
        self.norm = float(_bfloat(h16[4:5])[0])
        sections = int(root[10])
        self.num_children = 8 * sections
        ex = np.exp2(_s8(root[12:16]))
        base = _bfloat(h16[0:3])
        sec = root[16:16 + 48 * sections].reshape(sections, 48)
        self.mean = np.stack([sec[:, 8 * k:8 * k + 8].reshape(-1).astype(np.float64) * ex[k] + base[k] for k in range(3)], axis=1)
        self.sd = sec[:, 24:32].reshape(-1).astype(np.float64) * ex[3]
        self.power = np.ascontiguousarray(sec[:, 32:48]).view(np.uint16).reshape(-1).astype(np.float64)
        nodes = np.asarray(arrays["light_tree_nodes"], dtype=np.uint8).reshape(-1, 64)
        self.num_nodes = len(nodes)
        if len(nodes):
            nb = _bfloat(np.ascontiguousarray(nodes[:, 0:6]).view(np.uint16).reshape(-1, 3))
            ne = np.exp2(_s8(nodes[:, 8:12]).reshape(-1, 4))
            self.node_mean = np.stack([nodes[:, 24 + 8 * k:32 + 8 * k].astype(np.float64) * ne[:, k:k + 1] + nb[:, k:k + 1] for k in range(3)], axis=2)  # [M, 8, 3]
            self.node_sd = nodes[:, 48:56].astype(np.float64) * ne[:, 3:4]
            self.node_power = nodes[:, 56:64].astype(np.float64)
            self.node_num_lights = nodes[:, 12].astype(np.int64)
            ptr = np.ascontiguousarray(nodes[:, 16:24]).view(np.uint32).reshape(-1, 2).astype(np.int64)
            self.node_child_ptr, self.node_light_ptr = ptr[:, 0], ptr[:, 1]
        # the lights
        off = np.asarray(arrays["mesh_tri_offset"], dtype=np.int64)
        handles = np.asarray(arrays["light_tri_handles"], dtype=np.uint32).reshape(-1, 2)
        self.handles = handles
        self.num_lights = len(handles)
        tf = np.asarray(arrays["instance_transforms"], dtype=np.uint32).reshape(-1, 8)
        for i in np.unique(handles[:, 0]):
            rows, tr = ray_truth._inverse_rows(tf[i])
            assert np.array_equal(rows, np.eye(3, dtype=np.float32)) and not tr.any(), "the truth reads lights of identity instances only"
        mesh = np.asarray(arrays["instance_mesh_ids"], dtype=np.int64)[handles[:, 0]]
        scene_tri = off[mesh] + handles[:, 1]
        v = ray_truth._f32(arrays["vertices"]).reshape(-1, 3, 4)[scene_tri][:, :, 0:3]
        self.p0 = v[:, 0].astype(np.float64)
        self.e1 = (v[:, 1] - v[:, 0]).astype(np.float64)  # float32 subtraction, as load_tri_light forms the edges
        self.e2 = (v[:, 2] - v[:, 0]).astype(np.float64)
        self.area = 0.5 * np.linalg.norm(np.cross(self.e1, self.e2), axis=1)
        mid = np.asarray(arrays["tri_tex"], dtype=np.uint32).reshape(-1, 4)[scene_tri, 3] & 0xFFFF
        mat = np.asarray(arrays["materials"], dtype=np.uint16).reshape(-1, 16)[mid]
        self.bidirectional = (mat[:, 0] & 0x80) != 0
        scale = (mat[:, 11].astype(np.uint32) << 15).view(np.float32).astype(np.float64)
        self.color = mat[:, 8:11].astype(np.float64) / 65535.0 * scale[:, None] * (mat[:, 7].astype(np.float64) / 65535.0)[:, None]
        assert (mat[:, 12] == 0xFFFF).all() and (mat[:, 13] == 0xFFFF).all(), "untextured emitters only"


def scene_of_view(view):
    import oracle_lib
    return LightScene(oracle_lib.view_arrays(view))


def _recip(x, units):
    with np.errstate(all="ignore"):
        v = 1.0 / x[0]
        room = np.abs(x[0]) - x[1]
        prop = np.where(room > 0, x[1] / (np.abs(x[0]) * room), np.inf)
        return v, prop + units * (np.abs(v) + prop)


def importance(pos, nrm, translucent, mean, sd, power):
    """tree_importance in float64 with its bound. pos, nrm [..., 3] (nrm normalised in float64), translucent [...], mean [..., 3], sd, power [...]: broadcast."""
    with np.errstate(all="ignore"):
        po = [_sub(_exact(mean[..., k]), _exact(pos[..., k])) for k in range(3)]
        dist_sq = _dot(po, po)
        var = _mul(_exact(sd), _exact(sd))
        den = _add(dist_sq, var)
        inv = _recip(den, 2.0 * U_RSQ + U)
        r = _mul(_exact(power), inv)
        t = _mul(var, inv)
        n = [(nrm[..., k], 6.0 * U * np.abs(nrm[..., k])) for k in range(3)]
        d = _dot(po, n)
        room = den[0] - den[1]
        rs_v = den[0] ** -0.5
        rs = (rs_v, np.where(room > 0, 0.5 * rs_v * den[1] / room, np.inf) + 2.0 * U_RSQ * rs_v)
        ndl = _mul(d, rs)
        certain = (ndl[0] + ndl[1] <= 0.0) | (ndl[0] - ndl[1] >= 1.0)
        ndotl = (np.clip(ndl[0], 0.0, 1.0), np.where(certain, 0.0, ndl[1]))
        val = _mul(r, _add(_mul(ndotl, _sub(_exact(np.ones_like(t[0])), t)), t))
        w = np.where(translucent, r[0], np.maximum(val[0], 0.0))
        e = np.where(translucent, r[1], val[1])
        # no power; the vertex on a mean without variance (power * inf * (0 * inf) is a NaN, which the maximum drops); a squared distance beyond binary32 (its
        # reciprocal is 0; within a few per cent of FLT_MAX either may happen)
        dead = (power == 0) | ((den[0] == 0) & ~translucent) | (den[0] > 3.5e38)
        e = np.where((den[0] > 3.3e38) & (den[0] <= 3.5e38), np.inf, e)
        w, e = np.where(dead, 0.0, w), np.where(dead, 0.0, e)
        e = np.where(np.isfinite(e), e, np.inf)
    return np.broadcast_arrays(w, e)


def scan(ws, es, r, er=None):
    """The resampling recurrence of the module docstring. ws, es [K, N]: the candidates' weights and bounds in scan order; r [N, L]: the lanes' random numbers.
    Returns pick [N, L] (-1: none), decisive [N, L], the running sum and its bound [N], and the lanes' random numbers and bounds after the scan."""
    K, N = ws.shape
    L = r.shape[1]
    r = r.astype(np.float64).copy()
    er = np.zeros((N, L)) if er is None else er.copy()
    T, eT = np.zeros(N), np.zeros(N)
    pick = np.full((N, L), -1, dtype=np.int64)
    dec = np.ones((N, L), dtype=bool)
    with np.errstate(all="ignore"):
        for c in range(K):
            w, e = ws[c], es[c]
            live = (w > 0) | (e > 0)
            if not live.any():
                continue
            first = (T == 0) & (eT == 0)
            unsure = live & (w <= e)
            Tn = T + w
            eTn = np.where(first, e, eT + e + U * (Tn + eT + e))
            p = np.where(Tn > 0, w / np.where(Tn > 0, Tn, 1.0), 0.0)
            ep = np.where(first & ~unsure, 0.0, (e + p * eTn) / np.maximum(Tn - eTn, 1e-300) + 2.0 * U_RCP * p)
            dec &= ~(first & unsure)[:, None]
            pc, epc = p[:, None], ep[:, None]
            margin = er + epc + (1.0 - r) * np.where(first, 0.0, eTn / np.where(Tn > 0, Tn, 1.0))[:, None] + 4.0 * U
            acc = r < pc
            decided = np.abs(r - pc) > margin
            dec &= decided | ~live[:, None]
            den_a, den_r = pc - epc, 1.0 - pc - epc - U
            ra, era = r / pc, (er + epc) / den_a + 4.0 * U
            rr, err = (r - pc) / (1.0 - pc), (er + 2.0 * epc + 2.0 * U) / den_r + 2.0 * U
            nr = np.clip(np.where(acc, ra, rr), 0.0, HI)
            ner = np.where(np.where(acc, den_a, den_r) > 0, np.where(acc, era, err), np.inf)
            lv = live[:, None]
            r, er = np.where(lv, nr, r), np.where(lv, ner, er)
            pick = np.where(lv & acc, c, pick)
            T, eT = np.where(live, Tn, T), np.where(live, eTn, eT)
    return pick, dec, T, eT, r, er


def probability_of(ws, es, T, eT, k):
    """p = w_k / T and its bound for the chosen candidates k [N, L] (k < 0: 0)."""
    N = ws.shape[1]
    kk = np.maximum(k, 0)
    w, e = ws[kk, np.arange(N)[:, None]], es[kk, np.arange(N)[:, None]]
    with np.errstate(all="ignore"):
        p = np.where((k >= 0) & (T[:, None] > 0), w / T[:, None], 0.0)
        ep = (e + p * eT[:, None]) / np.maximum(T[:, None] - eT[:, None], 1e-300) + 2.0 * U_RCP * p
    return p, np.where(k >= 0, ep, 0.0), w, e


class Vertices:
    """The caller-made vertices of a family: float32 position, normal and V (any length), a material, a self handle and a pixel each."""

    def __init__(self, position, normal, V, albedo, opacity, roughness, ior, flags, self_handles, pixels):
        f = lambda a, k: np.ascontiguousarray(a, dtype=np.float32).reshape(-1, k)
        self.position, self.normal, self.V, self.albedo = f(position, 3), f(normal, 3), f(V, 3), f(albedo, 3)
        n = len(self.position)
        self.opacity, self.roughness, self.ior = [np.ascontiguousarray(a, dtype=np.float32).reshape(n) for a in (opacity, roughness, ior)]
        self.flags = np.ascontiguousarray(flags, dtype=np.uint32).reshape(n)
        self.self_handles = np.ascontiguousarray(self_handles, dtype=np.uint32).reshape(n, 2)
        self.pixels = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(n, 2)

    def __len__(self):
        return len(self.position)

    def words(self):
        w = np.zeros((len(self), 20), dtype=np.uint32)
        w[:, 0:3], w[:, 3:6], w[:, 6:9], w[:, 9:12] = self.position.view(np.uint32), self.normal.view(np.uint32), self.V.view(np.uint32), self.albedo.view(np.uint32)
        w[:, 12], w[:, 13], w[:, 14] = self.opacity.view(np.uint32), self.roughness.view(np.uint32), self.ior.view(np.uint32)
        w[:, 15], w[:, 16:18], w[:, 18:20] = self.flags, self.self_handles, self.pixels
        return w

    def material_words(self):
        """roughness and ior as MatParams::set quantises them (dev_bsdf.h): the numbers every later stage reads"""
        sat = lambda a: np.clip(a.astype(np.float32), np.float32(0), np.float32(1))
        ro = (sat(self.roughness) * np.float32(1023) + np.float32(0.5)).astype(np.uint32)
        io = (sat(self.ior * np.float32(1.0 / 3.0)) * np.float32(255) + np.float32(0.5)).astype(np.uint32)
        return ro.astype(np.float64) / 1023.0, io.astype(np.float64) / 255.0 * 3.0


def randoms(vertices, first_sample, samples):
    """The sampler's numbers of every (vertex, sample id): prepass [V, S, 8], postpass [V, S, 8], ray pairs [V, S, 8, 2], outer resampling [V, S] (float32, through
    oracle_random_2d_table: the sampler is integer arithmetic, restated by the oracle and pinned by tests/test_oracle_known_answers.py and tests/test_sobol_table.py)."""
    import oracle_lib
    targets = [RT_PREPASS + l for l in range(LANES)] + [RT_POSTPASS + l for l in range(LANES)] + [RT_RAY + l for l in range(LANES)] + [RT_RESAMPLING]
    t = np.stack([oracle_lib.random_2d_table(int(px), int(py), first_sample, samples, targets) for px, py in vertices.pixels])
    return t[:, :, 0:8, 0], t[:, :, 8:16, 0], t[:, :, 16:24, :], t[:, :, 24, 0]


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def peters(origin, p0, e1, e2, bidirectional, rnd):
    """sample_tri_solid_angle in float64: signed G0, solid angle, direction (Peters 2021). All arrays broadcast over the leading axes."""
    with np.errstate(all="ignore"):
        a, b, c = _unit(p0 - origin), _unit((p0 + e1) - origin), _unit((p0 + e2) - origin)
        g0s = np.sum(np.cross(a, b) * c, axis=-1)
        g0 = np.abs(g0s)
        g1 = np.sum(a * c, axis=-1) + np.sum(b * c, axis=-1)
        g2 = 1.0 + np.sum(a * b, axis=-1)
        sa = 2.0 * np.arctan2(g0, g1 + g2)
        half = 0.5 * rnd[..., 0] * sa
        sh, ch = np.sin(half), np.cos(half)
        r = a * (g0 * ch - g1 * sh)[..., None] + c * (g2 * sh)[..., None]
        ct = r * (2.0 * np.sum(a * r, axis=-1) / np.sum(r * r, axis=-1))[..., None] - a
        s2 = np.sum(b * ct, axis=-1)
        sv = (1.0 - rnd[..., 1]) + rnd[..., 1] * s2
        tt = np.sqrt(np.maximum((1.0 - sv * sv) / (1.0 - s2 * s2), 0.0))
        ray = _unit(b * (sv - tt * s2)[..., None] + ct * tt[..., None])
    return g0s, sa, ray


def intersect(origin, ray, p0, e1, e2):
    """Moeller-Trumbore in float64: t, u, v."""
    with np.errstate(all="ignore"):
        h = np.cross(ray, e2)
        a = np.sum(e1 * h, axis=-1)
        s = origin - p0
        u = np.sum(s * h, axis=-1) / a
        q = np.cross(s, e1)
        v = np.sum(ray * q, axis=-1) / a
        t = np.sum(e2 * q, axis=-1) / a
    return t, u, v


def direction_probability(nrm, V, L, roughness, ior, translucent):
    """light_direction_probability in float64 (analyze_direction, pdf_vndf_bounded, pdf_refraction, the roulette): the products N.V, N.H, H.V, H.L do not depend on the
    frame they are taken in, so the shading frame is not built."""
    with np.errstate(all="ignore"):
        ndl_s = np.sum(nrm * L, axis=-1)
        vz = np.sum(nrm * V, axis=-1)
        ndv = np.clip(vz, 0.0, 1.0)
        refr = ndl_s < 0.0
        hv = L + V * np.where(refr, ior, 1.0)[..., None]
        ln = np.linalg.norm(hv, axis=-1)
        H = np.where((ln > 0)[..., None], hv / ln[..., None], V)
        hdv, hdl = np.abs(np.sum(H * V, axis=-1)), np.abs(np.sum(H * L, axis=-1))
        ndh = np.abs(np.sum(nrm * H, axis=-1))
        sr = roughness + 0.04 * (1.0 - roughness)
        rr = np.clip((roughness - 0.5) / (0.1 - 0.5), 0.0, 1.0)
        r4 = sr ** 4
        n2 = np.minimum(ndh * ndh, 1.0)
        D = r4 / (np.pi * (1.0 - n2 + r4 * n2) ** 2)
        # bounded VNDF
        vxy2 = np.maximum(1.0 - vz * vz, 0.0)
        t = np.sqrt(r4 * vxy2 + vz * vz)
        s2 = (1.0 + np.sqrt(vxy2)) ** 2
        k = (1.0 - r4) * s2 / (s2 + r4 * vz * vz)
        pdf_refl = D / (2.0 * (k * ndv + t))
        m2 = np.maximum(0.0001, ndv * ndv)
        g1 = 2.0 / (np.sqrt((r4 * (1.0 - m2) + m2) / m2) + 1.0)
        den = (ior * hdv + hdl) ** 2
        pdf_refr = D * g1 * (hdv / ndv) * (hdl / den)
        refr_prob = np.where(translucent, 0.5, 0.0)
        prob = np.where(refr, refr_prob * pdf_refr, (1.0 - refr_prob) * pdf_refl)
    return prob * rr, refr


def mis_weight(dir_prob, sa, power, dist, root_sum):
    """1 - mis_base (mis_for_light_sample)"""
    with np.errstate(all="ignore"):
        dl = 8.0 * (1.0 / sa) * (power / (dist * dist)) * (1.0 / root_sum)
        return 1.0 - np.where(dl > 0.0, dir_prob / (dir_prob + dl), 1.0)


def _f(words):
    return np.ascontiguousarray(words, dtype=np.uint32).view(np.float32).astype(np.float64)


class Truth:
    """Everything the truth knows about a family before it sees an answer: the root scan per (vertex, sample id, lane)."""

    def __init__(self, scene, vertices, first_sample, samples):
        self.scene, self.vertices, self.first_sample, self.samples = scene, vertices, first_sample, samples
        V = len(vertices)
        self.pos = vertices.position.astype(np.float64)
        self.nrm = _unit(vertices.normal.astype(np.float64))
        self.view = _unit(vertices.V.astype(np.float64))
        self.translucent = (vertices.flags & TRANSLUCENT) != 0
        self.roughness, self.ior = vertices.material_words()
        self.r_pre, self.r_post, self.r_ray, self.r_outer = randoms(vertices, first_sample, samples)
        C = scene.num_children
        w, e = importance(self.pos[:, None, :], self.nrm[:, None, :], self.translucent[:, None], scene.mean[None, :, :], scene.sd[None, :], scene.power[None, :])
        self.w, self.e = np.ascontiguousarray(w), np.ascontiguousarray(e)  # [V, C]
        N = V * samples
        vi = np.repeat(np.arange(V), samples)
        self.vi = vi
        ws, es = np.ascontiguousarray(self.w[vi].T), np.ascontiguousarray(self.e[vi].T)  # [C, N]
        self.ws, self.es = ws, es
        self.pick, self.decisive, self.T, self.eT, _, _ = scan(ws, es, self.r_pre.reshape(N, LANES))
        self.p, self.ep, _, _ = probability_of(ws, es, self.T, self.eT, self.pick)
        with np.errstate(all="ignore"):
            self.q = np.where(self.p > 0, np.maximum(np.rint(1048575.0 * self.p), 1.0), 0.0)
            self.weight = np.where(self.p > 0, 1.0 / (8.0 * self.p), 0.0)
        k = scene.norm / 65535.0
        self.root_sum = self.T * k
        self.e_root_sum = (self.eT + 2.0 * U * self.T) * k + 2.0 * U * self.root_sum  # the sum, the constant's quotient, the product

    def decisive_share(self):
        return float(self.decisive.mean())

    # ---- the acceptor ----
    def check(self, out, yardstick=None, factor=1.0, bsdf_reference=None, bsdf_tolerance=None, luts=None):
        """out [V, S, 154] uint32: the probe's words. Returns (failures: dict name -> bool [N] or [N, 8], figures: dict name -> the largest distance from the truth per
        quantity). yardstick: the figures of the reference run; the distances may be `factor` times them (floor: 4 ulp of the quantity's scale)."""
        sc = self.scene
        N = len(self.vi)
        o = np.ascontiguousarray(out, dtype=np.uint32).reshape(N, WORDS)
        fo = o.view(np.float32).astype(np.float64)
        fail, fig = {}, {}
        ar = np.arange(N)[:, None]
        # root pass: the continuation words
        cont = o[:, 9:17].astype(np.int64)
        is_light, index, q = cont & 1, (cont >> 1) & 0xFF, (cont >> 9).astype(np.float64)
        child = np.where(is_light == 1, index, index + sc.num_root_lights)
        none = q == 0
        in_range = np.where(is_light == 1, index < sc.num_root_lights, child < sc.num_children)
        childc = np.clip(child, 0, sc.num_children - 1)
        p_c, ep_c, w_c, e_c = probability_of(self.ws, self.es, self.T, self.eT, childc)
        total_possible = (self.T + self.eT > 0)[:, None]
        fail["no pick although the vertex has importance"] = none & (self.T - self.eT > 0)[:, None]
        fail["a pick although nothing has importance"] = ~none & ~total_possible
        fail["picked child outside the root"] = ~none & ~in_range
        fail["picked child without importance"] = ~none & in_range & ~((w_c > 0) | (e_c > 0))
        fail["pick differs from the truth's on a decisive lane"] = self.decisive & ~none & (child != self.pick) | (self.decisive & none & (self.pick >= 0))
        want_q = np.maximum(1048575.0 * p_c, 1.0)
        fail["probability word is not the picked child's"] = ~none & in_range & (np.abs(q - want_q) > 1.0 + 2.0 ** -15 * want_q)
        fail["root_sum (root pass) outside its bound"] = ~(np.abs(fo[:, 17] - self.root_sum) <= self.e_root_sum)  # (written so that a NaN fails)
        fail["root_sum (sample) is not the root pass's"] = o[:, 8] != o[:, 17]
        fig["root_sum relative"] = float(np.max(np.abs(fo[:, 17] - self.root_sum) / np.maximum(self.root_sum, 1e-300) * (self.root_sum > 0)))
        # descent and the lane's pick
        lane = o[:, HEAD:].reshape(N, LANES, LANE_WORDS)
        fl = fo[:, HEAD:].reshape(N, LANES, LANE_WORDS)
        light = lane[:, :, 0].astype(np.int64)
        weight = fl[:, :, 1]
        status = lane[:, :, 2]
        with np.errstate(all="ignore"):
            w_root = np.where(none, 0.0, 1.0 / (8.0 * q / 1048575.0))
        want_light = np.where(none, INVALID, np.where(is_light == 1, index, -1))
        want_weight, e_weight = w_root.copy(), 4.0 * U * w_root
        dec_descent = np.ones((N, LANES), dtype=bool)
        if sc.num_nodes:
            going = ~none & (is_light == 0) & in_range
            node = np.where(going, index, 0)
            r, er = self.r_post.reshape(N, LANES).astype(np.float64), np.zeros((N, LANES))
            for _ in range(8):
                if not going.any():
                    break
                g = np.nonzero(going)
                nd = node[g]
                v = self.vi[g[0]]
                w, e = importance(self.pos[v][:, None, :], self.nrm[v][:, None, :], self.translucent[v][:, None], sc.node_mean[nd], sc.node_sd[nd], sc.node_power[nd])
                pk, dc, T, eT, r2, er2 = scan(np.ascontiguousarray(w.T), np.ascontiguousarray(e.T), r[g][:, None], er[g][:, None])
                p, ep, _, _ = probability_of(np.ascontiguousarray(w.T), np.ascontiguousarray(e.T), T, eT, pk)
                pk, dc, p, ep = pk[:, 0], dc[:, 0], p[:, 0], ep[:, 0]
                r[g], er[g] = r2[:, 0], er2[:, 0]
                dec_descent[g] &= dc
                with np.errstate(all="ignore"):
                    step = np.where(pk >= 0, 1.0 / p, 1.0)
                    e_weight[g] = np.where(pk >= 0, e_weight[g] * step + want_weight[g] * step * (ep / np.maximum(p - ep, 1e-300) + 4.0 * U), e_weight[g])
                    want_weight[g] = want_weight[g] * step
                nl = sc.node_num_lights[nd]
                leaf = (pk >= 0) & (pk < nl)
                want_light[g] = np.where(pk < 0, INVALID, np.where(leaf, sc.node_light_ptr[nd] + pk, -1))
                node[g] = np.where((pk >= 0) & ~leaf, sc.node_child_ptr[nd] + (pk - nl), 0)
                going[g] = (pk >= 0) & ~leaf
        sure = dec_descent & (want_light >= 0)
        fail["lane's light is not the tree's"] = sure & (light != want_light)
        has = light != INVALID
        fail["lane's light outside the scene"] = has & (light >= sc.num_lights)
        fail["lane's weight outside its bound"] = sure & has & (light == want_light) & ~(np.abs(weight - want_weight) <= e_weight + 4.0 * U * want_weight)
        fig["lane weight relative"] = float(np.max(np.where(sure & has & (light == want_light), np.abs(weight - want_weight) / np.maximum(want_weight, 1e-300), 0.0)))
        # the candidate
        lc = np.clip(light, 0, sc.num_lights - 1)
        vi = self.vi[:, None]
        is_self = has & (sc.handles[lc, 0] == self.vertices.self_handles[vi, 0]) & (sc.handles[lc, 1] == self.vertices.self_handles[vi, 1])
        fail["status of a lane without a light"] = ~has & (status != NO_PICK)
        fail["self not skipped"] = is_self & (status != SELF)
        fail["skipped as self although it is not"] = has & ~is_self & (status == SELF)
        fail["no status"] = has & ((status == NO_PICK) | (status > EVALUATED))
        cand = has & ~is_self
        pos = self.pos[vi]
        g0s, sa, ray = peters(pos, sc.p0[lc], sc.e1[lc], sc.e2[lc], sc.bidirectional[lc], self.r_ray.reshape(N, LANES, 2).astype(np.float64))
        m_g0 = 64.0 * U  # three unit vectors of 6 u per component, a cross and a dot product of them: the triple product to well inside 64 u
        with np.errstate(all="ignore"):
            sa_rel = m_g0 / np.abs(g0s) + 2.0 ** -20
        back = ~sc.bidirectional[lc] & (g0s > m_g0)
        front = sc.bidirectional[lc] | (g0s < -m_g0)
        with np.errstate(all="ignore"):
            small = front & (sa * (1.0 + sa_rel) < 1e-7)
            large = front & (sa * (1.0 - sa_rel) > 1e-7) & (np.abs(g0s) > m_g0)
        fail["back-facing one-sided light not refused"] = cand & back & (status != REFUSED)
        fail["solid angle below 1e-7 not refused"] = cand & small & (status != REFUSED)
        fail["refused although front-facing and large enough"] = cand & large & (status == REFUSED)
        sampled = cand & (status >= MISSED)
        d_ray = fl[:, :, 3:6]
        t, u, v = intersect(pos, d_ray, sc.p0[lc], sc.e1[lc], sc.e2[lc])
        inside = (u > 1e-4) & (v > 1e-4) & (u + v < 1.0 - 1e-4) & (t > 0)
        fail["missed although the ray crosses the light well inside"] = sampled & inside & (status == MISSED)
        ev = cand & (status == EVALUATED)
        # a word that is no number is a failure of its own, never a reason to leave a comparison out: every comparison below is written so that a NaN fails it,
        # and only the TRUTH's own value being no number (a degenerate triangle seen edge-on, say) excuses a lane from a comparison
        fail["non-finite word of an evaluated lane"] = ev & ~np.isfinite(fl[:, :, 3:17]).all(axis=-1)
        fail["non-finite ray or solid angle of a sampled lane"] = sampled & ~np.isfinite(fl[:, :, 3:7]).all(axis=-1)
        fail["non-finite weight of a lane with a light"] = has & ~np.isfinite(weight)
        fail["non-finite word of the sample or the root pass"] = ~np.isfinite(fo[:, 1:9]).all(axis=-1) | ~np.isfinite(fo[:, 17])
        clear = ev & large  # the quantities are compared where the truth's own evaluation is well conditioned
        dist = fl[:, :, 7]
        col = fl[:, :, 8:11]
        bw = fl[:, :, 11:14]
        dirp, mis, target = fl[:, :, 14], fl[:, :, 15], fl[:, :, 16]
        v_nrm, v_view = self.nrm[vi], self.view[vi]
        want_dirp, _ = direction_probability(v_nrm, v_view, d_ray, self.roughness[vi], self.ior[vi], self.translucent[vi])
        imp = np.max(col, axis=-1)
        want_mis = mis_weight(dirp, fl[:, :, 6], imp * sc.area[lc], dist, fo[:, 17][:, None])
        with np.errstate(all="ignore"):
            want_target = np.max(col * bw * mis[..., None], axis=-1)
        # want_mis is formed from the lane's own stages: it is a number wherever they are (a stage that is not has failed above); t from the lane's own ray likewise
        words_ok = np.isfinite(fl[:, :, 3:17]).all(axis=-1)
        with np.errstate(all="ignore"):
            dist_fig = {  # name: (distance from the truth, where the truth's own value is a number)
                "ray direction": (np.max(np.abs(d_ray - ray), axis=-1), np.isfinite(ray).all(axis=-1)),
                "ray length": (np.abs(np.linalg.norm(d_ray, axis=-1) - 1.0), np.ones((N, LANES), dtype=bool)),
                "solid angle relative": (np.abs(fl[:, :, 6] - sa) / sa, np.isfinite(sa) & (sa > 0)),
                "dist relative": (np.abs(dist - t) / np.abs(t), (np.isfinite(t) & (t != 0)) | ~words_ok),
                "direction probability relative": (np.abs(dirp - want_dirp) / np.maximum(want_dirp, 1e-30), np.isfinite(want_dirp) | ~words_ok),
                "MIS weight": (np.abs(mis - want_mis), np.isfinite(want_mis) | ~words_ok),
            }
        for name, (dval, truth_ok) in dist_fig.items():
            sel = clear & truth_ok
            fig[name] = float(np.max(np.where(sel & np.isfinite(dval), dval, 0.0))) if sel.any() else 0.0
            if yardstick is not None:
                fail[name + " beyond %g x the yardstick" % factor] = sel & ~(dval <= max(factor * yardstick[name], 4.0 * 2.0 ** -23))
        fail["ray does not reach the light's plane inside the light"] = ev & ~((u > -1e-3) & (v > -1e-3) & (u + v < 1.0 + 1e-3) & (t > 0))
        fail["emitted colour is not the material's"] = ev & ~(np.abs(col - sc.color[lc]) <= 4.0 * U * sc.color[lc]).all(axis=-1)
        fail["reservoir target is not colour x BSDF x MIS"] = ev & ~(np.abs(target - want_target) <= 8.0 * U * np.abs(want_target) + 2.0 ** -126)
        if bsdf_reference is not None:
            with np.errstate(all="ignore"):
                rel = np.max(np.abs(bw - bsdf_reference) / np.maximum(np.abs(bsdf_reference), 1e-6), axis=-1)
            fig["BSDF weight relative to the oracle"] = float(np.max(np.where(ev & np.isfinite(rel), rel, 0.0)))
            if bsdf_tolerance is not None:
                fail["BSDF weight beyond its tolerance"] = ev & ~(rel <= bsdf_tolerance)
        if luts is not None:
            # ... and to the float64 evaluation (bsdf_truth.py: eval_bsdf under the general hint) on the lane's own direction, away from the horizon
            import bsdf_truth
            lanes_of = np.repeat(self.vi, LANES)
            want_bw, clear_of_horizon = bsdf_truth.evaluate_direction(luts, bsdf_truth.Material(self.vertices, lanes_of), self.nrm[lanes_of], self.view[lanes_of],
                                                                      d_ray.reshape(-1, 3))
            want_bw, clear_of_horizon = want_bw.reshape(N, LANES, 3), clear_of_horizon.reshape(N, LANES) & np.isfinite(want_bw).all(axis=-1).reshape(N, LANES)
            with np.errstate(all="ignore"):
                rel64 = np.max(np.abs(bw - want_bw) / np.maximum(np.abs(want_bw), 1e-6), axis=-1)
            held = ev & clear_of_horizon
            fig["BSDF weight relative to the float64 evaluation"] = float(np.max(np.where(held & np.isfinite(rel64), rel64, 0.0)))
            if bsdf_tolerance is not None:
                fail["BSDF weight beyond its tolerance of the float64 evaluation"] = held & ~(rel64 <= bsdf_tolerance)
        # the outer reservoir and the sample
        with np.errstate(all="ignore"):
            wgt = np.where(ev, target * weight * fl[:, :, 6], 0.0)
        ws, es = np.ascontiguousarray(wgt.T), np.ascontiguousarray((3.0 * U * wgt).T)
        pk, dc, T, eT, _, _ = scan(ws, es, self.r_outer.reshape(N, 1))
        pk, dc = pk[:, 0], dc[:, 0]
        self.outer_decisive = dc
        f_light = o[:, 0].astype(np.int64)
        f_none = f_light == INVALID
        fail["a sample although no lane has a target"] = ~f_none & ~(wgt > 0).any(axis=1)
        fail["no sample although a lane has a target"] = f_none & (wgt > 0).any(axis=1)
        fail["sample is not the reservoir's lane"] = dc & (pk >= 0) & (f_light != light[np.arange(N), np.maximum(pk, 0)])
        # whichever lane the sample came from: it has to be one of them, word for word, and its colour the lane's times the reservoir's weight
        match = ev & (wgt > 0) & (light == f_light[:, None]) & (lane[:, :, 3:6] == o[:, None, 1:4]).all(axis=-1) & (lane[:, :, 7] == o[:, None, 7])
        fail["sample matches no evaluated lane"] = ~f_none & ~match.any(axis=1)
        sel_lane = np.where(dc & (pk >= 0), np.maximum(pk, 0), np.argmax(match, axis=1))
        rows = np.arange(N)
        with np.errstate(all="ignore"):
            sw = np.where(target[rows, sel_lane] > 0, T / target[rows, sel_lane], 0.0)
            want_col = (col * bw * mis[..., None])[rows, sel_lane] * sw[:, None]
        got_col = fo[:, 4:7]
        fail["sample colour is not the lane's colour x sampling_weight"] = ~f_none & match.any(axis=1) & ~(np.abs(got_col - want_col) <= 16.0 * U * np.abs(want_col) + 2.0 ** -126).all(axis=-1)
        return fail, fig
