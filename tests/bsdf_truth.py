"""A float64 truth for the bounce and the BSDF-driven light direction (csrc/device/dev_bsdf.h sample_bounce, csrc/device/dev_light.h sample_light_direction), and an
acceptor for what a binary32 implementation of them may answer through the bounce probe (include/lum_core.h lumc_bounce_probe_host). Test infrastructure only; plain
numpy, nothing here is taken from what a device or the oracle returned.

The acceptor is STAGE-WISE: a stage's word is recomputed in float64 from the words the answer itself reports for the stage before (m from the reported local V, the
terms from the reported m and ray, the pdfs and the evaluation from the reported terms, mis from the reported pdfs, w from the reported eval and mis, prob from the
reported w and weight_sum, pick from the reported pick and prob, the final weight from the reported chosen eval and weight_sum). Errors do not chain, and a decision
that the kernel takes on two words it reports (pick < prob, NdotH < 0, NdotL <= 0, rnd >= rr) is an exact comparison of those words. The decisions with a margin are
    total_reflection: the sign of b = 1 - ior^2 (1 - d^2), d = |m . V| from the reported m and V; binary32 forms d in three roundings, d^2, 1 - d^2, the product with
        ior^2 and the difference in five more: |b32 - b| <= (10 ior^2 + 2) u                                                                     (u = 2^-24)
    the face-normal test dot(face_normal, ray) * flip < kEps on the reported vectors: three roundings of a dot product of unit vectors, 8 u with room
    rotation_to_z's branch nz < -1 + kEps: the normal is normalised on the device, 6 u per component (light_truth.py), 8 u with the sum's rounding; an axis
        vector is normalised without a rounding and is always decided
    the roulette rnd >= rr of sample_light_direction: rr is one difference, one quotient by a rounded constant and a clamp, 8 u with room
    lut_axis' cell: the table's interpolant is continuous across cells, so the value is held on either side; the share of coordinates within their bound of a cell
        boundary is a figure
Besides the stage-wise walk the truth runs the whole chain on its own values (no answer involved) and calls a thread DECISIVE when every margin of that chain exceeds
its bound, the resampling decisions through light_truth.scan's recurrence with the weights' bounds taken from the conditioning below: there the chosen technique and
the flags have to be the truth's.

Conditioning. ggx_d forms a = 1 - n^2 + r^4 n^2 with n = NdotH. n^2 carries half an ulp of itself (u n^2), the sum another u a: D = r^4 / (pi a^2) lies between the
values at a -+ (u n^2 + 2 u a). At the roughness clamp (20 / 1023, r^4 = 1.5e-7) that is most of a itself. Every word that contains D (the bounded-VNDF and refraction
pdfs, eval_microfacet, eval_microfacet_over_diffuse, eval_diffuse_over_vndf, eval_refraction and what is built from them) carries the bound this interval gives it,
computed by evaluating the word at both ends. A word whose bound exceeds 1e-2 of its scale is ILL-CONDITIONED: it is held to finiteness, sign and that bound. The
D-free words (the sampled vectors, the terms, G1, G2, k, t, the hinted forms without D, the sums and quotients) are never excused. Two more conditionings are
propagated: a normalisation of a short vector (the scaled microfacet normal at grazing views and low roughness, V + ray of the diffuse draw) takes 4 u / length, and
the refracted ray and the Fresnel term near the critical angle take the root's d sqrt(b) = e_b / (2 sqrt(b)).

Continuous words are measured as distances from the stage's truth, relative to the word's scale (1 for components of unit vectors and for cosines). The largest
distance over the well-conditioned threads of a family is its FIGURE; the oracle's figures are the yardstick, and an answer may be `factor` times the yardstick away
(floor 4 ulp), or its propagated bound where that is larger. The figure is also taken in units of each thread's own bound (at least 4 ulp), and the yardstick's term
is the smaller of the two readings: one grazing thread of the reference does not widen the allowance of the threads whose own bound is small. Sums, quotients and
products of reported words are held to 4 ulp of the result.

Whatever the yardstick says, and for the reference's own answer too, a well-conditioned word lies within CEILING = 4 times its thread's bound, 16 ulp of its scale at
least. A word is one stage of the chain: the longest stages are a sampler (some 25 binary32 operations with two normalisations and a sine and cosine of 2 pi u, whose
argument alone carries 4 u) and a hinted evaluation (some 30 operations with divisions and roots), every operation within one ulp in either flavour, and the thread's
bound counts only the one ill-conditioned operation among them. Sixteen ulp is what a dozen of those roundings give when they all point the same way; a word further
off is wrong, not rounded. (The reference's answers reach 1.6 bounds in one word, the sampled normal of the light direction at the roughness clamp, and stay below 1
in all others.)

A word that is no number fails by name unless the truth's own value is none (0 / 0 of an empty reservoir: prob of a vertex seen from below).
"""
import numpy as np

import light_truth as lt
from ray_truth import U

KEPS = 2.0 ** -23
ULP4 = 4.0 * 2.0 ** -23
TINY = 1e-37
WORDS, HEAD, TECH_WORDS, LD_WORDS = 143, 44, 24, 27
LD0 = HEAD + 3 * TECH_WORDS
NOT_TAKEN, TAKEN, TOTAL_REFLECTION = 0, 1, 2
LD_REFUSED, LD_REFLECTION, LD_REFRACTION, LD_REFRACTION_TOTAL = 0, 1, 2, 3
NO_TECHNIQUE = 3
TECH_NAMES = ("reflection", "diffuse", "refraction")
GENERAL, MICROFACET, DIFFUSE, REFRACTION = 0, 1, 2, 3
TRANSLUCENT, INSIDE, METALLIC, COLOURED = 1, 2, 4, 8
# oracle/o_rng.h, csrc/device/dev_sampler.h
RT_REFLECTION, RT_DIFFUSE, RT_REFRACTION, RT_RESAMPLING, RT_OPACITY, RT_L_CHOICE, RT_L_DIRECTION, RT_L_RR = 39, 43, 47, 51, 55, 569, 571, 575
ILL = 1e-2
CEILING = 4.0


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _sat(x):
    return np.clip(x, 0.0, 1.0)


# ---- the frame ----
def rotation_to_z(n):
    with np.errstate(all="ignore"):
        r = np.stack([n[..., 1], -n[..., 0], np.zeros_like(n[..., 0]), 1.0 + n[..., 2]], axis=-1)
        length = np.linalg.norm(r, axis=-1)
        r = r / length[..., None]
    minus = n[..., 2] < -1.0 + KEPS
    return np.where(minus[..., None], np.array([1.0, 0.0, 0.0, 0.0]), r), minus, length


def qapply(q, v):
    u, s = q[..., :3], q[..., 3]
    return u * (2.0 * _dot(u, v))[..., None] + v * (s * s - _dot(u, u))[..., None] + np.cross(u, v) * (2.0 * s)[..., None]


def qinv(q):
    return q * np.array([-1.0, -1.0, -1.0, 1.0])


# ---- sampling ----
def _vndf_cap(V, roughness, rnd, bounded):
    """sample_vndf_bounded / sample_vndf_caps: m and the length of the vector the last normalisation takes"""
    with np.errstate(all="ignore"):
        r2 = roughness * roughness
        r4 = r2 * r2
        v = _unit(np.stack([r2 * V[..., 0], r2 * V[..., 1], V[..., 2]], axis=-1))
        phi = 2.0 * np.pi * rnd[..., 0]
        if bounded:
            s = 1.0 + np.sqrt(V[..., 0] ** 2 + V[..., 1] ** 2)
            k = (1.0 - r4) * s * s / (s * s + r4 * V[..., 2] ** 2)
            b = k * v[..., 2]
        else:
            b = v[..., 2]
        z = (1.0 - rnd[..., 1]) * (1.0 + b) - b
        st = np.sqrt(_sat(1.0 - z * z))
        m = np.stack([st * np.cos(phi), st * np.sin(phi), z], axis=-1) + v
        scaled = np.stack([m[..., 0] * r2, m[..., 1] * r2, m[..., 2]], axis=-1)
        length = np.linalg.norm(scaled, axis=-1)
        return scaled / length[..., None], length


def sample_vndf_bounded(V, roughness, rnd):
    return _vndf_cap(V, roughness, rnd, True)


def sample_vndf_caps(V, roughness, rnd):
    return _vndf_cap(V, roughness, rnd, False)


def sample_ray_sphere(alpha, beta):
    with np.errstate(all="ignore"):
        a = np.sqrt(np.maximum(1.0 - alpha * alpha, 0.0))
        b = 2.0 * np.pi * beta
        ray = np.stack([a * np.cos(b), a * np.sin(b), alpha], axis=-1)
    pole = np.abs(alpha) > 1.0 - KEPS
    return np.where(pole[..., None], np.stack([0 * alpha, 0 * alpha, np.copysign(1.0, alpha)], axis=-1), ray)


def reflect(V, n):
    with np.errstate(all="ignore"):
        return _unit(n * (2.0 * _dot(V, n))[..., None] - V)


def refract(V, n, ior):
    """ray, total_reflection, the discriminant b (+inf on the index_ratio < kEps exit, which is decided by an exact word) and its bound e_b"""
    with np.errstate(all="ignore"):
        d = np.abs(_dot(n, V))
        b = 1.0 - ior * ior * (1.0 - d * d)
        eb = (10.0 * ior * ior + 2.0) * U
        total = b < 0.0
        through = _unit(n * (ior * d - np.sqrt(np.maximum(b, 0.0)))[..., None] - V * np.asarray(ior)[..., None])
        ray = np.where(total[..., None], reflect(V, n), through)
        out = ior < KEPS
        ray = np.where(out[..., None], -V, ray)
        return ray, total & ~out, np.where(out, np.inf, b), np.where(out, 0.0, eb)


def fresnel_scalars(ndv, ndt, ior):
    with np.errstate(all="ignore"):
        s1, s2, p1, p2 = ior * ndv, ndt, ior * ndt, ndv
        rs, rp = (s1 - s2) / (s1 + s2), (p1 - p2) / (p1 + p2)
        return _sat(0.5 * (rs * rs + rp * rp))


def fresnel_dielectric(n, V, refr, ior):
    return fresnel_scalars(_dot(V, n), -_dot(refr, n), ior)


# ---- microfacet terms; `ds` scales every D (1: the value; "lo" / "hi": the ends of D's interval) ----
def ggx_d(ndh, r4, ds=1):
    with np.errstate(all="ignore"):
        n2 = np.minimum(ndh * ndh, 1.0)
        a = 1.0 - n2 + r4 * n2
        if isinstance(ds, str):
            ea = U * n2 + 2.0 * U * a
            a = a + ea if ds == "lo" else np.where(a - ea > 0, a - ea, 0.0)
        return r4 / (np.pi * a * a)


def ggx_g1(r4, nds):
    with np.errstate(all="ignore"):
        n2 = np.maximum(0.0001, nds * nds)
        return 2.0 / (np.sqrt((r4 * (1.0 - n2) + n2) / n2) + 1.0)


def ggx_g2(r4, ndl, ndv):
    with np.errstate(all="ignore"):
        a = ndv * np.sqrt(r4 + ndl * (ndl - r4 * ndl))
        b = ndl * np.sqrt(r4 + ndv * (ndv - r4 * ndv))
        return 0.5 / (a + b)


def ggx_g2_over_g1(r4, ndl, ndv):
    with np.errstate(all="ignore"):
        g1v, g1l = ggx_g1(r4, ndv), ggx_g1(r4, ndl)
        return g1l / (g1v + g1l - g1v * g1l)


def vndf_k(V, r4):
    with np.errstate(all="ignore"):
        xy2 = V[..., 0] ** 2 + V[..., 1] ** 2
        t = np.sqrt(r4 * xy2 + V[..., 2] ** 2)
        s2 = (1.0 + np.sqrt(xy2)) ** 2
        return (1.0 - r4) * s2 / (s2 + r4 * V[..., 2] ** 2), t


def pdf_vndf_bounded(V, roughness, ndh, ndv, ds=1):
    with np.errstate(all="ignore"):
        r4 = roughness ** 4
        k, t = vndf_k(V, r4)
        return ggx_d(ndh, r4, ds) / (2.0 * (k * ndv + t))


def pdf_refraction(roughness, ndh, ndv, hdv, hdl, ior, ds=1):
    with np.errstate(all="ignore"):
        r4 = roughness ** 4
        den = (ior * hdv + hdl) ** 2
        return ggx_d(ndh, r4, ds) * ggx_g1(r4, ndv) * (hdv / ndv) * (hdl / den)


def pdf_diffuse(ndl):
    return _sat(ndl) * (1.0 / np.pi)


def eval_microfacet(roughness, ndh, ndl, ndv, ds=1):
    r4 = roughness ** 4
    return ggx_d(ndh, r4, ds) * ggx_g2(r4, ndl, ndv) * ndl


def eval_microfacet_over_vndf(V, roughness, ndl, ndv):
    r4 = roughness ** 4
    k, t = vndf_k(V, r4)
    return 2.0 * (k * ndv + t) * ggx_g2(r4, ndl, ndv) * ndl


def eval_microfacet_over_diffuse(roughness, ndh, ndl, ndv, ds=1):
    r4 = roughness ** 4
    return ggx_d(ndh, r4, ds) * ggx_g2(r4, ndl, ndv) * np.pi


def eval_refraction(roughness, hdl, hdv, ndh, ndl, ndv, ior, ds=1):
    with np.errstate(all="ignore"):
        r4 = roughness ** 4
        den = (ior * hdv + hdl) ** 2
        return 4.0 * ndl * hdv * hdl * ggx_d(ndh, r4, ds) * ggx_g2(r4, ndl, ndv) / den


def eval_diffuse_over_vndf(V, roughness, ndl, ndh, ndv, ds=1):
    with np.errstate(all="ignore"):
        r4 = roughness ** 4
        k, t = vndf_k(V, r4)
        return ndl * (2.0 * (k * ndv + t)) / (np.pi * ggx_d(ndh, r4, ds))


# ---- the energy tables ----
def lut_axis(coord):
    x = coord * 32.0 - 0.5
    fl = np.floor(x)
    fl = np.where(np.isfinite(fl), fl, 0.0)   # (a coordinate that is no number: the value is none either, through x - fl)
    x = np.where(np.isfinite(x), x, np.nan)
    return np.clip(fl, 0, 31).astype(np.int64), np.clip(fl + 1, 0, 31).astype(np.int64), x - fl, np.abs(x - np.rint(x))


def _slice(t, x, y):
    a, b, c, d = t[y[0] * 32 + x[0]], t[y[0] * 32 + x[1]], t[y[1] * 32 + x[0]], t[y[1] * 32 + x[1]]
    top, bot = a + x[2] * (b - a), c + x[2] * (d - c)
    return top + y[2] * (bot - top)


def lut2d(table, u, v):
    t = np.asarray(table, dtype=np.float64) / 65535.0
    return _slice(t, lut_axis(u), lut_axis(v))


def lut3d(table, u, v, w):
    t = np.asarray(table, dtype=np.float64) / 65535.0
    x, y, z = lut_axis(u), lut_axis(v), lut_axis(w)
    lo, hi = _slice(t, (x[0] + z[0] * 1024, x[1] + z[0] * 1024, x[2]), y), _slice(t, (x[0] + z[1] * 1024, x[1] + z[1] * 1024, x[2]), y)
    return lo + z[2] * (hi - lo)


class Material:
    """The material words of every thread as MatParams::set packs and its getters unpack them: the integers are exact, the getters are one binary32 product each
    (q * (1 / 1023), q * (1 / 255) * 3), restated in binary32 so that the truth reads the numbers every later stage reads."""

    def __init__(self, vertices, rows):
        f32 = np.float32
        sat = lambda a: np.clip(np.asarray(a, dtype=f32), f32(0), f32(1))
        q = lambda a, n: (sat(a) * f32(n) + f32(0.5)).astype(np.uint32).astype(f32)
        self.roughness = (q(vertices.roughness, 1023) * f32(1.0 / 1023)).astype(np.float64)[rows]
        self.ior = ((q(vertices.ior * f32(1.0 / 3.0), 255) * f32(1.0 / 255)) * f32(3.0)).astype(np.float64)[rows]
        self.opacity = (q(vertices.opacity, 255) * f32(1.0 / 255)).astype(np.float64)[rows]
        self.albedo = (q(vertices.albedo, 1023) * f32(1.0 / 0x3FF)).astype(np.float64)[rows]
        flags = vertices.flags[rows]
        self.translucent = (flags & TRANSLUCENT) != 0
        self.metallic = (flags & METALLIC) != 0
        self.coloured = (flags & COLOURED) != 0
        self.with_diffuse = ~self.translucent & ~self.metallic


def energy_terms(luts, mat, ndv):
    """energy_terms of dev_bsdf.h as an interpolation of the uint16 tables: conductor, glossy, dielectric, and the smallest distance of a coordinate from a cell
    boundary (in cells)"""
    r = mat.roughness
    with np.errstate(all="ignore"):
        w = (1.0 / r - 1.0) * 0.5   # the dielectric table is read with the roughness as ior (sic, bsdf_utils.cuh:517): never above 1
        conductor = np.where(mat.translucent, 1.0, lut2d(luts["conductor"], ndv, r))
        glossy = np.where(mat.with_diffuse, lut2d(luts["glossy"], ndv, r), 0.0)
        dielectric = np.where(mat.translucent, lut3d(luts["dielectric"], ndv, r, np.minimum(w, 1e6)), 1.0)
        edge = np.minimum(lut_axis(ndv)[3], lut_axis(r)[3])
    return conductor, glossy, dielectric, edge


def luminance(c):
    return 0.212655 * c[..., 0] + 0.715158 * c[..., 1] + 0.072187 * c[..., 2]


def importance(c):
    return np.max(c, axis=-1)   # (numpy's max hands a NaN on, as the integer comparison of the bit patterns does for the positive NaN of 0 / 0)


def schlick(f0, f90, hdv):
    t = (1.0 - np.abs(hdv)) ** 5
    return f0 + (f90[..., None] - f0) * t[..., None]


def terms_of(mat, V, H, L, is_refraction):
    """sampled_direction_terms in the shading frame (normal = +z). Returns the dict of the seven words (fresnel None: see fresnel_of) and H.z's sign."""
    ndl = np.where(is_refraction, -L[..., 2], L[..., 2])
    return {"ndl": ndl, "ndv": _sat(V[..., 2]), "hdv": np.abs(_dot(H, V)), "hdl": np.abs(_dot(H, L)), "ndh": np.abs(H[..., 2]), "isr": is_refraction}


def fresnel_of(mat, V, H, L, is_refraction):
    """fresnel_dielectric as sampled_direction_terms forms it, its conditioning bound near the critical angle, and whether the inner total-reflection decision of a
    reflected direction is decided. 1 exactly where the substrate is not translucent."""
    with np.errstate(all="ignore"):
        flip = np.where(H[..., 2] < 0.0, -1.0, 1.0)[..., None]
        Hf = H * flip
        _, total, b, eb = refract(V, H, mat.ior)
        f_refr = fresnel_dielectric(Hf, V, L, mat.ior)
        # a reflected direction: the refracted one is formed inside, N.T = sqrt(b) / length with the root's conditioning
        refr_in, _, _, _ = refract(V, H, mat.ior)
        ndt = -_dot(refr_in, Hf)
        ndvh = _dot(V, Hf)
        e_ndt = eb / (2.0 * np.sqrt(np.maximum(b, 1e-300))) + 8.0 * U
        f_in = fresnel_scalars(ndvh, ndt, mat.ior)
        f_lo, f_hi = fresnel_scalars(ndvh, np.maximum(ndt - e_ndt, 0.0), mat.ior), fresnel_scalars(ndvh, ndt + e_ndt, mat.ior)
        bound = np.maximum(np.abs(f_lo - f_in), np.abs(f_hi - f_in))
        decided = np.abs(b) > eb
        f_reflected = np.where(total, 1.0, f_in)
        bound = np.where(total, 0.0, bound)
        f = np.where(is_refraction, f_refr, f_reflected)
        bound = np.where(is_refraction, 0.0, np.where(decided, bound, np.inf))
        f = np.where(mat.translucent, f, 1.0)
        bound = np.where(mat.translucent, bound, 0.0)
    return f, bound


def eval_layers(mat, energy, c, V, hint, inv_pdf, ds=1):
    """eval_layers of dev_bsdf.h on the terms c (a dict of arrays with the fresnel word "f"): [..., 3]"""
    r, albedo = mat.roughness, mat.albedo
    ndh, ndl, ndv, hdl, hdv, isr, fres_d = c["ndh"], c["ndl"], c["ndv"], c["hdl"], c["hdv"], c["isr"], c["f"]
    conductor_da, glossy_da, dielectric_da = energy
    with np.errstate(all="ignore"):
        iorq = r if hint == REFRACTION else np.ones_like(r)
        if hint == GENERAL:
            ss = eval_microfacet(r, ndh, ndl, ndv, ds) * inv_pdf
        elif hint == MICROFACET:
            ss = eval_microfacet_over_vndf(V, r, ndl, ndv)
        elif hint == DIFFUSE:
            ss = eval_microfacet_over_diffuse(r, ndh, ndl, ndv, ds)
        else:
            ss = eval_microfacet(r, ndh, ndl, ndv, ds) / pdf_refraction(r, ndh, ndv, hdv, hdl, iorq, ds)
        fres = schlick(albedo, np.minimum(1.0, (1.0 / 0.04) * luminance(albedo)), hdv)
        conductor = fres * ss[..., None] + albedo * (fres * (((1.0 / conductor_da) - 1.0) * ss)[..., None])
        if hint == GENERAL:
            diff = pdf_diffuse(ndl) * inv_pdf
        elif hint == DIFFUSE:
            diff = np.ones_like(r)
        elif hint == MICROFACET:
            diff = eval_diffuse_over_vndf(V, r, ndl, ndh, ndv, ds)
        else:
            diff = pdf_diffuse(ndl) / pdf_refraction(r, ndh, ndv, hdv, hdl, iorq, ds)
        f0 = np.full(albedo.shape, 0.04)
        fres0 = schlick(f0, np.minimum(1.0, (1.0 / 0.04) * luminance(f0)), hdv)
        glossy = fres0 * (ss / conductor_da)[..., None] + albedo * (diff * (1.0 - glossy_da))[..., None]
        # the dielectric lobe reads the roughness as ior (sic)
        if hint == GENERAL:
            t_refr = eval_refraction(r, hdl, hdv, ndh, ndl, ndv, r, ds) * inv_pdf
        elif hint == REFRACTION:
            t_refr = ggx_g2_over_g1(r ** 4, ndl, ndv)
        else:
            t_refr = np.zeros_like(r)
        t_refr = t_refr * (1.0 - fres_d)
        if hint == GENERAL:
            t_refl = eval_microfacet(r, ndh, ndl, ndv, ds) * inv_pdf
        elif hint == MICROFACET:
            t_refl = eval_microfacet_over_vndf(V, r, ndl, ndv)
        else:
            t_refl = eval_microfacet(r, ndh, ndl, ndv, ds) / pdf_refraction(r, ndh, ndv, hdv, hdl, r, ds)
        t_refl = t_refl * fres_d
        term = np.where(isr, t_refr, t_refl) / dielectric_da
        term = np.where((r == 1.0) & isr, 1.0 if hint == REFRACTION else 0.0, term)
        dielectric = albedo * term[..., None]
        zero = np.zeros_like(albedo)
        dead = ((ndl <= 0.0) | (ndv <= 0.0))[..., None]
        opaque = (~mat.translucent)[..., None]
        conductor = np.where(dead | ~(opaque & mat.metallic[..., None]), zero, conductor)
        glossy = np.where(dead | ~(opaque & ~mat.metallic[..., None]), zero, glossy)
        dielectric = np.where(dead | opaque, zero, dielectric)
        total = np.where(isr[..., None], dielectric, (conductor + glossy) + dielectric)
        return total * mat.opacity[..., None]


def eval_with_face_normal(mat, energy, c, V, hint, L, fnl, inv_pdf, ds=1):
    """... and the face-normal test: the value, and whether the test is decided (8 u)"""
    with np.errstate(all="ignore"):
        fl = _dot(fnl, L) * np.where(c["isr"], -1.0, 1.0)
        value = eval_layers(mat, energy, c, V, hint, inv_pdf, ds)
        return np.where((fl < KEPS)[..., None], 0.0, value), np.abs(fl - KEPS) > 8.0 * U, fl


def evaluate_direction(luts, mat, nrm, view, L):
    """eval_bsdf under the general hint with inv_pdf 1 (analyze_direction, eval_with_face_normal) in world space for directions L [M, 3] of vertices with unit
    normals and views [M, 3] and a Material of M rows: the value [M, 3] and where it is clear of the horizon. The face normal is the vertex normal through a 16-bit
    octahedral packing (2^-13 of it at most), so the face-normal test and the sign of N.L are decided where |N.L| > 2^-12."""
    with np.errstate(all="ignore"):
        ndl_s = _dot(nrm, L)
        isr = ndl_s < 0.0
        hv = L + view * np.where(isr, mat.ior, 1.0)[..., None]
        ln = np.linalg.norm(hv, axis=-1)
        H = np.where((ln > 0)[..., None], hv / ln[..., None], view)
        flip = np.where(_dot(nrm, H) < 0.0, -1.0, 1.0)[..., None]
        refr, total, _, _ = refract(view, H, mat.ior)
        f = np.where(isr, fresnel_dielectric(H * flip, view, L, mat.ior), np.where(total, 1.0, fresnel_dielectric(H * flip, view, refr, mat.ior)))
        ndv = _sat(_dot(nrm, view))
        c = {"f": np.where(mat.translucent, f, 1.0), "ndh": np.abs(_dot(nrm, H)), "ndl": np.abs(ndl_s), "ndv": ndv, "hdl": np.abs(_dot(H, L)),
             "hdv": np.abs(_dot(H, view)), "isr": isr}
        energy = energy_terms(luts, mat, ndv)[:3]
        return eval_layers(mat, energy, c, view, GENERAL, np.ones_like(ndv)), np.abs(ndl_s) > 2.0 ** -12


def _f(words):
    return np.ascontiguousarray(words, dtype=np.uint32).view(np.float32).astype(np.float64)


def randoms(vertices, first_sample, samples):
    """[V, S, 8, 2] float32: the pairs of the targets reflection, diffuse, refraction, resampling, opacity, light choice, light direction, light roulette"""
    import oracle_lib
    targets = [RT_REFLECTION, RT_DIFFUSE, RT_REFRACTION, RT_RESAMPLING, RT_OPACITY, RT_L_CHOICE, RT_L_DIRECTION, RT_L_RR]
    return np.stack([oracle_lib.random_2d_table(int(px), int(py), first_sample, samples, targets) for px, py in vertices.pixels])


class Truth:
    def __init__(self, luts, vertices, first_sample, samples):
        self.luts, self.vertices, self.samples = luts, vertices, samples
        V = len(vertices)
        self.rows = np.repeat(np.arange(V), samples)
        N = self.N = V * samples
        self.mat = Material(vertices, self.rows)
        self.nrm = _unit(vertices.normal.astype(np.float64))[self.rows]
        self.view = _unit(vertices.V.astype(np.float64))[self.rows]
        r = randoms(vertices, first_sample, samples).reshape(N, 8, 2)
        self.rnd32 = r
        self.rnd = r.astype(np.float64)
        self._chain()

    # ---- the truth's own chain: what it expects and where it is decisive ----
    def _chain(self):
        mat, N = self.mat, self.N
        with np.errstate(all="ignore"):
            q, minus, qlen = rotation_to_z(self.nrm)
            self.q, self.q_minus, self.q_len = q, minus, qlen
            # an axis vector is its own normalisation in binary32: its squared length is 1 without a rounding and the reciprocal root of 1 is 1 in both flavours
            n32 = self.vertices.normal[self.rows]
            axis = ((n32 != 0).sum(axis=-1) == 1) & (np.abs(n32).max(axis=-1) == 1.0)
            self.q_decided = axis | (np.abs(self.nrm[:, 2] - (-1.0 + KEPS)) > 8.0 * U)
            Vl = qapply(q, self.view)
            fnl = qapply(q, self.nrm)
            energy = energy_terms(self.luts, mat, _sat(Vl[:, 2]))
            self.lut_edge = energy[3]
            self.lut_decided = energy[3] > 64.0 * U * 32.0
            draw = self.rnd[:, 4, 0]
            self.passes = (mat.opacity < 1.0) & (draw > mat.opacity)
            pick = self.rnd[:, 3, 0]
            ws, es, dec = [], [], np.ones(N, dtype=bool)
            self.tr_decided = np.ones(N, dtype=bool)
            self.total_reflection = np.zeros(N, dtype=bool)
            self.face_decided = np.ones(N, dtype=bool)
            taken = [~self.passes, ~self.passes & mat.with_diffuse, ~self.passes & mat.translucent]
            self.taken = taken
            for t in range(3):
                w3 = []
                for ds in (1, "lo", "hi"):
                    if t == 0:
                        m, _ = sample_vndf_bounded(Vl, mat.roughness, self.rnd[:, 0])
                        ray = reflect(Vl, m)
                        isr = np.zeros(N, dtype=bool)
                        tr = isr
                    elif t == 1:
                        ray = sample_ray_sphere(self.rnd[:, 1, 0], self.rnd[:, 1, 1])
                        m = _unit(Vl + ray)
                        isr = np.zeros(N, dtype=bool)
                        tr = isr
                    else:
                        m, _ = sample_vndf_caps(Vl, mat.roughness, self.rnd[:, 2])
                        ray, tr, b, eb = refract(Vl, m, mat.ior)
                        isr = ~tr
                        if ds == 1:
                            self.total_reflection = tr & taken[2]
                            self.tr_decided = ~taken[2] | (np.abs(b) > eb + 64.0 * U)   # m and V are the truth's own here: their few u on top
                    c = terms_of(mat, Vl, m, ray, isr)
                    c["f"], _ = fresnel_of(mat, Vl, m, ray, isr)
                    hint = (MICROFACET, DIFFUSE, REFRACTION)[t]
                    ev, face_ok, _ = eval_with_face_normal(mat, energy[:3], c, Vl, hint, ray, fnl, 1.0, ds)
                    if ds == 1:
                        self.face_decided &= face_ok | ~taken[t]
                    pv = pdf_vndf_bounded(Vl, mat.roughness, c["ndh"], c["ndv"], ds)
                    pd = np.where(mat.with_diffuse, pdf_diffuse(c["ndl"]), 0.0)
                    pr = np.where(mat.translucent, pdf_refraction(mat.roughness, c["ndh"], c["ndv"], c["hdv"], c["hdl"], mat.ior, ds), 0.0)
                    own = (pv, pd, pr)[t]
                    s = pv + pd + pr
                    mis = np.where(s > 0.0, own / s, 0.0)
                    if t == 2:
                        mis = np.where(tr, mis, 1.0)
                    w3.append(np.where(taken[t], importance(ev) * mis, 0.0))
                w = np.nan_to_num(w3[0], nan=0.0, posinf=0.0)
                e = np.maximum(np.abs(np.nan_to_num(w3[1], nan=np.inf) - w), np.abs(np.nan_to_num(w3[2], nan=np.inf) - w)) + 64.0 * U * w
                e = np.where(np.isfinite(w3[0]), e, np.inf)
                ws.append(w); es.append(np.where(taken[t], e, 0.0))
            pk, dc, T, eT, _, _ = lt.scan(np.asarray(ws), np.asarray(es), pick[:, None])
            self.chosen = np.where(self.passes, NO_TECHNIQUE, np.maximum(pk[:, 0], 0))
            self.pick_decided = dc[:, 0] | self.passes
            # the light direction
            self.ld_refraction = mat.translucent & ((self.rnd32[:, 5, 0] * np.float32(2.0)).astype(np.uint32) == 1)
            rr = _sat((mat.roughness - 0.5) / (float(np.float32(0.1)) - 0.5))
            self.rr = rr
            self.ld_refused = self.rnd[:, 7, 0] >= rr
            self.rr_decided = np.abs(self.rnd[:, 7, 0] - rr) > 8.0 * U
            sr = mat.roughness + 0.04 * (1.0 - mat.roughness)
            m, _ = sample_vndf_caps(Vl, sr, self.rnd[:, 6])
            _, tr, b, eb = refract(Vl, m, mat.ior)
            live = self.ld_refraction & ~self.ld_refused
            self.ld_total = tr & live
            self.ld_tr_decided = ~live | (np.abs(b) > eb + 64.0 * U)
        self.decisions = {"rotation_to_z's branch": self.q_decided, "total_reflection": self.tr_decided, "pick < prob": self.pick_decided,
                          "the face-normal test": self.face_decided, "the light direction's roulette": self.rr_decided,
                          "the light direction's total_reflection": self.ld_tr_decided, "lut_axis' cell": self.lut_decided}
        # (the opacity draw, the technique draw and NdotH < 0 compare exact words: always decided)
        self.decisive = np.all([v for k, v in self.decisions.items() if k != "lut_axis' cell"], axis=0)
        self.transparent_pass = self.passes | ((self.chosen == 2) & ~self.total_reflection)
        self.microfacet_based = ~self.passes & (self.chosen != 1)
        self.pass_through = self.transparent_pass & ((mat.ior == 1.0) | ~self.microfacet_based)

    def shares(self):
        out = {k: float(v.mean()) for k, v in self.decisions.items()}
        out["all"] = float(self.decisive.mean())
        return out

    # ---- the acceptor ----
    def check(self, out, yardstick=None, factor=4.0, bitwise_walks=True):
        """out [V, S, 143] uint32. Returns (fail: name -> bool [N], fig: name -> largest relative distance over the well-conditioned threads, and the shares of
        ill-conditioned threads of the D-containing words). yardstick: the reference run's figures."""
        N, mat = self.N, self.mat
        o = np.ascontiguousarray(out, dtype=np.uint32).reshape(N, WORDS)
        fo = o.view(np.float32).astype(np.float64)
        fail, fig = {}, {}
        nonfinite = np.zeros(N, dtype=bool)
        false = np.zeros(N, dtype=bool)

        def held(name, got, want, where, scale=1.0, bound=None, ulps=None):
            """a continuous word (or vector: last axis). ulps: a sum / quotient / product of reported words, held to that many ulps of the result and never to a
            yardstick"""
            nonlocal nonfinite
            vec = got.ndim == 2
            red = (lambda a: a.any(axis=-1)) if vec else (lambda a: a)
            alls = (lambda a: a.all(axis=-1)) if vec else (lambda a: a)
            with np.errstate(all="ignore"):
                scale_a = np.broadcast_to(np.asarray(scale, dtype=np.float64)[..., None] if vec and np.ndim(scale) == 1 else np.asarray(scale, dtype=np.float64), got.shape)
                truth_ok = alls(np.isfinite(want) & (np.abs(want) < 3e38))
                nonfinite |= where & truth_ok & red(~np.isfinite(got))
                d = np.abs(got - want)
                if ulps is not None:
                    fail[name] = fail.get(name, false) | (where & truth_ok & red(~(d <= ulps * 2.0 ** -23 * np.abs(want) + TINY)))
                    return
                b = np.zeros(got.shape) if bound is None else np.broadcast_to(bound[..., None] if vec and bound.ndim == 1 else bound, got.shape)
                ill = red(~(b <= ILL * scale_a))
                well = where & truth_ok & ~ill
                rel = d / np.maximum(scale_a, TINY)
                relmax = rel.max(axis=-1) if vec else rel
                fig[name] = max(fig.get(name, 0.0), float(np.max(np.where(well & np.isfinite(relmax), relmax, 0.0))) if well.any() else 0.0)
                # ... and the same in units of the thread's own bound (at least 4 ulp): the yardstick of a thread whose bound is small stays small
                unit = np.maximum(b, ULP4 * scale_a)
                ratio = d / unit
                ratio = ratio.max(axis=-1) if vec else ratio
                key_u = name + " | in units of the thread's bound"
                fig[key_u] = max(fig.get(key_u, 0.0), float(np.max(np.where(well & np.isfinite(ratio), ratio, 0.0))) if well.any() else 0.0)
                if bound is not None:
                    fig[name + " | ill-conditioned share"] = float((where & truth_ok & ill).sum() / max(int(where.sum()), 1))
                    bad = where & truth_ok & ill & red(~((d <= b + TINY) | ~np.isfinite(b)) | ((got < 0) != (want < 0)) & (np.abs(want) > b) & np.isfinite(b))
                    fail[name + " outside its conditioning bound"] = fail.get(name + " outside its conditioning bound", false) | bad
                # the ceiling that holds with or without a yardstick, the reference's answer included
                key_c = name + " beyond %g x its bound" % CEILING
                fail[key_c] = fail.get(key_c, false) | (well & red(~(d <= CEILING * unit + TINY)))
                if yardstick is not None:
                    allowed = np.maximum(np.minimum(factor * yardstick.get(name, 0.0) * scale_a, factor * yardstick.get(key_u, 0.0) * unit), unit)
                    key = name + " beyond %g x the yardstick" % factor
                    fail[key] = fail.get(key, false) | (well & red(~(d <= allowed + TINY)))

        # ---- the frame ----
        q = fo[:, 9:13]
        Vl, fnl = fo[:, 13:16], fo[:, 16:19]
        with np.errstate(all="ignore"):
            fail["quaternion is not a unit quaternion"] = ~(np.abs(_dot(q, q) - 1.0) <= 8.0 * U)
            to_z = qapply(q, self.nrm)
            general = ~(np.abs(to_z - np.array([0.0, 0.0, 1.0])).max(axis=-1) <= 32.0 * U) | (q[:, 2] != 0.0)
            minus_ok = (q == np.array([1.0, 0.0, 0.0, 0.0])).all(axis=-1)
            fail["quaternion does not take the normal to +z"] = np.where(self.q_decided, np.where(self.q_minus, ~minus_ok, general), general & ~minus_ok)
            held("quaternion", q, self.q, ~self.q_minus & self.q_decided, bound=8.0 * U / np.maximum(self.q_len, TINY) + 4.0 * U)
            held("local V", Vl, qapply(q, self.view), np.ones(N, dtype=bool))
            fail["local V is not a unit vector"] = ~(np.abs(np.linalg.norm(Vl, axis=-1) - 1.0) <= 16.0 * U)
            # the face normal is the vertex normal through 16-bit octahedral packing: within 2^-13 of +z, and a unit vector
            fail["local face normal is not the packed vertex normal"] = ~(np.abs(fnl - qapply(q, self.nrm)).max(axis=-1) <= 2.0 ** -13) | ~(
                np.abs(np.linalg.norm(fnl, axis=-1) - 1.0) <= 16.0 * U)
            nonfinite |= ~np.isfinite(fnl).all(axis=-1)
            ndv = _sat(Vl[:, 2])
            e_c, e_g, e_d, _ = energy_terms(self.luts, mat, ndv)
            energy = (fo[:, 19], fo[:, 20], fo[:, 21])
            everyone = np.ones(N, dtype=bool)
            held("energy terms", fo[:, 19:22], np.stack([e_c, e_g, e_d], axis=-1), everyone)
        # ---- the bounce: opacity, pick ----
        drawn = mat.opacity < 1.0
        draw32 = np.where(drawn, self.rnd32[:, 4, 0], np.float32(0.0)).astype(np.float32)
        fail["opacity draw is not the sampler's"] = o[:, 22] != draw32.view(np.uint32)
        fail["opacity outcome is not the draw's"] = o[:, 23] != np.where(drawn, np.where(self.passes, 2, 1), 0)
        passes = self.passes
        live = ~passes
        fail["initial pick is not the sampler's"] = live & (o[:, 24] != self.rnd32[:, 3, 0].view(np.uint32)) | (passes & (o[:, 24] != 0))
        pick = fo[:, 24].copy()
        wsum = np.zeros(N)
        chosen_want = np.zeros(N, dtype=np.int64)
        chosen_eval, chosen_ray = np.zeros((N, 3)), np.zeros((N, 3))
        tp_want, mf_want = np.zeros(N, dtype=bool), np.ones(N, dtype=bool)
        status_all = []
        for t, kind in enumerate(TECH_NAMES):
            w = fo[:, HEAD + TECH_WORDS * t: HEAD + TECH_WORDS * (t + 1)]
            wi = o[:, HEAD + TECH_WORDS * t: HEAD + TECH_WORDS * (t + 1)]
            status = wi[:, 0]
            status_all.append(status)
            taken = self.taken[t]
            on = taken & (status != NOT_TAKEN)
            fail["%s: status" % kind] = (taken != (status != NOT_TAKEN)) | (status > TOTAL_REFLECTION) | ((t < 2) & (status == TOTAL_REFLECTION))
            fail["%s: words of a technique that is not taken" % kind] = ~taken & wi.any(axis=-1)
            m, ray = w[:, 1:4], w[:, 4:7]
            c_got = w[:, 7:13]
            with np.errstate(all="ignore"):
                if t == 0:
                    m_want, m_len = sample_vndf_bounded(Vl, mat.roughness, self.rnd[:, 0])
                    ray_want, b_ray = reflect(Vl, m), None
                    tr = np.zeros(N, dtype=bool)
                elif t == 1:
                    ray_want, b_ray = sample_ray_sphere(self.rnd[:, 1, 0], self.rnd[:, 1, 1]), None
                    m_len = np.linalg.norm(Vl + ray, axis=-1)
                    m_want = (Vl + ray) / m_len[:, None]
                    tr = np.zeros(N, dtype=bool)
                else:
                    m_want, m_len = sample_vndf_caps(Vl, mat.roughness, self.rnd[:, 2])
                    ray_want, tr_want, b, eb = refract(Vl, m, mat.ior)
                    tr = status == TOTAL_REFLECTION
                    decided = np.abs(b) > eb
                    fail["refraction: total_reflection differs on a decisive thread"] = on & decided & (tr != tr_want)
                    # the ray of the branch the answer took, with the root's conditioning
                    through = _unit(m * (mat.ior * np.abs(_dot(m, Vl)) - np.sqrt(np.maximum(b, 0.0)))[:, None] - Vl * mat.ior[:, None])
                    ray_want = np.where((mat.ior < KEPS)[:, None], -Vl, np.where(tr[:, None], reflect(Vl, m), through))
                    b_ray = np.where(tr | (mat.ior < KEPS), 0.0, np.where(b > eb, eb / (2.0 * np.sqrt(np.maximum(b, 1e-300))) + 8.0 * U, np.inf))
                b_m = 4.0 * U / np.maximum(m_len, TINY) + 4.0 * U
                held("%s: m" % kind, m, m_want, on, bound=b_m)
                held("%s: ray" % kind, ray, ray_want, on, bound=b_ray)
                unit_bad = ~(np.abs(np.linalg.norm(m, axis=-1) - 1.0) <= 16.0 * U) | ~(np.abs(np.linalg.norm(ray, axis=-1) - 1.0) <= 16.0 * U)
                fail["%s: m or ray is not a unit vector" % kind] = on & unit_bad
                if t == 1:
                    plane = np.abs(_dot(m, np.cross(Vl, ray))) <= 16.0 * U * np.maximum(1.0, 1.0 / np.maximum(m_len, TINY))
                else:
                    plane = np.abs(_dot(ray, np.cross(Vl, m))) <= 16.0 * U
                fail["%s: ray is not in the plane of V and m" % kind] = on & ~plane
                isr = (t == 2) & ~tr
                isr_a = np.broadcast_to(isr, (N,))
                fail["%s: is_refraction word" % kind] = on & (wi[:, 13] != isr_a.astype(np.uint32))
                c_want = terms_of(mat, Vl, m, ray, isr_a)
                held("%s: terms" % kind, c_got[:, 1:6], np.stack([c_want["ndh"], c_want["ndl"], c_want["ndv"], c_want["hdl"], c_want["hdv"]], axis=-1), on)
                f_want, f_bound = fresnel_of(mat, Vl, m, ray, isr_a)
                if t == 2:   # under total reflection the inner refraction repeats the outer one's discriminant: 1 exactly
                    f_want, f_bound = np.where(tr, 1.0, f_want), np.where(tr, 0.0, f_bound)
                held("%s: fresnel" % kind, c_got[:, 0], f_want, on & mat.translucent, bound=f_bound)
                fail["%s: fresnel of a substrate that is not translucent is not 1" % kind] = on & ~mat.translucent & (c_got[:, 0] != 1.0)
                c = {"f": c_got[:, 0], "ndh": c_got[:, 1], "ndl": c_got[:, 2], "ndv": c_got[:, 3], "hdl": c_got[:, 4], "hdv": c_got[:, 5], "isr": isr_a}
                hint = (MICROFACET, DIFFUSE, REFRACTION)[t]
                ev = w[:, 14:17]
                ev3 = [eval_with_face_normal(mat, energy, c, Vl, hint, ray, fnl, 1.0, ds) for ds in (1, "lo", "hi")]
                ev_want, face_ok = ev3[0][0], ev3[0][1]
                ev_bound = np.maximum(np.abs(ev3[1][0] - ev_want), np.abs(ev3[2][0] - ev_want))
                ev_bound = np.where(np.isfinite(ev_bound), ev_bound, np.inf).max(axis=-1)
                scale = np.maximum(np.abs(ev_want).max(axis=-1), TINY)
                held("%s: eval" % kind, ev, ev_want, on & face_ok, scale=scale, bound=ev_bound)
                either = (ev == 0.0).all(axis=-1) | (np.abs(ev - eval_layers(mat, energy, c, Vl, hint, 1.0)).max(axis=-1) <= np.maximum(ev_bound, 1e-3 * scale))
                fail["%s: eval where the face-normal test is undecided" % kind] = on & ~face_ok & ~either
                fail["%s: negative eval" % kind] = on & (ev < 0.0).any(axis=-1)
                # the pdfs
                has_pdfs = on if t < 2 else on & tr

                def pdf3(ds):
                    pv = pdf_vndf_bounded(Vl, mat.roughness, c["ndh"], c["ndv"], ds)
                    pd = np.where(mat.with_diffuse, pdf_diffuse(c["ndl"]), 0.0)
                    pr = np.where(mat.translucent, pdf_refraction(mat.roughness, c["ndh"], c["ndv"], c["hdv"], c["hdl"], mat.ior, ds), 0.0)
                    return {0: (pv, pd, pr), 1: (pd, pv, pr), 2: (pr, pv, pd)}[t]
                p1, plo, phi = pdf3(1), pdf3("lo"), pdf3("hi")
                names = {0: ("reflection", "diffuse", "refraction"), 1: ("diffuse", "reflection", "refraction"), 2: ("refraction", "reflection", "diffuse")}[t]
                for k in range(3):
                    pb = np.maximum(np.abs(plo[k] - p1[k]), np.abs(phi[k] - p1[k]))
                    pb = np.where(np.isfinite(pb), pb, np.inf)
                    held("%s: pdf of the %s technique" % (kind, names[k]), w[:, 17 + k], p1[k], has_pdfs, scale=np.maximum(np.abs(p1[k]), TINY),
                         bound=None if names[k] == "diffuse" else pb)
                if t == 2:
                    fail["refraction: pdfs without total reflection"] = on & ~tr & wi[:, 17:20].any(axis=-1)
                # mis, w, weight_sum, prob, pick: sums and quotients of reported words
                s = (w[:, 17] + w[:, 18]) + w[:, 19]
                mis_want = np.where(s > 0.0, w[:, 17] / s, 0.0)
                if t == 2:
                    mis_want = np.where(tr, mis_want, 1.0)
                held("%s: mis is not the own pdf over the sum" % kind, w[:, 20], mis_want, on, ulps=4)
                held("%s: w is not importance(eval) * mis" % kind, w[:, 21], importance(ev) * w[:, 20], on, ulps=4)
                wsum_got = fo[:, 25 + t]
                wsum_want = np.where(on, w[:, 21] if t == 0 else wsum + w[:, 21], wsum)
                held("weight_sum is not the sum of the w", wsum_got, wsum_want, live, ulps=4)
                if t == 0:
                    fail["reflection: prob or pick"] = on & ((wi[:, 22] != 0) | (wi[:, 23] != o[:, 24]))
                    chosen_eval, chosen_ray = np.where(on[:, None], ev, chosen_eval), np.where(on[:, None], ray, chosen_ray)
                else:
                    prob = w[:, 22]
                    held("%s: prob is not w over weight_sum" % kind, prob, w[:, 21] / wsum_got, on, ulps=4)
                    accept = pick < prob
                    after = np.clip(np.where(accept, pick / prob, (pick - prob) / (1.0 - prob)), 0.0, lt.HI)
                    after = np.where(np.isnan(np.where(accept, pick / prob, (pick - prob) / (1.0 - prob))), 0.0, after)   # fmaxf drops the NaN
                    held("%s: pick after the decision" % kind, w[:, 23], after, on, ulps=4)
                    take = on & accept
                    chosen_want = np.where(take, t, chosen_want)
                    chosen_eval, chosen_ray = np.where(take[:, None], ev, chosen_eval), np.where(take[:, None], ray, chosen_ray)
                    tp_want = np.where(take, (t == 2) & ~tr, tp_want)
                    mf_want = np.where(take, t == 2, mf_want)
                    pick = np.where(on, w[:, 23], pick)
                wsum = np.where(live, wsum_got, wsum)
        # ---- the walk's result and the head ----
        with np.errstate(all="ignore"):
            fail["chosen technique is not the walk's decisions'"] = o[:, 28] != np.where(passes, NO_TECHNIQUE, chosen_want)
            fail["chosen technique differs from the truth's on a decisive thread"] = self.decisive & (o[:, 28] != self.chosen)
            imp = importance(chosen_eval)
            weight_want = np.where((wsum > 0.0)[:, None], chosen_eval * (wsum / imp)[:, None], 0.0)
            albedo_or_one = np.where(mat.coloured[:, None], mat.albedo, 1.0)
            weight_want = np.where(passes[:, None], albedo_or_one, weight_want)
            held("final weight is not chosen_eval * (weight_sum / importance)", fo[:, 29:32], weight_want, everyone, ulps=4)
            back = _unit(qapply(qinv(q), chosen_ray))
            held("world ray", fo[:, 32:35], back, live)
            held("world ray", fo[:, 32:35], -self.view, passes)
            fail["world ray is not a unit vector"] = ~(np.abs(np.linalg.norm(fo[:, 32:35], axis=-1) - 1.0) <= 16.0 * U)
            tp_want, mf_want = np.where(passes, True, tp_want), np.where(passes, False, mf_want)
            fail["flags are not the chosen technique's"] = (o[:, 35] != tp_want) | (o[:, 36] != mf_want)
            fail["flags differ from the truth's on a decisive thread"] = self.decisive & ((o[:, 0] != self.transparent_pass) | (o[:, 1] != self.microfacet_based) | (
                o[:, 2] != self.pass_through))
            fail["is_pass_through is not transparent_pass and (ior == 1 or not microfacet_based)"] = o[:, 2] != ((o[:, 0] != 0) & ((mat.ior == 1.0) | (o[:, 1] == 0)))
            fail["the two walks' flags differ"] = (o[:, 0] != o[:, 35]) | (o[:, 1] != o[:, 36])
            if bitwise_walks:
                fail["the two walks' rays differ"] = (o[:, 3:6] != o[:, 32:35]).any(axis=-1)
                fail["the two walks' weights differ"] = (o[:, 6:9] != o[:, 29:32]).any(axis=-1)
            else:   # two inlined copies may contract differently: the rotation's bound (three products and sums of unit vectors, a normalisation: 16 u), and
                # the weight's two quotients and a product (16 u of it)
                fail["the two walks' rays differ"] = ~(np.abs(fo[:, 3:6] - fo[:, 32:35]).max(axis=-1) <= 16.0 * U)
                fail["the two walks' weights differ"] = ~(np.abs(fo[:, 6:9] - fo[:, 29:32]) <= 16.0 * U * np.abs(fo[:, 29:32]) + TINY).all(axis=-1)
            nonfinite |= ~np.isfinite(fo[:, 3:9]).all(axis=-1)
            # hemisphere: a bounce that is no transparent pass leaves on the face normal's side or carries nothing; a transparent one on the other side
            side = _dot(fnl, chosen_ray)
            zero_w = (fo[:, 6:9] == 0.0).all(axis=-1)
            transparent = o[:, 35] != 0
            fail["hemisphere"] = live & ~zero_w & np.where(transparent, ~(side <= -KEPS + 8.0 * U), ~(side >= KEPS - 8.0 * U))
        # ---- the light direction ----
        L = fo[:, LD0:LD0 + LD_WORDS]
        Li = o[:, LD0:LD0 + LD_WORDS]
        with np.errstate(all="ignore"):
            status = Li[:, 0]
            rr, sr = L[:, 1], L[:, 2]
            held("light direction: rr", rr, self.rr, everyone, ulps=4)
            fail["light direction: rr"] = fail["light direction: rr"] | ~(np.abs(rr - self.rr) <= 8.0 * U)
            refused = self.rnd[:, 7, 0] >= rr
            fail["light direction: roulette"] = (refused != (status == LD_REFUSED)) | (self.rr_decided & (self.ld_refused != (status == LD_REFUSED)))
            on = ~refused & (status != LD_REFUSED)
            refraction = self.ld_refraction
            tr = status == LD_REFRACTION_TOTAL
            fail["light direction: technique"] = on & (refraction != (status >= LD_REFRACTION))
            fail["light direction: words after a refused roulette"] = (status == LD_REFUSED) & (Li[:, 2:].any(axis=-1) | o[:, 40:44].any(axis=-1) | (
                o[:, 37:40] != np.float32([0.0, 0.0, 1.0]).view(np.uint32)).any(axis=-1))
            held("light direction: sampling roughness", sr, mat.roughness + 0.04 * (1.0 - mat.roughness), on, ulps=4)
            m, ray = L[:, 3:6], L[:, 6:9]
            mb, lb = sample_vndf_bounded(Vl, sr, self.rnd[:, 6])
            mc, lc = sample_vndf_caps(Vl, sr, self.rnd[:, 6])
            m_want, m_len = np.where(refraction[:, None], mc, mb), np.where(refraction, lc, lb)
            held("light direction: m", m, m_want, on, bound=4.0 * U / np.maximum(m_len, TINY) + 4.0 * U)
            _, tr_want, b, eb = refract(Vl, m, mat.ior)
            fail["light direction: total_reflection differs on a decisive thread"] = on & refraction & (np.abs(b) > eb) & (tr != tr_want)
            through = _unit(m * (mat.ior * np.abs(_dot(m, Vl)) - np.sqrt(np.maximum(b, 0.0)))[:, None] - Vl * mat.ior[:, None])
            refr_ray = np.where((mat.ior < KEPS)[:, None], -Vl, np.where(tr[:, None], reflect(Vl, m), through))
            ray_want = np.where(refraction[:, None], refr_ray, reflect(Vl, m))
            b_ray = np.where(~refraction | tr | (mat.ior < KEPS), 0.0, np.where(b > eb, eb / (2.0 * np.sqrt(np.maximum(b, 1e-300))) + 8.0 * U, np.inf))
            held("light direction: ray", ray, ray_want, on, bound=b_ray)
            unit_bad = ~(np.abs(np.linalg.norm(m, axis=-1) - 1.0) <= 16.0 * U) | ~(np.abs(np.linalg.norm(ray, axis=-1) - 1.0) <= 16.0 * U)
            fail["light direction: m or ray is not a unit vector"] = on & unit_bad
            fail["light direction: ray is not in the plane of V and m"] = on & ~(np.abs(_dot(ray, np.cross(Vl, m))) <= 16.0 * U)
            isr = refraction & ~tr
            fail["light direction: is_refraction word"] = on & (Li[:, 15] != isr.astype(np.uint32))
            c_got = L[:, 9:15]
            c_want = terms_of(mat, Vl, m, ray, isr)
            held("light direction: terms", c_got[:, 1:6], np.stack([c_want["ndh"], c_want["ndl"], c_want["ndv"], c_want["hdl"], c_want["hdv"]], axis=-1), on)
            f_want, f_bound = fresnel_of(mat, Vl, m, ray, isr)
            f_want, f_bound = np.where(tr, 1.0, f_want), np.where(tr, 0.0, f_bound)
            held("light direction: fresnel", c_got[:, 0], f_want, on & mat.translucent, bound=f_bound)
            fail["light direction: fresnel of a substrate that is not translucent is not 1"] = on & ~mat.translucent & (c_got[:, 0] != 1.0)
            c = {"f": c_got[:, 0], "ndh": c_got[:, 1], "ndl": c_got[:, 2], "ndv": c_got[:, 3], "hdl": c_got[:, 4], "hdv": c_got[:, 5], "isr": isr}
            pdf = L[:, 16]

            def ld_pdf(ds):
                return np.where(refraction, pdf_refraction(sr, c["ndh"], c["ndv"], c["hdv"], c["hdl"], mat.ior, ds), pdf_vndf_bounded(Vl, sr, c["ndh"], c["ndv"], ds))
            p1 = ld_pdf(1)
            pb = np.maximum(np.abs(ld_pdf("lo") - p1), np.abs(ld_pdf("hi") - p1))
            held("light direction: pdf", pdf, p1, on, scale=np.maximum(np.abs(p1), TINY), bound=np.where(np.isfinite(pb), pb, np.inf))
            ev3 = [eval_with_face_normal(mat, energy, c, Vl, GENERAL, ray, fnl, 1.0 / pdf, ds) for ds in (1, "lo", "hi")]
            ev_want, face_ok = ev3[0][0], ev3[0][1]
            ev_bound = np.maximum(np.abs(ev3[1][0] - ev_want), np.abs(ev3[2][0] - ev_want))
            ev_bound = np.where(np.isfinite(ev_bound), ev_bound, np.inf).max(axis=-1)
            scale = np.maximum(np.abs(ev_want).max(axis=-1), TINY)
            before, after = L[:, 17:20], L[:, 20:23]
            held("light direction: weight", before, ev_want, on & face_ok, scale=scale, bound=ev_bound)
            fail["light direction: negative weight"] = on & (before < 0.0).any(axis=-1)
            held("light direction: weight after 1 / rr", after, before * (1.0 / rr)[:, None], on, ulps=4)
            coef = np.where(mat.translucent, 0.5, np.where(refraction, 0.0, 1.0))
            held("light direction: probability is not (1 - refr_prob or refr_prob) * pdf * rr", L[:, 23], coef * pdf * rr, on, ulps=4)
            held("light direction: world ray", L[:, 24:27], _unit(qapply(qinv(q), ray)), on)
            if bitwise_walks:
                fail["light direction: the two walks differ"] = on & ((o[:, 37:40] != Li[:, 24:27]).any(axis=-1) | (o[:, 40:43] != Li[:, 20:23]).any(axis=-1) | (o[:, 43] != Li[:, 23]))
            else:
                fail["light direction: the two walks differ"] = on & (~(np.abs(fo[:, 37:40] - L[:, 24:27]).max(axis=-1) <= 16.0 * U) | ~(
                    (np.abs(fo[:, 40:43] - after) <= 16.0 * U * np.abs(after) + TINY) | (o[:, 40:43] == Li[:, 20:23])).all(axis=-1) | ~(
                    (np.abs(fo[:, 43] - L[:, 23]) <= 16.0 * U * np.abs(L[:, 23]) + TINY) | (o[:, 43] == Li[:, 23])))
            # a light direction's sample is no number only where the truth's is none: its weight is eval / pdf, 0 / 0 where the pdf underflows
            nonfinite |= on & np.isfinite(ev_want).all(axis=-1) & ~(np.isfinite(fo[:, 37:43]).all(axis=-1) & np.isfinite(before).all(axis=-1))
            nonfinite |= on & np.isfinite(L[:, 23]) & ~np.isfinite(fo[:, 43])
        fail["non-finite word"] = nonfinite
        self.statuses = (status_all, status)
        return fail, fig
