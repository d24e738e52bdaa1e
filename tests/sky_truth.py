"""A float64 truth for the procedural sky's ray march (csrc/device/dev_sky.h sky_compute_path, sky_compute_atmosphere, sky_get_color, sky_trace_inscattering) and its
two tables (kernels_scene.h k_sky_transmittance_lut, k_sky_multiscattering_lut), and an acceptor for what a binary32 implementation may answer through the sky probe
(include/lum_core.h lumc_sky_probe_host). Test infrastructure only; plain numpy, nothing here is taken from what a device or the oracle returned.

The acceptor is STAGE-WISE, as tests/bsdf_truth.py's: a stage's word is recomputed in float64 from the words the answer itself reports for the stage before -
    path start and distance from the ray; the marched distance from the reported path and the limit; a step's reach from the reported start, distance and step count;
    height, cos_angle, zenith_cos and the shadow from the reported reach; the two phases from the reported cos_angle; u, v from the reported height and zenith_cos;
    extinction_sun from the reported u, v and ms_tex from the reported zenith_cos and height, on the binary32 tables the answer was computed with; step_t from the
    reported height and the two reported reaches; result and transmittance after the step from the reported words of the step and of the step before; the final
    spectrum from the last reported result, the marched transmittance and the reported hit distances; the colour from the reported spectrum
- so the eight-step recurrence and the colour do not accumulate a chain.

Every word carries a FORWARD BOUND from the conditioning of its formula in binary32 (u = 2^-24; a sum of n products carries n u of the sum of magnitudes):
    sphere tests (math.cuh:620-779): d0 = o.r carries 3 u sum|o_i r_i|; k = o - r d0 carries per component |r_i| e(d0) + u |r_i d0| + u |k_i|; the discriminant
        r^2 - k.k carries u r^2 + 2 sum|k_i| e(k_i) + 3 u k.k: at the earth's radius that is some 10 km^2 (an ulp of 6371^2 is 4 km^2), about the sun, where the
        difference o - p is formed at 1.5e8 km and an ulp is 16 km, some 3e7 km^2 against r^2 = 4.8e11. c = o.o - r^2 carries 4 u (o.o + r^2): from 106 m above the
        ground c = 2 R h = 1350 km^2 of the earth's sphere is known to 0.7 %, and so is the distance c / q to the ground below. The root carries e / (2 sqrt d), the quotient both terms.
    height = |pos| - R: 2.5 u |pos| and the position's own u (|pos| + reach): 1.4e-3 km whatever the height is.
    sky_transmittance_uv (sky_utils.cuh:273-287): disc = h^2 (z^2 - 1) + A^2 and rho^2 = h^2 - R^2 carry 3 u h^2 = 7 km^2; d - d_min cancels.
    hg_phase: den = 1 + g^2 - 2 g c carries 6 u, den^-3/2 1.5 times that relative to den (g = 0.99 at the sun: den = 1e-4), 1 - g^2 carries 2 u.
    exp(x) carries (4 |x| + 4) u, plus the measured error of v_exp_f32 in the fast flavour (`hw`, see tests/test_sky_truth.py).
    S - S step_t carries 3 u S, which is all of it when the step is short (limit 1e-4 km).
    a bilinear fetch carries the table's slope times the coordinate's error (2 u of the texel coordinate), the interpolant being continuous across texels.
A word whose bound exceeds ILL = 1e-2 of its scale is ill-conditioned: it is held to finiteness and that bound alone. Everything else lies within CEILING = 4 times its
thread's bound, 16 ulp of its scale at least, whatever the yardstick says (bsdf_truth.py has the reasoning), and within `factor` times the yardstick run's distance.

DECISIONS carry a margin: the truth classes them decided where the margin exceeds the bound, and only there an answer must agree: height <= earth radius and
height > shell radius (4 u |o|), the sphere hits (discriminant, and the signs of c and q), the step count's truncation ((int) x: x within 8 u of an integer is
undecided), the shadow of a step, the sun's rim. Besides the stage-wise walk the truth runs the chain on its own values and calls a ray DECISIVE when all of these are.

Reference quirks, restated as they are: the cap's solid angle is 2 pi a^2 with a = asin(r / d) (math.cuh:1429-1439) where the exact one is 2 pi (1 - cos a) =
pi a^2 (1 - a^2 / 12): the reference's is twice the cap (1 + a^2 / 6 above it at the sun's 4.65 mrad), and light_angle with it; the star grid's cell is not clamped there (sky.cuh:486-489) and is here, to the last cell the generator fills; the Rayleigh phase's pi
is 3.1415926535f (sky.cuh:70).

Not restated: the moon's shading (its hit and lit decisions are).
"""
import numpy as np

import bsdf_truth as bt

U = 2.0 ** -24
ULP4 = 4.0 * 2.0 ** -23
TINY = 1e-37
ILL = 1e-2
CEILING = 4.0
FLT_MAX = float(np.finfo(np.float32).max)
R_E, R_SUN, D_SUN, H_ATMO, R_MOON, HEIGHT_OFFSET = 6371.0, 696340.0, 149597870.0, 100.0, float(np.float32(1737.4)), float(np.float32(0.0005))
R_A = R_E + H_ATMO
H_HORIZON = np.sqrt(R_A * R_A - R_E * R_E)
REF_PI = float(np.float32(3.141592653589))
RAY_WORDS, WORDS, HEAD, STEP_WORDS, MAX_STEPS = 12, 628, 40, 49, 12
CELESTIALS, PRIMARY, AERIAL = 1, 2, 4
NO_CELL = 0xFFFFFFFF
RECORD_IN = np.array([0.75, 0.5, 0.25])


def _c(values):
    """the binary32 constants of sky_utils.cuh as the numbers they are"""
    return np.asarray(values, dtype=np.float32).astype(np.float64)


SP_IDENT = _c([8.4205e-03, 2.6449e-01, 4.0273e-01, 1.6624e-01, 2.4324e-01, 3.5849e-01, 3.6342e-01, 2.4177e-01])                      # sky_utils.cuh:112-127
SUN_RADIANCE = _c([2.463170e+04, 2.888721e+04, 2.795153e+04, 2.629836e+04, 2.667237e+04, 2.638737e+04, 2.490630e+04, 2.338930e+04])  # :251-259
RAYLEIGH = _c([3.945800e-02, 2.939289e-02, 2.235060e-02, 1.730112e-02, 1.360286e-02, 1.084340e-02, 8.750306e-03, 7.139216e-03])      # :260-264
OZONE = _c([1.484836e-05, 8.501668e-05, 2.646158e-04, 7.953520e-04, 1.661103e-03, 2.510733e-03, 2.697211e-03, 1.727741e-03])         # :265-269
MIE_SCATTERING = float(np.float32(3.996) * np.float32(0.001))
MIE_EXTINCTION = float(np.float32(4.440) * np.float32(0.001))
RGB_MATRIX = _c([[0.00640271, 0.179441, 0.04852, -0.43822, -0.920721, -0.0226871, 1.83443, 2.36265],                                 # sky_utils.cuh:289-316
                 [-0.00550232, -0.164, -0.119836, 0.365423, 1.28952, 1.41809, 0.629138, -0.0816028],
                 [0.0386558, 1.21426, 1.80395, 0.475181, -0.0638328, -0.169502, -0.114583, -0.0374822]])


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _adot(a, b):
    return (np.abs(a) * np.abs(b)).sum(axis=-1)


def _unit(v):
    return v / np.sqrt(_dot(v, v))[..., None]


def _f(words):
    return np.ascontiguousarray(words, dtype=np.uint32).view(np.float32).astype(np.float64)


def _e_sqrt(x, e):
    """how far the root of a number known to e can be from the root of x (x >= 0 after the clamp the callers apply), plus the root's own rounding"""
    x = np.maximum(x, 0.0)
    r = np.sqrt(x)
    return np.maximum(np.sqrt(x + e) - r, r - np.sqrt(np.maximum(x - e, 0.0))) + U * r


class Atmosphere:
    """The parameters the kernels read (DeviceSky, device_structs.h:101-124), taken from a scene view, and the two binary32 tables the answers were computed with."""
    FIELDS = ("sun_strength", "base_density", "rayleigh_density", "mie_density", "ozone_density", "rayleigh_falloff", "mie_falloff", "ground_visibility",
              "ozone_layer_thickness", "multiscattering_factor")

    def __init__(self, view, tm=None, ms=None):
        for k in self.FIELDS:
            setattr(self, k, float(getattr(view, "sky_" + k)))
        self.steps, self.ozone_absorption = int(view.sky_steps), bool(view.sky_ozone_absorption)
        self.sun_pos = np.array(list(view.sky_sun_pos), dtype=np.float64)
        self.moon_pos = np.array(list(view.sky_moon_pos), dtype=np.float64)
        self.has_moon = view.sky_moon_albedo_tex != 0xFFFFFFFF
        self.geometry_offset = np.array(list(view.sky_geometry_offset), dtype=np.float64)
        self.g_hg, self.g_d, self.alpha, self.w_d = [float(x) for x in view.sky_mie_phase]
        self.has_stars = bool(view.sky_stars)
        self.stars_intensity = float(view.sky_stars_intensity)
        if self.has_stars:   # 4 floats per star in grid order: altitude, azimuth, radius, intensity; 64 x 32 + 1 cell offsets
            import ctypes as C
            count = int(view.sky_stars_count)
            self.stars = np.ctypeslib.as_array(C.cast(view.sky_stars, C.POINTER(C.c_float)), shape=(count, 4)).astype(np.float64)
            self.star_offsets = np.ctypeslib.as_array(C.cast(view.sky_stars_offsets, C.POINTER(C.c_uint32)), shape=(64 * 32 + 1,)).astype(np.int64)
        self.set_tables(tm, ms)

    def set_tables(self, tm, ms):
        self.tm = None if tm is None else np.asarray(tm, dtype=np.float32).reshape(2, 64, 256, 4).astype(np.float64)
        self.ms = None if ms is None else np.asarray(ms, dtype=np.float32).reshape(2, 32, 32, 4).astype(np.float64)


# ---- the sphere tests (math.cuh:620-779) ----
def sphere(ray, origin, centre, r, back=False, e_o=0.0, e_r=0.0):
    """sph_int_p0 / sphere_int (back: sph_int_back_p0) of rays [..., 3] from origins [..., 3] against the sphere of radius r about `centre`; e_o, e_r: what the
    caller's binary32 origin and direction already carry per component. Returns t (FLT_MAX: no hit), its bound, `hit` as sph_hit_p0 / sphere_hit see it, and whether
    every decision on the way is decided."""
    with np.errstate(all="ignore"):
        centre = np.asarray(centre, dtype=np.float64)
        diff = origin - centre
        e_diff = np.broadcast_to(e_o, diff.shape) + (U * np.abs(diff) if centre.any() else 0.0)
        e_ray = np.broadcast_to(e_r, ray.shape)
        d0 = _dot(diff, ray)
        e_d0 = 3.0 * U * _adot(diff, ray) + _adot(e_diff, ray) + _adot(diff, e_ray)
        r2 = r * r
        e_r2 = U * r2
        dd = _dot(diff, diff)
        c = dd - r2
        e_c = 3.0 * U * dd + 2.0 * _adot(diff, e_diff) + e_r2 + U * np.abs(c)
        k = diff - ray * d0[..., None]
        e_k = e_diff + np.abs(ray) * e_d0[..., None] + np.abs(d0)[..., None] * e_ray + U * np.abs(ray * d0[..., None]) + U * np.abs(k)
        kk = _dot(k, k)
        disc = r2 - kk
        e_disc = e_r2 + 2.0 * _adot(k, e_k) + 3.0 * U * kk + U * np.abs(disc)
        miss = disc < 0.0
        sd = np.sqrt(np.maximum(disc, 0.0))
        e_sd = _e_sqrt(disc, e_disc)
        q = -d0 - np.copysign(sd, d0)
        e_q = e_d0 + e_sd + U * np.abs(q)
        t0 = c / q
        e_t0 = e_c / np.abs(q) + np.abs(c) * e_q / (q * q) + U * np.abs(t0)
        signs = (np.abs(c) > e_c) & (np.abs(q) > e_q)
        if back:
            t = np.where(q >= 0.0, q, np.where(t0 >= 0.0, t0, FLT_MAX))
            e_t = np.where(q >= 0.0, e_q, np.where(t0 >= 0.0, e_t0, 0.0))
            decided = (np.abs(q) > e_q) & ((q >= 0.0) | signs)
        else:
            t = np.where(t0 >= 0.0, t0, np.where(q >= 0.0, q, FLT_MAX))
            e_t = np.where(t0 >= 0.0, e_t0, np.where(q >= 0.0, e_q, 0.0))
            decided = signs
        t = np.where(miss, FLT_MAX, t)
        e_t = np.where(miss, 0.0, e_t)
        decided = (np.abs(disc) > e_disc) & (miss | decided)
        hit = ~miss & (t0 >= 0.0)
        return {"t": t, "e": np.where(np.isfinite(e_t), e_t, np.inf), "hit": hit, "decided": decided, "disc": disc, "e_disc": e_disc}


def sphere_solid_angle(p, r, origin, two_pi=2.0 * np.pi, exact=False):
    """math.cuh:1429-1439: 2 pi a^2 with a = asin(r / d), the reference's form - twice the cap's 2 pi (1 - cos a) (`exact`)"""
    d = np.sqrt(_dot(p - origin, p - origin))
    with np.errstate(all="ignore"):
        a = np.arcsin(np.minimum(r / d, 1.0))
    val = two_pi * (1.0 - np.cos(a)) if exact else two_pi * a * a
    return np.where(d < r, two_pi, val)


# ---- sky_compute_path (sky.cuh:78-108) ----
def compute_path(origin, ray):
    h = np.sqrt(_dot(origin, origin))
    e_h = 4.0 * U * h
    below, above = h <= R_E, h > R_A
    earth, atmo, atmo2 = sphere(ray, origin, 0.0, R_E), sphere(ray, origin, 0.0, R_A), sphere(ray, origin, 0.0, R_A, back=True)
    with np.errstate(all="ignore"):
        inside_d = np.minimum(earth["t"], atmo["t"])
        inside_e = np.where(earth["t"] <= atmo["t"], earth["e"], atmo["e"])
        a, b = earth["t"] - atmo["t"], atmo2["t"] - atmo["t"]
        above_d = np.minimum(a, b)
        above_e = np.where(a <= b, earth["e"], atmo2["e"]) + atmo["e"] + U * np.abs(above_d)
    start = np.where(below, 0.0, np.where(above, atmo["t"], 0.0))
    dist = np.where(below, -FLT_MAX, np.where(above, above_d, inside_d))
    decided = (np.abs(h - R_E) > e_h) & (below | ((np.abs(h - R_A) > e_h) & earth["decided"] & atmo["decided"] & (~above | atmo2["decided"])))
    return {"start": start, "e_start": np.where(above & ~below, atmo["e"], 0.0), "distance": dist, "e_distance": np.where(below, 0.0, np.where(above, above_e, inside_e)),
            "decided": decided, "below": below, "below_decided": np.abs(h - R_E) > e_h, "above": above, "above_decided": np.abs(h - R_A) > e_h,
            "earth": earth, "atmo": atmo, "height": h}


def step_count(limit, primary, sky_steps, step_random):
    """sky_trace_inscattering (sky.cuh:517-532): (int) (clamp(limit / base_range, 0.5, 2) (steps / 6) + step_random - 0.5); the margin of the truncation"""
    base = np.where(primary, 40.0, 80.0)
    k = (sky_steps // 6).astype(np.float64)
    with np.errstate(all="ignore"):
        c = np.clip(limit / base, 0.5, 2.0)
        x = c * k + step_random - 0.5
        # binary32 forms the same number wherever every operation on the way is exact (limit 40 primary, step_random 0.5: x = 1 exactly, and (int) x is 1)
        c32 = np.clip(limit.astype(np.float32) / base.astype(np.float32), np.float32(0.5), np.float32(2.0))
        p32 = c32 * k.astype(np.float32)
        s32 = p32 + step_random.astype(np.float32)
        exact = (c32.astype(np.float64) == c) & (p32.astype(np.float64) == c * k) & (s32.astype(np.float64) == c * k + step_random) & ((s32 - np.float32(0.5)).astype(np.float64) == x)
    e = np.where(exact, 0.0, 8.0 * U * (np.abs(x) + 2.0 * k + 1.0))
    n = np.trunc(x)
    edge = np.where(np.abs(x) < 1.0, 1.0 - np.abs(x), np.minimum(np.abs(x) - np.abs(n), np.abs(n) + 1.0 - np.abs(x)))
    return n.astype(np.int64), (edge > e) | exact


# ---- densities, medium, phases (sky.cuh:47-75, math.cuh:1162-1239) ----
def medium(atm, h, hw_exp=0.0):
    """sky_medium at heights h [...]: scattering_rayleigh [..., 8], scattering_mie [...], scattering, extinction [..., 8] and their bounds (relative `rel`, and the
    ozone profile's absolute part `e_abs` of the extinction)"""
    xr, xm = -h / atm.rayleigh_falloff, -h / atm.mie_falloff
    with np.errstate(all="ignore"):
        dr = 2.5 * atm.base_density * np.exp(xr) * atm.rayleigh_density
        waso = np.where(h < 2.0, 1.0 + 0.125 * (2.0 - h), np.where(h < 3.0, 3.0 - h, 0.0)) * (60.0 / atm.ground_visibility)
        dm = atm.base_density * (np.exp(xm) + waso) * atm.mie_density
        if atm.ozone_absorption:
            doz = atm.base_density * np.maximum(np.where(h > 25.0, 0.0, 0.1), 1.0 - np.abs(h - 25.0) / atm.ozone_layer_thickness) * atm.ozone_density
        else:
            doz = np.zeros_like(h)
    scat_r = RAYLEIGH * dr[..., None]
    scat_m = MIE_SCATTERING * dm
    ext = scat_r + (MIE_EXTINCTION * dm)[..., None] + OZONE * doz[..., None]
    rel = (4.0 * np.maximum(np.abs(xr), np.abs(xm)) + 16.0) * U + hw_exp * (1.0 + np.maximum(np.abs(xr), np.abs(xm)))
    e_abs = 4.0 * U * OZONE * atm.base_density * atm.ozone_density * (1.0 + np.abs(h - 25.0)[..., None] / atm.ozone_layer_thickness) * (1.0 if atm.ozone_absorption else 0.0)
    return {"scat_r": scat_r, "scat_m": scat_m, "scat": scat_r + scat_m[..., None], "ext": ext, "rel": rel, "e_abs": e_abs}


def rayleigh_phase(c, sixteen_pi=16.0 * np.pi):
    """sky.cuh:70: 3 (1 + c^2) / (16 pi) = (3 / 4) (1 + c^2) / (2 pi) / 2"""
    return 3.0 * (1.0 + c * c) / sixteen_pi


def hg_phase(c, g, four_pi=4.0 * np.pi):
    """math.cuh:1162-1168, with the bound: den carries 6 u, its power -3/2 one and a half times that relative to den; 1 - g^2 carries 2 u"""
    den = 1.0 + g * g - 2.0 * g * c
    with np.errstate(all="ignore"):
        val = (1.0 - g * g) / (four_pi * den * np.sqrt(den))
        rel = 9.0 * U / den + 2.0 * U / (1.0 - g * g) + 6.0 * U
    return val, np.abs(val) * rel


def mie_phase(atm, c, swap_weights=False, four_pi=4.0 * np.pi):
    """Jendersie-Eon (math.cuh:1189-1239): (1 - w_d) HG(g_hg) + w_d Draine(g_d, alpha)"""
    hg, e_hg = hg_phase(c, atm.g_hg, four_pi)
    dh, e_dh = hg_phase(c, atm.g_d, four_pi)
    f = (1.0 + atm.alpha * c * c) / (1.0 + (atm.alpha / 3.0) * (1.0 + 2.0 * atm.g_d * atm.g_d))
    w = 1.0 - atm.w_d if swap_weights else atm.w_d
    val = (1.0 - w) * hg + w * dh * f
    return val, np.abs(1.0 - w) * e_hg + np.abs(w * f) * e_dh + 8.0 * U * (np.abs((1.0 - w) * hg) + np.abs(w * dh * f))


# ---- sky_transmittance_uv (sky_utils.cuh:273-287) and the software fetch ----
def transmittance_uv(height, zenith_cos, e_height=0.0, e_z=0.0):
    h = height + R_E
    e_h = e_height + U * h
    hh = h * h
    e_hh = 2.0 * h * e_h + U * hh
    rho2 = hh - R_E * R_E
    e_rho2 = e_hh + U * R_E * R_E + U * np.abs(rho2)
    rho = np.sqrt(np.maximum(rho2, 0.0))
    e_rho = _e_sqrt(rho2, e_rho2)
    t2 = zenith_cos * zenith_cos - 1.0
    e_t2 = 2.0 * np.abs(zenith_cos) * e_z + U * zenith_cos * zenith_cos + U * np.abs(t2)
    disc = hh * t2 + R_A * R_A
    e_disc = hh * e_t2 + np.abs(t2) * e_hh + U * np.abs(hh * t2) + U * R_A * R_A + U * np.abs(disc)
    d = np.maximum(0.0, -h * zenith_cos + np.sqrt(np.maximum(disc, 0.0)))
    e_d = np.abs(zenith_cos) * e_h + h * e_z + U * np.abs(h * zenith_cos) + _e_sqrt(disc, e_disc) + U * np.abs(d)
    d_min, d_max = R_A - h, rho + H_HORIZON
    e_dmin = e_h + U * np.abs(d_min)
    e_dmax = e_rho + 4.0 * U * H_HORIZON + U * d_max
    num, den = d - d_min, d_max - d_min
    e_num, e_den = e_d + e_dmin + U * np.abs(num), e_dmax + e_dmin + U * np.abs(den)
    with np.errstate(all="ignore"):
        u = num / den
        e_u = e_num / np.abs(den) + np.abs(num) * e_den / (den * den) + U * np.abs(u)
        v = rho / H_HORIZON
        e_v = e_rho / H_HORIZON + 5.0 * U * np.abs(v)
    return u, v, e_u, e_v


def fetch(table, u, v, e_u=0.0, e_v=0.0):
    """sky_lut_fetch: normalised coordinates, linear filter, clamp addressing (device_sky.c:46-60) on table [2, h, w, 4]; values [..., 8] and their bound"""
    hgt, wid = table.shape[1], table.shape[2]
    with np.errstate(all="ignore"):
        x, y = u * wid - 0.5, v * hgt - 0.5
        bad = ~np.isfinite(x) | ~np.isfinite(y)
        x, y = np.where(bad, 0.0, x), np.where(bad, 0.0, y)
        fx, fy = np.floor(x), np.floor(y)
        tx, ty = (x - fx)[..., None], (y - fy)[..., None]
        x0, x1 = np.clip(fx, 0, wid - 1).astype(np.int64), np.clip(fx + 1, 0, wid - 1).astype(np.int64)
        y0, y1 = np.clip(fy, 0, hgt - 1).astype(np.int64), np.clip(fy + 1, 0, hgt - 1).astype(np.int64)
        g = lambda yy, xx: np.concatenate([table[0][yy, xx], table[1][yy, xx]], axis=-1)
        a, b, c, d = g(y0, x0), g(y0, x1), g(y1, x0), g(y1, x1)
        top, bot = a + tx * (b - a), c + tx * (d - c)
        val = top + ty * (bot - top)
        e_x = (np.asarray(e_u) * wid + 2.0 * U * (np.abs(u) * wid + 0.5))[..., None]
        e_y = (np.asarray(e_v) * hgt + 2.0 * U * (np.abs(v) * hgt + 0.5))[..., None]
        bound = np.maximum(np.abs(b - a), np.abs(d - c)) * e_x + np.maximum(np.abs(c - a), np.abs(d - b)) * e_y + 6.0 * U * np.maximum(np.maximum(np.abs(a), np.abs(b)), np.maximum(np.abs(c), np.abs(d)))
    return np.where(bad[..., None], np.nan, val), bound


def rgb(spectrum):
    """sky_color_from_spectrum and its bound and scale: eight products of mixed sign"""
    val = np.maximum(spectrum @ RGB_MATRIX.T, 0.0)
    mag = np.abs(spectrum) @ np.abs(RGB_MATRIX.T)
    return val, 10.0 * U * mag, mag


# ---- the geometry of a step ----
def step_geometry(atm, origin, ray, reach):
    pos = origin + ray * reach[..., None]
    e_pos = U * np.abs(ray * reach[..., None]) + U * np.abs(pos)
    plen = np.sqrt(_dot(pos, pos))
    height = plen - R_E
    e_height = 2.5 * U * plen + _adot(e_pos, pos) / np.maximum(plen, TINY)   # the dot product's 3 u halved by the root, and the root's own u
    scatter = _unit(atm.sun_pos - pos)
    e_scatter = 6.0 * U
    cos_angle = _dot(ray, scatter)
    e_cos = (3.0 * U + e_scatter) * np.sqrt(_dot(ray, ray)) + U
    up = pos / plen[..., None]
    zenith_cos = _dot(up, scatter)
    e_zen = 16.0 * U
    shadow = sphere(scatter, pos, 0.0, R_E, e_o=e_pos, e_r=e_scatter)
    return {"pos": pos, "plen": plen, "height": height, "e_height": e_height, "cos_angle": cos_angle, "e_cos": e_cos, "zenith_cos": zenith_cos, "e_zen": e_zen,
            "shadow": np.where(shadow["hit"], 0.0, 1.0), "shadow_decided": shadow["decided"]}


def step_transmittance(atm, height, step_size, hw_exp=0.0):
    m = medium(atm, height, hw_exp)
    y = m["ext"] * step_size[..., None]
    with np.errstate(all="ignore"):
        val = np.exp(-y)
    e = val * (np.abs(y) * (m["rel"][..., None] + 4.0 * U) + np.abs(step_size)[..., None] * m["e_abs"] + 4.0 * U + hw_exp)
    return val, e, m


def step_result(m, ext_sun, ms_tex, step_t, phase_r, phase_m, shadow, light_angle, prev_result, prev_t, use_shadow=True, use_ms=True):
    """one step of the march's recurrence (sky.cuh:398-430) on given words; returns result, transmittance and the result's bound"""
    pts = m["scat_r"] * phase_r[..., None] + (m["scat_m"] * phase_m)[..., None]
    S = ext_sun * pts * ((shadow if use_shadow else 1.0) * light_angle)[..., None]
    if use_ms:
        S = S + ms_tex * m["scat"]
    rel = m["rel"][..., None]
    with np.errstate(all="ignore"):
        om = S - S * step_t
        s_int = om / m["ext"]
        res = prev_result + s_int * prev_t
        e_S = np.abs(S) * (rel + 12.0 * U)
        e_om = e_S * np.abs(1.0 - step_t) + 3.0 * U * np.abs(S)
        e_sint = (e_om + np.abs(s_int) * m["e_abs"]) / m["ext"] + np.abs(s_int) * (rel + 3.0 * U)
        e_res = e_sint * np.abs(prev_t) + 3.0 * U * np.abs(s_int * prev_t) + U * (np.abs(res) + np.abs(prev_result))
    return res, prev_t * step_t, e_res


class Rays:
    """The probe's records: origin (sky space), direction, limit, flags, steps, random_offset, step_random - binary32 values"""
    def __init__(self, origin, direction, limit, flags, steps, random_offset, step_random):
        n = len(origin)
        f32 = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64).astype(np.float32), (n,)).copy()
        self.origin = np.asarray(origin, dtype=np.float64).astype(np.float32).reshape(n, 3)
        self.direction = np.asarray(direction, dtype=np.float64).astype(np.float32).reshape(n, 3)
        self.limit, self.random_offset, self.step_random = f32(np.minimum(limit, FLT_MAX)), f32(random_offset), f32(step_random)
        self.flags = np.broadcast_to(np.asarray(flags, dtype=np.uint32), (n,)).copy()
        self.steps = np.broadcast_to(np.asarray(steps, dtype=np.uint32), (n,)).copy()

    def __len__(self):
        return len(self.origin)

    def words(self):
        w = np.zeros((len(self), RAY_WORDS), dtype=np.uint32)
        w[:, 0:3], w[:, 3:6] = self.origin.view(np.uint32), self.direction.view(np.uint32)
        w[:, 6], w[:, 7], w[:, 8] = self.limit.view(np.uint32), self.flags, self.steps
        w[:, 9], w[:, 10] = self.random_offset.view(np.uint32), self.step_random.view(np.uint32)
        return w


class _Acceptor:
    """the rule every continuous word is held by (the module's docstring): fail and fig are filled word by word"""
    def __init__(self, n, yardstick, factor):
        self.fail, self.fig, self.yardstick, self.factor = {}, {}, yardstick, factor
        self.false, self.nonfinite = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)

    def held(self, name, got, want, where, scale, bound, ulps=None):
        fail, fig, false, yardstick, factor = self.fail, self.fig, self.false, self.yardstick, self.factor
        vec = got.ndim == 2
        red = (lambda a: a.any(axis=-1)) if vec else (lambda a: a)
        ex = (lambda a: np.broadcast_to(a[..., None] if vec and np.ndim(a) == 1 else a, got.shape))
        with np.errstate(all="ignore"):
            scale_a, b = ex(np.asarray(scale, dtype=np.float64)), ex(np.asarray(bound, dtype=np.float64))
            truth_ok = np.isfinite(want) & (np.abs(want) < 3e38) & np.isfinite(b)
            sentinel = (np.abs(want) >= 3e38) & np.isfinite(want)
            fail[name + " is not the truth's FLT_MAX"] = fail.get(name + " is not the truth's FLT_MAX", false) | (where & red(sentinel & (got != want)))
            self.nonfinite |= where & red(truth_ok & ~np.isfinite(got))
            d = np.abs(got - want)
            if ulps is not None:
                key = name + " beyond %g ulp of its inputs" % ulps
                fail[key] = fail.get(key, false) | (where & red(truth_ok & ~(d <= ulps * 2.0 ** -23 * scale_a + TINY)))
                return
            ill = ~(b <= ILL * scale_a)
            well = where[..., None] & truth_ok & ~ill if vec else where & truth_ok & ~ill
            unit = np.maximum(b, ULP4 * scale_a)
            rel = np.where(well, d / np.maximum(scale_a, TINY), 0.0)
            ratio = np.where(well, d / np.maximum(unit, TINY), 0.0)
            key_u = name + " | in units of the thread's bound"
            fig[name] = max(fig.get(name, 0.0), float(np.nanmax(rel)) if rel.size else 0.0)
            fig[key_u] = max(fig.get(key_u, 0.0), float(np.nanmax(ratio)) if ratio.size else 0.0)
            share = name + " | ill-conditioned share"
            cnt = (where[..., None] & truth_ok if vec else where & truth_ok)
            fig[share] = max(fig.get(share, 0.0), float((cnt & ill).sum() / max(int(cnt.sum()), 1)))
            key_i = name + " outside its conditioning bound"
            fail[key_i] = fail.get(key_i, false) | red((where[..., None] if vec else where) & truth_ok & ill & ~(d <= b + TINY))
            key_c = name + " beyond %g x its bound" % CEILING
            fail[key_c] = fail.get(key_c, false) | red(well & ~(d <= CEILING * unit + TINY))
            if yardstick is not None:
                allowed = np.maximum(np.minimum(factor * yardstick.get(name, 0.0) * scale_a, factor * yardstick.get(key_u, 0.0) * unit), unit)
                key = name + " beyond %g x the yardstick" % factor
                fail[key] = fail.get(key, false) | red(well & ~(d <= allowed + TINY))


MUTATIONS = ("pi for 2 pi in the Rayleigh phase", "shadow dropped", "u and v swapped", "ms_tex omitted", "pi for 2 pi in the cap's solid angle", "2 pi for 4 pi in the Mie phase", "HG and Draine weights swapped",
             "sun radius off by 1 %", "reach at i + 0.5 random_offset")


class Truth:
    def __init__(self, atm, rays):
        self.atm, self.rays, self.N = atm, rays, len(rays)
        self.o, self.d = rays.origin.astype(np.float64), rays.direction.astype(np.float64)
        self.limit, self.ro, self.sr = rays.limit.astype(np.float64), rays.random_offset.astype(np.float64), rays.step_random.astype(np.float64)
        self.celestials, self.primary, self.aerial = (rays.flags & CELESTIALS) != 0, (rays.flags & PRIMARY) != 0, (rays.flags & AERIAL) != 0
        self.path = compute_path(self.o, self.d)
        n_aerial, self.steps_decided = step_count(self.limit, self.primary, rays.steps.astype(np.int64), self.sr)
        self.steps = np.where(self.aerial, n_aerial, rays.steps.astype(np.int32).astype(np.int64))
        self.steps_decided = self.steps_decided | ~self.aerial
        self.sun = sphere(self.d, self.o, atm.sun_pos, R_SUN)
        self.earth = sphere(self.d, self.o, 0.0, R_E)
        self.moon = sphere(self.d, self.o, atm.moon_pos, R_MOON)
        self._own_chain()

    def _own_chain(self):
        """the chain on the truth's own values: which decisions are decided, and on which side"""
        N, p = self.N, self.path
        with np.errstate(all="ignore"):
            rest = self.limit - p["start"]
            dist = np.minimum(p["distance"], rest)
        e_rest = p["e_start"] + U * np.abs(rest)
        nowhere = p["start"] == FLT_MAX   # past the shell: FLT_MAX - FLT_MAX = 0 exactly, and 0 > 0 is false in every arithmetic
        marches = (dist > 0.0) & (self.steps > 0)
        shadow_decided = np.ones(N, dtype=bool)
        for i in range(MAX_STEPS):
            on = marches & (self.steps > i)
            with np.errstate(all="ignore"):
                reach = np.where(on, p["start"] + dist * (i + self.ro) / np.maximum(self.steps, 1), 0.0)
            g = step_geometry(self.atm, self.o, self.d, reach)
            shadow_decided &= ~on | g["shadow_decided"]
        cel = self.celestials & ~self.aerial
        self.decisions = {
            "height <= min_height": (p["below"], p["below_decided"]),
            "shell": (p["above"], p["above_decided"]),
            "earth hit": (p["earth"]["t"] < FLT_MAX, p["earth"]["decided"] | p["below"]),
            "path": (dist > 0.0, p["decided"] & (p["below"] | nowhere | ((p["distance"] > p["e_distance"]) & (rest > e_rest)) | (p["distance"] < -p["e_distance"]) | (rest < -e_rest))),
            "step count": (self.steps > 0, self.steps_decided),
            "shadow": (np.ones(N, dtype=bool), shadow_decided),
            "sun rim": (self.sun["t"] < FLT_MAX, self.sun["decided"] | ~cel),
        }
        self.decisive = np.ones(N, dtype=bool)
        for _, dec in self.decisions.values():
            self.decisive &= dec

    def shares(self):
        out = {k: float(1.0 - dec.mean()) for k, (_, dec) in self.decisions.items()}
        out["all"] = float(1.0 - self.decisive.mean())
        return out

    def _star_cells(self):
        """the grid cell of every ray (clamped here to the last cell the generator fills; the reference does not clamp, sky.cuh:486-489), and whether it is decided"""
        with np.errstate(all="ignore"):
            alt = np.arcsin(np.clip(self.d[:, 1], -1.0, 1.0))
            az = np.arctan2(-self.d[:, 2], -self.d[:, 0]) + REF_PI
            cx, cy = az * 10.0, (alt + REF_PI * 0.5) * 10.0
            # asin through atan2(x, sqrt(1 - x^2)): the root carries u / (2 sqrt(1 - x^2)) of its argument's rounding near the poles
            e_c = 10.0 * (16.0 * U * np.pi + 2.0 * U / np.maximum(np.sqrt(np.maximum(1.0 - self.d[:, 1] ** 2, 0.0)), 1e-4))
            cell = np.minimum(np.floor(np.maximum(cx, 0.0)), 63.0) + 64.0 * np.minimum(np.floor(np.maximum(cy, 0.0)), 31.0)
            decided = (np.abs(cx - np.round(cx)) > e_c) & (np.abs(cy - np.round(cy)) > e_c)
        return cell.astype(np.int64), decided

    def _star_sums(self, mask, cells, hw_sincos=0.0):
        """the stars of the given cells: angles_to_direction (math.cuh:781-789), sphere_hit about the star's direction; the sum of the hit stars' intensities"""
        atm, N = self.atm, self.N
        star_sum, e_sum, decided = np.zeros(N), np.zeros(N), np.ones(N, dtype=bool)
        for t in np.nonzero(mask)[0]:
            s = atm.stars[atm.star_offsets[cells[t]]:atm.star_offsets[cells[t] + 1]]
            if len(s):
                pos = np.stack([np.cos(s[:, 1]) * np.cos(s[:, 0]), np.sin(s[:, 0]), np.sin(s[:, 1]) * np.cos(s[:, 0])], axis=-1)
                h = sphere(np.tile(self.d[t], (len(s), 1)), np.zeros((len(s), 3)), pos, s[:, 2], e_o=8.0 * U + 2.0 * hw_sincos)   # a product of two of them per component
                star_sum[t] = (s[:, 3] * atm.stars_intensity * h["hit"]).sum()
                e_sum[t] = 4.0 * U * len(s) * star_sum[t]
                decided[t] = h["decided"].all()
        return star_sum, e_sum, decided

    # ---- an answer made of the truth's own stages, each rounded to binary32 and handed on: what a correct implementation reports, and with `mutation` a wrong one ----
    def synthesize(self, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        N, atm = self.N, self.atm
        out = np.zeros((N, WORDS), dtype=np.uint32)
        def r32(a):
            with np.errstate(over="ignore"):
                return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)
        put = lambda sl, a: out.__setitem__((slice(None), sl), np.asarray(a, dtype=np.float64).astype(np.float32).reshape(N, -1).view(np.uint32))
        p = self.path
        start, pd = r32(p["start"]), r32(p["distance"])
        with np.errstate(all="ignore"):
            dist = r32(np.minimum(pd, r32(self.limit - start)))
        put(slice(0, 1), start); put(slice(1, 2), pd); put(slice(2, 3), dist)
        out[:, 3] = self.steps.astype(np.int32).view(np.uint32)
        marches = dist > 0.0
        two_pi = np.pi if mutation == "pi for 2 pi in the cap's solid angle" else 2.0 * np.pi
        r_sun = R_SUN * (1.01 if mutation == "sun radius off by 1 %" else 1.0)
        la = r32(np.where(marches, sphere_solid_angle(atm.sun_pos, r_sun, self.o, two_pi), 0.0))
        put(slice(4, 5), la)
        result, T = np.zeros((N, 8)), np.tile(SP_IDENT, (N, 1))
        reach_prev = start
        for i in range(MAX_STEPS):
            on = marches & (self.steps > i)
            w0 = HEAD + i * STEP_WORDS
            k = i + (0.5 if mutation == "reach at i + 0.5 random_offset" else 1.0) * self.ro
            with np.errstate(all="ignore"):
                reach = r32(np.where(on, start + dist * k / np.maximum(self.steps, 1), 0.0))
            g = step_geometry(atm, self.o, self.d, reach)
            height, cos_angle, zen = r32(g["height"]), r32(g["cos_angle"]), r32(g["zenith_cos"])
            pr = r32(rayleigh_phase(cos_angle, 8.0 * np.pi if mutation == "pi for 2 pi in the Rayleigh phase" else 16.0 * np.pi))
            pm = r32(mie_phase(atm, cos_angle, swap_weights=mutation == "HG and Draine weights swapped",
                               four_pi=2.0 * np.pi if mutation == "2 pi for 4 pi in the Mie phase" else 4.0 * np.pi)[0])
            u, v, _, _ = transmittance_uv(height, zen)
            u, v = r32(u), r32(v)
            ext_sun = r32(fetch(atm.tm, v, u)[0] if mutation == "u and v swapped" else fetch(atm.tm, u, v)[0])
            ms_tex = r32(fetch(atm.ms, r32(zen * 0.5 + 0.5), r32(height / H_ATMO))[0])
            step_t, _, m = step_transmittance(atm, height, reach - reach_prev)
            step_t = r32(step_t)
            res, Tn, _ = step_result(m, ext_sun, ms_tex, step_t, pr, pm, g["shadow"], la, result, T, use_shadow=mutation != "shadow dropped", use_ms=mutation != "ms_tex omitted")
            res, Tn = r32(res), r32(Tn)
            words = np.concatenate([np.stack([reach, height, cos_angle, zen, u, v, g["shadow"], pr, pm], axis=-1), ext_sun, ms_tex, step_t, res, Tn], axis=-1)
            out[:, w0:w0 + STEP_WORDS] = np.where(on[:, None], words.astype(np.float32).view(np.uint32), 0)
            result, T, reach_prev = np.where(on[:, None], res, result), np.where(on[:, None], Tn, T), np.where(on, reach, reach_prev)
        put(slice(31, 39), T)
        spectrum = r32(result * r32(SUN_RADIANCE * atm.sun_strength)) * marches[:, None]
        cel = self.celestials & ~self.aerial
        sun = sphere(self.d, self.o, atm.sun_pos, r_sun)
        sun_t, earth_t = r32(sun["t"]), r32(self.earth["t"])
        moon_t = r32(self.moon["t"]) if atm.has_moon else np.full(N, FLT_MAX)
        for k, t in ((25, sun_t), (26, earth_t), (27, moon_t)):
            out[:, k] = np.where(cel, t.astype(np.float32).view(np.uint32), 0)
        disk = cel & (earth_t > sun_t) & (moon_t > sun_t)
        spectrum = r32(spectrum + np.where(disk[:, None], T * r32(SUN_RADIANCE * atm.sun_strength), 0.0))
        out[:, 29] = NO_CELL
        stars = cel & atm.has_stars & (sun_t == FLT_MAX) & (earth_t == FLT_MAX) & (moon_t == FLT_MAX)
        if stars.any():
            cell, _ = self._star_cells()
            star_sum = r32(self._star_sums(stars, cell)[0])
            out[:, 29] = np.where(stars, cell, NO_CELL).astype(np.uint32)
            out[:, 30] = np.where(stars, star_sum.astype(np.float32).view(np.uint32), 0)
            spectrum = r32(spectrum + np.where(stars[:, None], T * star_sum[:, None], 0.0))
        put(slice(11, 19), spectrum)
        colour = rgb(spectrum)[0]
        record = RECORD_IN * rgb(T)[0]
        put(slice(19, 22), np.where(self.aerial[:, None], colour * RECORD_IN, colour))
        put(slice(22, 25), np.where(self.aerial[:, None], record, RECORD_IN))
        out[:, 5:11] = out[:, 19:25]
        return out

    # ---- the acceptor ----
    def check(self, out, yardstick=None, factor=4.0, bitwise_walks=True, hw_exp=0.0, hw_sincos=0.0, skip_celestial_shading=True):
        """out [N, 628] uint32. Returns (fail: name -> bool [N], fig: name -> the largest distance over the well-conditioned threads, relative to the word's scale and
        in units of the thread's bound). yardstick: the reference run's figures. hw_exp: the measured relative error of v_exp_f32, hw_sincos: the measured absolute error of v_sin_f32 and v_cos_f32, which angles_to_direction issues for a star's
        direction (fast flavour)."""
        N, atm = self.N, self.atm
        o = np.ascontiguousarray(out, dtype=np.uint32).reshape(N, WORDS)
        fo = _f(o)
        acc = _Acceptor(N, yardstick, factor)
        held, fail, fig, false = acc.held, acc.fail, acc.fig, acc.false

        everyone = np.ones(N, dtype=bool)
        p = self.path
        # ---- the path, from the ray ----
        start, pdist, dist, steps = fo[:, 0], fo[:, 1], fo[:, 2], o[:, 3].astype(np.int32).astype(np.int64)
        scale_o = np.sqrt(_dot(self.o, self.o))
        held("path start", start, p["start"], p["decided"], scale_o, p["e_start"])
        held("path distance", pdist, p["distance"], p["decided"], np.maximum(np.abs(p["distance"]), 1.0), p["e_distance"])
        fail["path of an origin at or below the earth radius"] = p["below"] & p["below_decided"] & ((start != 0.0) | (pdist != -FLT_MAX))
        with np.errstate(all="ignore"):
            want_dist = np.minimum(pdist, (self.limit - start).astype(np.float32).astype(np.float64))
        held("marched distance", dist, want_dist, everyone, np.maximum(np.abs(want_dist), TINY), 0.0, ulps=1)
        fail["step count"] = self.steps_decided & (steps != self.steps)
        marches = dist > 0.0
        la = fo[:, 4]
        want_la = sphere_solid_angle(atm.sun_pos, R_SUN, self.o)
        held("light_angle", la, want_la, marches, want_la, 12.0 * U * want_la)
        fail["light_angle of a ray that does not march"] = ~marches & (o[:, 4] != 0)
        # ---- the steps, each from the answer's words for the stage before ----
        result, T = np.zeros((N, 8)), np.tile(SP_IDENT, (N, 1))
        reach_prev = start
        reached = np.zeros(N, dtype=np.int64)
        for i in range(MAX_STEPS):
            on = marches & (steps > i)
            w = fo[:, HEAD + i * STEP_WORDS:HEAD + (i + 1) * STEP_WORDS]
            fail["words of a step that was not reached"] = fail.get("words of a step that was not reached", false) | (~on & o[:, HEAD + i * STEP_WORDS:HEAD + (i + 1) * STEP_WORDS].any(axis=-1))
            if not on.any():
                continue
            reach, height, cos_angle, zen, u, v, shadow, pr, pm = [w[:, k] for k in range(9)]
            ext_sun, ms_tex, step_t, res, Tn = w[:, 9:17], w[:, 17:25], w[:, 25:33], w[:, 33:41], w[:, 41:49]
            with np.errstate(all="ignore"):
                want_reach = start + dist * (i + self.ro) / np.maximum(steps, 1)
                held("reach", reach, want_reach, on, np.abs(start) + np.abs(dist), 4.0 * U * (np.abs(start) + np.abs(dist) * np.maximum(1.0, (i + self.ro) / np.maximum(steps, 1))))
            g = step_geometry(atm, self.o, self.d, np.where(on, reach, 0.0))
            held("height", height, g["height"], on, g["plen"], g["e_height"])
            held("cos_angle", cos_angle, g["cos_angle"], on, np.maximum(np.sqrt(_dot(self.d, self.d)), 1.0), g["e_cos"])
            held("zenith_cos", zen, g["zenith_cos"], on, 1.0, g["e_zen"])
            fail["shadow"] = fail.get("shadow", false) | (on & (((shadow != 0.0) & (shadow != 1.0)) | (g["shadow_decided"] & (shadow != g["shadow"]))))
            want_pr = rayleigh_phase(cos_angle)
            held("Rayleigh phase", pr, want_pr, on, want_pr, 6.0 * U * want_pr)
            want_pm, e_pm = mie_phase(atm, cos_angle)
            held("Mie phase", pm, want_pm, on, np.abs(want_pm), e_pm)
            wu, wv, e_u, e_v = transmittance_uv(np.where(on, height, 0.0), np.where(on, zen, 0.0))
            held("transmittance u", u, wu, on, 1.0, e_u)
            held("transmittance v", v, wv, on, 1.0, e_v)
            want_es, e_es = fetch(atm.tm, u, v)
            held("extinction_sun", ext_sun, want_es, on, np.maximum(np.abs(want_es).max(axis=-1), 1e-30), e_es)
            want_ms, e_ms = fetch(atm.ms, (zen * 0.5 + 0.5).astype(np.float32).astype(np.float64), (height / H_ATMO).astype(np.float32).astype(np.float64))
            held("ms_tex", ms_tex, want_ms, on, np.maximum(np.abs(want_ms).max(axis=-1), 1e-30), e_ms)
            want_st, e_st, m = step_transmittance(atm, np.where(on, height, 0.0), np.where(on, reach - reach_prev, 0.0), hw_exp)
            held("step_t", step_t, want_st, on, 1.0, e_st)
            want_res, want_T, e_res = step_result(m, ext_sun, ms_tex, step_t, pr, pm, shadow, la, result, T)
            held("result", res, want_res, on, np.maximum(np.abs(want_res).max(axis=-1), 1e-30), e_res)
            held("transmittance", Tn, want_T, on, np.maximum(np.abs(want_T), TINY), 0.0, ulps=1)
            result, T, reach_prev = np.where(on[:, None], res, result), np.where(on[:, None], Tn, T), np.where(on, reach, reach_prev)
            reached += on
        complete = (reached == np.where(marches, np.maximum(steps, 0), 0))   # (a march of more steps than the probe reports cannot be followed to its end)
        held("marched transmittance", fo[:, 31:39], T, complete, np.maximum(np.abs(T), TINY), 0.0, ulps=0)
        # ---- the celestial bodies ----
        cel = self.celestials & ~self.aerial
        sun_t, earth_t, moon_t = fo[:, 25], fo[:, 26], fo[:, 27]
        for name, got, sp in (("sun hit", sun_t, self.sun), ("earth hit", earth_t, self.earth)) + ((("moon hit", moon_t, self.moon),) if atm.has_moon else ()):
            held(name, got, sp["t"], cel & sp["decided"], np.maximum(np.abs(sp["t"]), 1.0), sp["e"])
        if not atm.has_moon:
            fail["moon hit without a moon"] = cel & (moon_t != FLT_MAX)
        fail["celestial words of a ray without celestials"] = ~cel & (o[:, 25:29].any(axis=-1) | (o[:, 29] != NO_CELL) | (o[:, 30] != 0))
        disk = cel & (earth_t > sun_t) & (moon_t > sun_t)
        moon_branch = cel & ~disk & (earth_t > moon_t)
        fail["moon point state"] = np.where(moon_branch, (o[:, 28] != 1) & (o[:, 28] != 2), o[:, 28] != 0)
        with np.errstate(all="ignore"):
            mp = self.o + self.d * np.where(moon_branch, moon_t, 0.0)[:, None]
            lit = sphere(_unit(atm.sun_pos - mp), mp, 0.0, R_E, e_o=2.0 * U * np.abs(mp), e_r=6.0 * U)
        fail["moon point lit"] = moon_branch & lit["decided"] & ((o[:, 28] == 1) != ~lit["hit"])
        stars = cel & atm.has_stars & (sun_t == FLT_MAX) & (earth_t == FLT_MAX) & (moon_t == FLT_MAX)
        cell, cell_decided = self._star_cells()
        fail["star cell"] = np.where(stars, cell_decided & (o[:, 29] != cell), o[:, 29] != NO_CELL)
        star_sum, e_sum, sum_decided = self._star_sums(stars & (o[:, 29] < 64 * 32), o[:, 29].astype(np.int64), hw_sincos)
        held("star sum", fo[:, 30], star_sum, stars & sum_decided, np.maximum(star_sum, 1e-30), e_sum)
        # ---- the end ----
        spectrum = fo[:, 11:19]
        sun_term = T * (SUN_RADIANCE * atm.sun_strength)
        want_sp = result * (SUN_RADIANCE * atm.sun_strength) * marches[:, None] + np.where(disk[:, None], sun_term, 0.0) + np.where(stars[:, None], T * fo[:, 30:31], 0.0)
        shaded = moon_branch & (o[:, 28] == 1) if skip_celestial_shading else false
        held("final spectrum", spectrum, want_sp, complete & ~shaded, np.maximum(np.abs(want_sp).max(axis=-1), 1e-30), 6.0 * U * np.abs(want_sp) + 2.0 * U * np.abs(want_sp).max(axis=-1)[:, None])
        c_val, c_e, c_mag = rgb(spectrum)
        t_val, t_e, t_mag = rgb(fo[:, 31:39])
        held("colour", fo[:, 19:22], np.where(self.aerial[:, None], c_val * RECORD_IN, c_val), everyone, np.maximum(c_mag, 1e-30), c_e + U * c_mag)
        held("record", fo[:, 22:25], np.where(self.aerial[:, None], t_val * RECORD_IN, RECORD_IN), everyone, np.where(self.aerial[:, None], t_mag, 1.0),
             np.where(self.aerial[:, None], t_e + U * t_mag, 0.0))
        if bitwise_walks:
            fail["the second walk is not the real call"] = (o[:, 5:11] != o[:, 19:25]).any(axis=-1) & ~np.isnan(fo[:, 5:11]).any(axis=-1)
        fail["a word is no number"] = acc.nonfinite
        return fail, fig


PANORAMA = 8
ST_CAMERA_DIRECTION, ST_ALLOW_EMISSION = 2, 8   # the path state's bits that let a ray see emitters (csrc/device/dev_trace.h kSt*, oracle ST_*)
PANORAMA_MUTATIONS = ("u and v of the panorama swapped", "the panorama's v not flipped", "the sun's disk added to a ray that may not see emitters")


class Panorama:
    """The panorama lookup (sky_hdri_sample, sky_utils.cuh:49-63, and sky_color_main's HDRI branch, sky.cuh:579-595) on the probe's panorama records: the origin
    is in world space and the steps word is the path state. Stage-wise like Truth: theta and phi from the ray, u and v from the reported angles, the texel's x and y
    from the reported u and v (exact: frac, a product with the dimension, a truncation), the texel's colour from the reported x and y (exact), the sun's table
    coordinates from the origin and the ray, its colour from the reported coordinates, the sum from the reported colours. asin is atan2(y, sqrt(1 - y^2)): a
    ray.y of 1 + ulp gives a negative 1 - y^2, clamped to 0, and phi = pi / 2. The texel is DECIDED where frac(u) dim and frac(v) dim are further from an integer
    than the angles' bounds carry them."""
    def __init__(self, atm, rays, panorama):
        self.atm, self.rays, self.N = atm, rays, len(rays)
        self.o, self.d = rays.origin.astype(np.float64), rays.direction.astype(np.float64)
        self.state = rays.steps.astype(np.int64)
        self.pano = np.asarray(panorama, dtype=np.float32).astype(np.float64)
        self.dim = self.pano.shape[0]
        self.asked = (self.state & (ST_CAMERA_DIRECTION | ST_ALLOW_EMISSION)) != 0
        self.sky_o = self.o * float(np.float32(0.001)) + np.array([0.0, R_E, 0.0]) + atm.geometry_offset   # world_to_sky
        self.e_sky_o = 3.0 * U * (np.abs(self.sky_o) + np.abs(atm.geometry_offset)) + U * np.abs(self.o) * 0.001
        self.disk = sphere(self.d, self.sky_o, atm.sun_pos, R_SUN, e_o=self.e_sky_o)
        self.earth = sphere(self.d, self.sky_o, 0.0, R_E, e_o=self.e_sky_o)
        theta, phi, e_t, e_p = self.angles()
        u, v = (theta + REF_PI) / (2.0 * REF_PI), 1.0 - (phi + 0.5 * REF_PI) / REF_PI
        fx, fy = (u - np.floor(u)) * self.dim, (v - np.floor(v)) * self.dim
        e_x, e_y = (e_t / (2.0 * REF_PI) + 4.0 * U) * self.dim, (e_p / REF_PI + 4.0 * U) * self.dim
        self.texel = (np.floor(fx).astype(np.int64) % self.dim, np.floor(fy).astype(np.int64) % self.dim)
        texel_decided = (np.abs(fx - np.round(fx)) > e_x) & (np.abs(fy - np.round(fy)) > e_y)
        self.decisions = {"texel": (np.ones(self.N, dtype=bool), texel_decided), "sun rim": (self.disk["hit"], self.disk["decided"] | ~self.asked),
                          "earth hit": (self.earth["hit"], self.earth["decided"] | ~self.asked)}
        self.decisive = texel_decided & (self.disk["decided"] | ~self.asked) & (self.earth["decided"] | ~self.asked)

    def shares(self):
        out = {k: float(1.0 - dec.mean()) for k, (_, dec) in self.decisions.items()}
        out["all"] = float(1.0 - self.decisive.mean())
        return out

    def angles(self):
        d = self.d
        with np.errstate(all="ignore"):
            theta = np.arctan2(d[:, 2], d[:, 0])
            root = np.sqrt(np.maximum(1.0 - d[:, 1] ** 2, 0.0))
            phi = np.arctan2(d[:, 1], root)
            # atan2's quotient of the two components carries 2 u, its polynomial a few; the root under asin carries u / root of its argument's rounding
            e_theta = 16.0 * U * np.pi
            e_phi = 16.0 * U * np.pi + np.minimum(2.0 * U / np.maximum(root, TINY), np.sqrt(2.0 * U))
        return theta, phi, np.full(self.N, e_theta), e_phi

    def _texel_of(self, u, v):
        """x and y as binary32 forms them from a binary32 u and v: every operation is exact for a dimension that is a power of two"""
        u32, v32, dim = u.astype(np.float32), v.astype(np.float32), np.float32(self.dim)
        x = ((u32 - np.floor(u32)) * dim).astype(np.int64) % self.dim
        y = ((v32 - np.floor(v32)) * dim).astype(np.int64) % self.dim
        return x, y

    def _sun(self, uv=None):
        atm = self.atm
        plen = np.sqrt(_dot(self.sky_o, self.sky_o))
        zen = _dot(self.sky_o / plen[:, None], self.d)
        if uv is None:
            return transmittance_uv(plen - R_E, zen, 4.0 * U * plen, 8.0 * U)
        ext, e_ext = fetch(atm.tm, uv[0], uv[1])
        k = SP_IDENT * SUN_RADIANCE * atm.sun_strength
        val, e, mag = rgb(ext * k)
        return val, e + np.abs(e_ext * k) @ np.abs(RGB_MATRIX.T) + 4.0 * U * mag, mag

    def synthesize(self, mutation=None):
        assert mutation is None or mutation in PANORAMA_MUTATIONS
        N = self.N
        out = np.zeros((N, WORDS), dtype=np.uint32)
        r32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)
        put = lambda sl, a: out.__setitem__((slice(None), sl), np.asarray(a, dtype=np.float64).astype(np.float32).reshape(N, -1).view(np.uint32))
        theta, phi, _, _ = self.angles()
        theta, phi = r32(theta), r32(phi)
        u = r32((theta + REF_PI) / (2.0 * REF_PI))
        v = r32((phi + 0.5 * REF_PI) / REF_PI) if mutation == "the panorama's v not flipped" else r32(1.0 - (phi + 0.5 * REF_PI) / REF_PI)
        x, y = self._texel_of(v, u) if mutation == "u and v of the panorama swapped" else self._texel_of(u, v)
        texel = self.pano[y, x, :3]
        put(slice(11, 15), np.stack([theta, phi, u, v], axis=-1))
        out[:, 15], out[:, 16] = x, y
        put(slice(31, 34), texel)
        asked = self.asked | (mutation == "the sun's disk added to a ray that may not see emitters")
        put(slice(0, 3), np.where(asked[:, None], self.sky_o, 0.0))
        disk, earth = self.disk["hit"], self.earth["hit"]
        out[:, 25], out[:, 26] = np.where(asked, np.where(disk, 1, 2), 0), np.where(asked, np.where(earth, 1, 2), 0)
        su, sv, _, _ = self._sun()
        su, sv = r32(su), r32(sv)
        sun = r32(self._sun((su, sv))[0])
        add = asked & disk & ~earth
        put(slice(34, 37), np.where(add[:, None], sun, 0.0))
        put(slice(37, 39), np.where(add[:, None], np.stack([su, sv], axis=-1), 0.0))
        put(slice(19, 22), texel + np.where(add[:, None], sun, 0.0))
        put(slice(22, 25), np.tile(RECORD_IN, (N, 1)))
        out[:, 5:11] = out[:, 19:25]
        return out

    def check(self, out, yardstick=None, factor=4.0, bitwise_walks=True, **_):
        N = self.N
        o = np.ascontiguousarray(out, dtype=np.uint32).reshape(N, WORDS)
        fo = _f(o)
        acc = _Acceptor(N, yardstick, factor)
        held, fail, fig = acc.held, acc.fail, acc.fig
        everyone = np.ones(N, dtype=bool)
        theta, phi, e_t, e_p = self.angles()
        held("theta", fo[:, 11], theta, everyone, np.pi, e_t)
        held("phi", fo[:, 12], phi, everyone, np.pi, e_p)
        held("panorama u", fo[:, 13], (fo[:, 11] + REF_PI) / (2.0 * REF_PI), everyone, 1.0, 0.0, ulps=2)
        held("panorama v", fo[:, 14], 1.0 - (fo[:, 12] + 0.5 * REF_PI) / REF_PI, everyone, 1.0, 0.0, ulps=2)
        x, y = self._texel_of(fo[:, 13], fo[:, 14])
        fail["texel x, y of the reported u, v"] = (o[:, 15] != x) | (o[:, 16] != y)
        fail["texel of the truth's own angles"] = self.decisions["texel"][1] & ((o[:, 15] != self.texel[0]) | (o[:, 16] != self.texel[1]))
        inside = (o[:, 15] < self.dim) & (o[:, 16] < self.dim)
        want = self.pano[np.minimum(o[:, 16], self.dim - 1), np.minimum(o[:, 15], self.dim - 1), :3]
        fail["texel colour"] = ~inside | (fo[:, 31:34] != want).any(axis=-1)
        # the sun's disk
        asked = self.asked
        fail["words of a sun that was not asked for"] = ~asked & (o[:, 0:3].any(axis=-1) | o[:, 25:27].any(axis=-1) | o[:, 34:39].any(axis=-1))
        held("origin in sky space", fo[:, 0:3], self.sky_o, asked, np.sqrt(_dot(self.sky_o, self.sky_o)), self.e_sky_o)
        for name, k, sp in (("sun's disk", 25, self.disk), ("earth", 26, self.earth)):
            fail[name] = asked & (((o[:, k] != 1) & (o[:, k] != 2)) | (sp["decided"] & ((o[:, k] == 1) != sp["hit"])))
        add = asked & (o[:, 25] == 1) & (o[:, 26] == 2)
        fail["sun colour of a ray that does not see the disk"] = ~add & o[:, 34:39].any(axis=-1)
        su, sv, e_su, e_sv = self._sun()
        held("sun u", fo[:, 37], su, add, 1.0, e_su)
        held("sun v", fo[:, 38], sv, add, 1.0, e_sv)
        sun, e_sun, mag = self._sun((fo[:, 37], fo[:, 38]))
        held("sun colour", fo[:, 34:37], sun, add, np.maximum(mag, 1e-30), e_sun)
        total = fo[:, 31:34] + np.where(add[:, None], fo[:, 34:37], 0.0)
        held("panorama colour", fo[:, 19:22], total, everyone, np.maximum(np.abs(total), TINY), 0.0, ulps=1)
        if bitwise_walks:
            fail["the second walk is not the real call"] = (o[:, 5:11] != o[:, 19:25]).any(axis=-1)
        acc.nonfinite |= ~np.isfinite(fo[:, 19:22]).all(axis=-1)
        fail["a word is no number"] = acc.nonfinite
        return fail, fig


SUN_WORDS = 64
SHORT_H = 1e-3     # a half vector L + ior V shorter than this (a ray refracted straight through at an ior ratio of 1) has no direction binary32 can hold to 1e-4
E_NDH = 8.0 * U   # N.H of a direction in world space: N, V and H are normalised in binary32 (2 u a component each) and the dot product adds 3 u
RT_SUN_BSDF, RT_SUN_BSDF_METHOD, RT_SUN_RAY, RT_SUN_RESAMPLING = 346, 349, 352, 355   # csrc/device/dev_sky.h kRndSun*, oracle/o_sky.h RT_SUN_*


def sample_hemisphere_basis(altitude, azimuth, basis):
    """math.cuh:277-299: create_basis of `basis`, the direction at `altitude` from it and `azimuth` about it, normalised"""
    sign = np.copysign(1.0, basis[..., 2])
    a = -1.0 / (sign + basis[..., 2])
    b = basis[..., 0] * basis[..., 1] * a
    u1 = np.stack([1.0 + sign * basis[..., 0] ** 2 * a, sign * b, -sign * basis[..., 0]], axis=-1)
    u2 = np.stack([b, sign + basis[..., 1] ** 2 * a, -basis[..., 1]], axis=-1)
    c1, c2, c3 = np.sin(altitude) * np.cos(azimuth), np.sin(altitude) * np.sin(azimuth), np.cos(altitude)
    return _unit(c1[..., None] * u1 + c2[..., None] * u2 + c3[..., None] * basis)


def sample_sphere(p, r, origin, rnd, radius_scale=1.0):
    """math.cuh:1393-1419 from outside the sphere: the direction and the reference's `area` 2 pi a^2 (twice the cap, see sphere_solid_angle)"""
    d = p - origin
    dist = np.sqrt(_dot(d, d))
    r1, r2 = 0.999 * rnd[..., 0], 0.999 * rnd[..., 1]
    angle = np.arcsin(np.clip(r * radius_scale / dist, 0.0, 1.0))
    return sample_hemisphere_basis(np.sqrt(r1) * angle, 2.0 * np.pi * r2, d / dist[..., None]), 2.0 * np.pi * angle * angle


def analyze_direction(mat, nrm, view, L):
    """analyze_direction of dev_bsdf.h in world space (bsdf_truth.evaluate_direction has the same statements): the terms, and whether N.L is clear of the horizon"""
    with np.errstate(all="ignore"):
        ndl_s = _dot(nrm, L)
        isr = ndl_s < 0.0
        hv = L + view * np.where(isr, mat.ior, 1.0)[..., None]
        ln = np.sqrt(_dot(hv, hv))
        H = np.where((ln > 0)[..., None], hv / ln[..., None], view)
        flip = np.where(_dot(nrm, H) < 0.0, -1.0, 1.0)[..., None]
        refr, total, _, _ = bt.refract(view, H, mat.ior)
        f = np.where(isr, bt.fresnel_dielectric(H * flip, view, L, mat.ior), np.where(total, 1.0, bt.fresnel_dielectric(H * flip, view, refr, mat.ior)))
        ndv = np.clip(_dot(nrm, view), 0.0, 1.0)
        c = {"f": np.where(mat.translucent, f, 1.0), "ndh": np.abs(_dot(nrm, H)), "ndl": np.abs(ndl_s), "ndv": ndv, "hdl": np.abs(_dot(H, L)),
             "hdv": np.abs(_dot(H, view)), "isr": isr}
    return c, np.abs(ndl_s) > 2.0 ** -12, ln


SUN_MUTATIONS = ("1 / (pdf Omega) for Omega / (pdf Omega + 1)", "the solid-angle candidate's weight without its MIS term", "the BSDF candidate kept off the disk")


class Sun:
    """The sun's next-event estimation (sample_sun, dev_sky.h; cuda/direct_lighting.cuh:21-119, :352-383, cuda/bsdf.cuh:355-458) on the sun probe's words
    (include/lum_core.h lumc_sun_probe_host), stage-wise like Truth: sky_pos and the two flags from the vertex; the local ray from the reported frame and the
    sampler's numbers; the world direction from the reported quaternion and local ray; the disk from the reported direction and sky_pos; the sun's colour from the
    reported sky_pos and direction; eval_bsdf and sun_bsdf_pdf from the reported directions (the terms in WORLD space, and the world-space view vector handed to the
    bounded-VNDF density as a local one, as bsdf.cuh:438-458 does; the refraction pdf is the reference's, no density, see bsdf_truth.py); the solid-angle candidate
    from the reported sky_pos and the sampler's pair (the reference's 0.999 on both numbers and its 2 pi a^2); the MIS terms Omega / (pdf Omega + 1), the weights,
    their sum, the choice and the light from the reported words before them. Words that contain ggx_d carry D's interval (bsdf_truth.ggx_d) and are ill-conditioned
    at the roughness clamp. The sampler's numbers are the oracle's table of the pixel (integer arithmetic, pinned elsewhere). Decisions with a margin: below the
    horizon (the sphere test of the sun's direction), inside the earth, the BSDF candidate's disk hit, total reflection."""
    def __init__(self, atm, luts, vertices, first_sample, samples):
        import oracle_lib
        self.atm, self.luts, self.vertices, self.samples = atm, luts, vertices, samples
        V = len(vertices)
        self.rows = np.repeat(np.arange(V), samples)
        N = self.N = V * samples
        self.mat = bt.Material(vertices, self.rows)
        self.nrm = _unit(vertices.normal.astype(np.float64))[self.rows]
        self.view = _unit(vertices.V.astype(np.float64))[self.rows]
        pos = vertices.position.astype(np.float64)[self.rows]
        targets = [RT_SUN_BSDF_METHOD, RT_SUN_BSDF, RT_SUN_RAY, RT_SUN_RESAMPLING]
        self.rnd32 = np.stack([oracle_lib.random_2d_table(int(px), int(py), first_sample, samples, targets) for px, py in vertices.pixels]).reshape(N, 4, 2)
        self.sky_o = pos * float(np.float32(0.001)) + np.array([0.0, R_E, 0.0]) + atm.geometry_offset
        self.e_sky_o = 3.0 * U * (np.abs(self.sky_o) + np.abs(atm.geometry_offset)) + U * np.abs(pos) * 0.001
        h = sphere(_unit(atm.sun_pos - self.sky_o), self.sky_o, 0.0, R_E, e_o=self.e_sky_o, e_r=6.0 * U)
        plen = np.sqrt(_dot(self.sky_o, self.sky_o))
        self.below, self.below_decided = h["hit"], h["decided"]
        self.inside, self.inside_decided = plen < R_E, np.abs(plen - R_E) > 4.0 * U * plen + np.abs(self.e_sky_o).sum(axis=-1)
        # the truth's own chain up to the disk
        rnd = self.rnd32.astype(np.float64)
        q, _, _ = bt.rotation_to_z(self.nrm)
        Vl = bt.qapply(q, self.view)
        ray, _, total_decided = self._local_ray(Vl, rnd)
        with np.errstate(all="ignore"):
            d_bsdf = _unit(bt.qapply(bt.qinv(q), ray))
            disk = sphere(np.where(np.isfinite(d_bsdf), d_bsdf, 0.0), self.sky_o, atm.sun_pos, R_SUN, e_o=self.e_sky_o, e_r=16.0 * U)
        seen = ~self.below & ~self.inside
        self.decisions = {"below horizon": (self.below, self.below_decided), "inside earth": (self.inside, self.inside_decided),
                          "disk": (disk["hit"], disk["decided"] | ~seen), "total reflection": (np.ones(N, dtype=bool), total_decided | ~seen)}
        self.decisive = np.ones(N, dtype=bool)
        for _, dec in self.decisions.values():
            self.decisive &= dec

    def shares(self):
        out = {k: float(1.0 - dec.mean()) for k, (_, dec) in self.decisions.items()}
        out["all"] = float(1.0 - self.decisive.mean())
        return out

    def _local_ray(self, Vl, rnd):
        """bsdf_sample_for_sun (bsdf.cuh:380-403): the local ray, the technique and whether total reflection is decided"""
        mat = self.mat
        refl_prob = np.where(mat.translucent, 0.5, 1.0)
        reflection = rnd[:, 0, 0] < refl_prob
        with np.errstate(all="ignore"):
            m1, len1 = bt.sample_vndf_bounded(Vl, mat.roughness, rnd[:, 1])
            r1 = bt.reflect(Vl, m1)
            m2, len2 = bt.sample_vndf_caps(Vl, mat.roughness, rnd[:, 1])
            r2, total, b, eb = bt.refract(Vl, m2, mat.ior)
        ray = np.where(reflection[:, None], r1, r2)
        technique = np.where(reflection, 0, np.where(total, 2, 1))
        self._sample_length = np.where(reflection, len1, len2)   # of the vector the sampler's last normalisation takes: m carries 4 u / length, the ray twice that
        return ray, technique, reflection | (np.abs(b) > eb)

    def sun_colour(self, sky_o, d):
        """sky_get_sun_color (sky_utils.cuh:318-347) without clouds: value, bound, scale"""
        atm = self.atm
        plen = np.sqrt(_dot(sky_o, sky_o))
        zen = _dot(sky_o / plen[:, None], d)
        u, v, e_u, e_v = transmittance_uv(plen - R_E, zen, 4.0 * U * plen, 8.0 * U)
        ext, e_ext = fetch(atm.tm, u, v, e_u, e_v)
        k = SP_IDENT * SUN_RADIANCE * atm.sun_strength
        val, e, mag = rgb(ext * k)
        return val, e + np.abs(e_ext * k) @ np.abs(RGB_MATRIX.T) + 4.0 * U * mag, mag

    def evaluate(self, L):
        """eval_bsdf under the general hint with inv_pdf 1: value, the bound D's interval gives it, and where N.L is clear of the horizon"""
        c, clear, ln = analyze_direction(self.mat, self.nrm, self.view, L)
        energy = bt.energy_terms(self.luts, self.mat, c["ndv"])[:3]
        one = np.ones(self.N)
        with np.errstate(all="ignore"):
            val = bt.eval_layers(self.mat, energy, c, self.view, bt.GENERAL, one)
            # N.H is not a reported word here: it carries the three normalisations and the dot product before it (E_NDH), and D is steep in it at low roughness
            e_ndh = E_NDH + 4.0 * U / np.maximum(ln, TINY)   # (H = (L + ior V) / length carries 2 u / length a component)
            lo = bt.eval_layers(self.mat, energy, dict(c, ndh=np.maximum(c["ndh"] - e_ndh, 0.0)), self.view, bt.GENERAL, one, "lo")
            hi = bt.eval_layers(self.mat, energy, dict(c, ndh=np.minimum(c["ndh"] + e_ndh, 1.0)), self.view, bt.GENERAL, one, "hi")
            # the Fresnel term ((a - b) / (a + b))^2 of two cosines that carry 4 u each: near an ior ratio of 1 it is all cancellation
            root = 8.0 * U / np.maximum(c["hdv"], 1e-3)
            e_f = np.where(self.mat.translucent, 2.0 * np.sqrt(np.clip(c["f"], 0.0, 1.0)) * root + root * root, 0.0)
            f_lo = bt.eval_layers(self.mat, energy, dict(c, f=np.clip(c["f"] - e_f, 0.0, 1.0)), self.view, bt.GENERAL, one)
            f_hi = bt.eval_layers(self.mat, energy, dict(c, f=np.clip(c["f"] + e_f, 0.0, 1.0)), self.view, bt.GENERAL, one)
            rel = 64.0 * U * (1.0 + 1.0 / np.maximum(ln, 1e-3)) + 8.0 * U / np.maximum(c["ndv"], 1e-6)   # (N.V carries 4 u, and the terms divide by it)
            bound = np.maximum(np.abs(lo - val), np.abs(hi - val)) + np.maximum(np.abs(f_lo - val), np.abs(f_hi - val)) + np.abs(val) * rel[:, None]
        return val, np.where(np.isfinite(bound), bound, np.inf), clear & np.isfinite(val).all(axis=-1) & (ln > SHORT_H)

    def bsdf_pdf(self, L):
        """bsdf_sample_for_sun_pdf (bsdf.cuh:438-458): value and bound"""
        mat = self.mat
        c, clear, ln = analyze_direction(mat, self.nrm, self.view, L)
        refl_prob, refr_prob = np.where(mat.translucent, 0.5, 1.0), np.where(mat.translucent, 0.5, 0.0)

        def pdf(ds, shift=0.0):
            ndh = np.clip(c["ndh"] + shift, 0.0, 1.0)
            with np.errstate(all="ignore"):
                return np.where(c["isr"], refr_prob * bt.pdf_refraction(mat.roughness, ndh, c["ndv"], c["hdv"], c["hdl"], mat.ior, ds),
                                refl_prob * bt.pdf_vndf_bounded(self.view, mat.roughness, ndh, c["ndv"], ds))   # (the WORLD-space V, as the reference)
        val = pdf(1)
        with np.errstate(all="ignore"):
            e_ndh = E_NDH + 4.0 * U / np.maximum(ln, TINY)
            bound = np.maximum(np.abs(pdf("lo", -e_ndh) - val), np.abs(pdf("hi", e_ndh) - val)) + np.abs(val) * (64.0 * U * (1.0 + 1.0 / np.maximum(ln, 1e-3)) + 8.0 * U / np.maximum(c["ndv"], 1e-6))
        return val, np.where(np.isfinite(bound), bound, np.inf), clear & np.isfinite(val) & (ln > SHORT_H)

    def mutate(self, out, mutation):
        """the answer `out` with one stage computed wrongly and everything after it computed consistently from it, as a wrong implementation would report"""
        assert mutation in SUN_MUTATIONS
        o = np.array(out, dtype=np.uint32).reshape(self.N, SUN_WORDS)
        f = o.view(np.float32)
        f32 = np.float32
        with np.errstate(all="ignore"):
            seen = o[:, 63] == 1
            omega, pdf_b, pdf_s = f[:, 44], f[:, 51], f[:, 52]
            disk = o[:, 34] == 1
            light_b = np.where(disk[:, None], f[:, 35:38] * f[:, 38:41], f32(0))
            if mutation == "the BSDF candidate kept off the disk":
                light_b = f[:, 35:38] * f[:, 38:41] + np.where(disk[:, None], f32(0), f[:, 45:48] * f32(0.5))
            light_s = f[:, 45:48] * f[:, 48:51]
            if mutation == "1 / (pdf Omega) for Omega / (pdf Omega + 1)":
                mis_b, mis_s = f32(1) / (pdf_b * omega), f32(1) / (pdf_s * omega)
            else:
                mis_b, mis_s = omega / (pdf_b * omega + f32(1)), omega / (pdf_s * omega + f32(1))
            t_b, t_s = light_b.max(axis=-1), light_s.max(axis=-1)
            w_b = t_b * mis_b
            w_s = t_s if mutation == "the solid-angle candidate's weight without its MIS term" else t_s * mis_s
            total = w_b + w_s
            pick_b = f[:, 26] * total < w_b
            live = seen & (total != 0)
            target = np.where(pick_b, t_b, t_s)
            light = np.where(pick_b[:, None], light_b, light_s) * (total / target)[:, None]
            returned = live & (target != 0) & (light.max(axis=-1) != 0)
        for k, a in ((53, mis_b), (54, mis_s), (55, w_b), (56, w_s), (57, total)):
            f[:, k] = np.where(seen, a, f32(0))
        o[:, 58] = np.where(live, np.where(pick_b, 1, 2), 0)
        f[:, 59:62] = np.where(live[:, None], light, f32(0))
        o[:, 62] = returned
        o[:, 0] = returned
        f[:, 1:4] = np.where(returned[:, None], light, f32(0))
        f[:, 4:7] = np.where(returned[:, None], np.where(pick_b[:, None], f[:, 31:34], f[:, 41:44]), f32(0))
        return o

    def check(self, out, yardstick=None, factor=4.0, bitwise_walks=True, hw_sincos=0.0, **_):
        N, mat, atm = self.N, self.mat, self.atm
        o = np.ascontiguousarray(out, dtype=np.uint32).reshape(N, SUN_WORDS)
        fo = _f(o)
        f32w = o.view(np.float32)
        acc = _Acceptor(N, yardstick, factor)
        held, fail, fig = acc.held, acc.fail, acc.fig
        everyone = np.ones(N, dtype=bool)
        sky_o = fo[:, 7:10]
        held("sky_pos", sky_o, self.sky_o, everyone, np.sqrt(_dot(self.sky_o, self.sky_o)), self.e_sky_o)
        fail["below horizon"] = (o[:, 10] > 1) | (self.below_decided & ((o[:, 10] == 1) != self.below))
        fail["inside earth"] = (o[:, 11] > 1) | (self.inside_decided & ((o[:, 11] == 1) != self.inside))
        seen = (o[:, 10] == 0) & (o[:, 11] == 0)
        fail["a vertex that does not see the sun goes on"] = (o[:, 63] == 1) != seen
        fail["words of a vertex that does not see the sun"] = ~seen & (o[:, 21:63].any(axis=-1) | (o[:, 0] != 0))
        refl_prob, refr_prob = np.where(mat.translucent, 0.5, 1.0), np.where(mat.translucent, 0.5, 0.0)
        fail["probabilities"] = (fo[:, 12] != refl_prob) | (fo[:, 13] != refr_prob)
        q, Vl = fo[:, 14:18], fo[:, 18:21]
        with np.errstate(all="ignore"):
            fail["quaternion"] = ~(np.abs(_dot(q, q) - 1.0) <= 8.0 * U) | ~(np.abs(bt.qapply(q, self.nrm) - np.array([0.0, 0.0, 1.0])).max(axis=-1) <= 32.0 * U)
        held("local V", Vl, bt.qapply(q, self.view), everyone, 1.0, 8.0 * U)
        fail["the sampler's numbers"] = seen & (o[:, 21:27] != self.rnd32.reshape(N, 8)[:, [0, 2, 3, 4, 5, 6]].view(np.uint32)).any(axis=-1)
        rnd = self.rnd32.astype(np.float64)
        ray, technique, total_decided = self._local_ray(Vl, rnd)
        e_sample = 32.0 * U + 16.0 * U / np.maximum(self._sample_length, TINY) + 4.0 * hw_sincos
        held("local ray", fo[:, 27:30], ray, seen, 1.0, e_sample)
        with np.errstate(all="ignore"):
            fail["local ray is not a unit vector"] = seen & ~(np.abs(np.sqrt(_dot(fo[:, 27:30], fo[:, 27:30])) - 1.0) <= 16.0 * U)
        fail["technique"] = seen & ((o[:, 30] > 2) | (total_decided & (o[:, 30] != technique)))
        with np.errstate(all="ignore"):
            want_dir = _unit(bt.qapply(bt.qinv(q), fo[:, 27:30]))
        d_bsdf, d_sa = fo[:, 31:34], fo[:, 41:44]
        held("BSDF direction", d_bsdf, want_dir, seen, 1.0, 8.0 * U)
        safe = lambda a: np.where(np.isfinite(a), a, 0.0)
        disk = sphere(safe(d_bsdf), safe(sky_o), atm.sun_pos, R_SUN, e_r=0.0)
        fail["disk"] = seen & (((o[:, 34] != 1) & (o[:, 34] != 2)) | (disk["decided"] & ((o[:, 34] == 1) != disk["hit"])))
        on_disk = seen & (o[:, 34] == 1)
        fail["colour of a BSDF candidate off the disk"] = seen & ~on_disk & o[:, 35:41].any(axis=-1)
        for name, d, k, where in (("BSDF candidate", d_bsdf, 35, on_disk), ("solid-angle candidate", d_sa, 45, seen)):
            c_val, c_e, c_mag = self.sun_colour(safe(sky_o), safe(d))
            held("sun colour, " + name, fo[:, k:k + 3], c_val, where, np.maximum(c_mag, 1e-30), c_e)
            e_val, e_e, clear = self.evaluate(safe(d))
            held("eval_bsdf, " + name, fo[:, k + 3:k + 6], e_val, where & clear, np.maximum(np.abs(e_val).max(axis=-1), 1e-30), e_e)
        want_sa, want_omega = sample_sphere(atm.sun_pos, R_SUN, safe(sky_o), rnd[:, 2])
        held("solid-angle direction", d_sa, want_sa, seen, 1.0, 16.0 * U + 4.0 * hw_sincos)
        held("solid angle", fo[:, 44], want_omega, seen, want_omega, 16.0 * U * want_omega)
        omega = fo[:, 44]
        for name, d, k in (("BSDF candidate", d_bsdf, 51), ("solid-angle candidate", d_sa, 52)):
            p_val, p_e, clear = self.bsdf_pdf(safe(d))
            held("sun_bsdf_pdf, " + name, fo[:, k], p_val, seen & clear, np.maximum(np.abs(p_val), 1e-30), p_e)
            with np.errstate(all="ignore"):
                want_mis = omega / (fo[:, k] * omega + 1.0)
            held("MIS term, " + name, fo[:, k + 2], want_mis, seen, np.maximum(np.abs(want_mis), TINY), 0.0, ulps=4)
        with np.errstate(all="ignore"):
            light_b = np.where(on_disk[:, None], fo[:, 35:38] * fo[:, 38:41], 0.0)
            light_s = fo[:, 45:48] * fo[:, 48:51]
            t_b, t_s = light_b.max(axis=-1), light_s.max(axis=-1)
            held("weight, BSDF candidate", fo[:, 55], t_b * fo[:, 53], seen, np.maximum(np.abs(t_b * fo[:, 53]), TINY), 0.0, ulps=4)
            held("weight, solid-angle candidate", fo[:, 56], t_s * fo[:, 54], seen, np.maximum(np.abs(t_s * fo[:, 54]), TINY), 0.0, ulps=4)
            held("sum of weights", fo[:, 57], fo[:, 55] + fo[:, 56], seen, np.maximum(np.abs(fo[:, 55] + fo[:, 56]), TINY), 0.0, ulps=1)
            total = f32w[:, 57]
            live = seen & (total != 0)
            pick_b = f32w[:, 26] * total < f32w[:, 55]          # the kernel's own comparison, in binary32 on the reported words
            fail["choice"] = np.where(live, o[:, 58] != np.where(pick_b, 1, 2), o[:, 58] != 0)
            target = np.where(pick_b, t_b, t_s)
            want_light = np.where(pick_b[:, None], light_b, light_s) * (fo[:, 57] / target)[:, None]
            held("light", fo[:, 59:62], want_light, live, np.maximum(np.abs(want_light), TINY), 0.0, ulps=6)
            returned = live & (target != 0) & (fo[:, 59:62].max(axis=-1) != 0)
            fail["returned"] = (o[:, 62] == 1) != returned
        if bitwise_walks:
            chosen_dir = np.where((o[:, 58] == 1)[:, None], o[:, 31:34], o[:, 41:44])
            ret = o[:, 62] == 1
            fail["the second walk is not the real call"] = (o[:, 0] != o[:, 62]) | (ret & ((o[:, 1:4] != o[:, 59:62]).any(axis=-1) | (o[:, 4:7] != chosen_dir).any(axis=-1))) | (
                ~ret & o[:, 1:7].any(axis=-1))
        fail["a word is no number"] = acc.nonfinite
        return fail, fig


# ---- the two tables ----
def unit_uv(u, res):
    return (u - 0.5 / res) * (res / (res - 1.0))


def optical_depth(atm, r, mu, end_weight=0.5, steps=2500, e_r=0.0, with_bound=True):
    """sky_compute_transmittance_optical_depth (sky.cuh:110-140): the trapezoid over steps + 1 points; returns depth [8] and its bound (the samples' heights carry
    7e-4 km each: 1.5 ulp of the root's argument at 4e7 and the root's own rounding; the sequential sum of positive terms carries steps u)"""
    disc = r * r * (mu * mu - 1.0) + R_A * R_A
    dist = max(-r * mu + np.sqrt(max(0.0, disc)), 0.0)
    step = dist / steps
    i = np.arange(steps + 1, dtype=np.float64)
    reach = i * step
    h = np.sqrt(reach * reach + 2.0 * r * mu * reach + r * r) - R_E
    w = np.where((i == 0) | (i == steps), end_weight, 1.0) * step
    ext = medium(atm, h)["ext"]
    depth = (ext * w[:, None]).sum(axis=0)
    if not with_bound:
        return depth, None
    e_h = 1.5 * U * (r + reach) ** 2 / R_E + U * R_A + e_r
    dext = np.maximum(np.abs(medium(atm, h + e_h)["ext"] - ext), np.abs(medium(atm, h - e_h)["ext"] - ext))
    e_disc = 4.0 * U * (r * r + R_A * R_A)
    e_dist = 2.0 * U * abs(r * mu) + _e_sqrt(disc, e_disc) + U * dist
    # the weights are dist / steps: the path length's relative error is the depth's
    return depth, (dext * w[:, None]).sum(axis=0) + (steps + 16.0) * U * depth + 2.0 * depth * (min(e_dist / dist, 1.0) if dist > 0.0 else 0.0)


def transmittance_texel(atm, x, y, end_weight=0.5):
    """k_sky_transmittance_lut (sky.cuh:142-176) of texel (x, y): the eight transmittances and their bound, through the texel's (r, mu) as binary32 can form them"""
    fx, fy = unit_uv((x + 0.5) / 256.0, 256.0), unit_uv((y + 0.5) / 64.0, 64.0)
    rho = H_HORIZON * fy
    r = np.sqrt(rho * rho + R_E * R_E)
    e_r = 3.0 * U * r
    d_min, d_max = R_A - r, rho + H_HORIZON
    d = d_min + fx * (d_max - d_min)
    e_d = e_r + 8.0 * U * d_max
    if d == 0.0:
        mu, e_mu = 1.0, 0.0
    else:
        num = H_HORIZON * H_HORIZON - rho * rho - d * d
        mu = num / (2.0 * r * d)
        e_mu = (6.0 * U * H_HORIZON ** 2 + 2.0 * d * e_d) / (2.0 * r * d) + abs(mu) * (e_d / d + 4.0 * U)
    mu_c = min(1.0, max(-1.0, mu))
    depth, bound = optical_depth(atm, r, mu_c, end_weight, e_r=e_r)
    sensitivity = np.zeros(8)   # to mu, which is steep at grazing directions
    for dm in (-e_mu, e_mu):
        other, _ = optical_depth(atm, r, min(1.0, max(-1.0, mu + dm)), end_weight, with_bound=False)
        sensitivity = np.maximum(sensitivity, np.abs(other - depth))
    bound = bound + sensitivity
    T = np.exp(-depth)
    return T, T * (bound + 4.0 * U * (1.0 + depth))


def multiscattering_texel(atm, x, y, offset=0.3, steps=500):
    """k_sky_multiscattering_lut (sky.cuh:186-332, kernels_scene.h:107-135) of texel (x, y) on the binary32 transmittance table atm.tm: 256 directions of 500 steps"""
    fx, fy = unit_uv((x + 0.5) / 32.0, 32.0), unit_uv((y + 0.5) / 32.0, 32.0)
    cos_angle = fx * 2.0 - 1.0
    sun_pos = np.array([0.0, cos_angle, np.sqrt(np.clip(1.0 - cos_angle * cos_angle, 0.0, 1.0))]) * D_SUN
    height = R_E + np.clip(fy + HEIGHT_OFFSET, 0.0, 1.0) * (H_ATMO - HEIGHT_OFFSET)
    pos = np.array([0.0, height, 0.0])
    t = np.arange(256)
    rays = bt.sample_ray_sphere(2.0 * ((t // 16) / 16.0) - 1.0, (t % 16) / 16.0)
    origin = np.tile(pos, (256, 1))
    p = compute_path(origin, rays)
    start, dist = p["start"], p["distance"]
    ok = dist > 0.0
    i = np.arange(steps, dtype=np.float64)
    reach = start[:, None] + np.where(ok, dist, 0.0)[:, None] * (i + offset)[None, :] / steps          # [256, steps]
    step_size = np.diff(np.concatenate([start[:, None], reach], axis=1), axis=1)
    flat = lambda a: a.reshape((-1,) + a.shape[2:])
    O, D = np.repeat(origin, steps, axis=0), np.repeat(rays, steps, axis=0)
    sun_atm = _SunAt(atm, sun_pos)
    g = step_geometry(sun_atm, O, D, flat(reach))
    la = sphere_solid_angle(sun_pos, R_SUN, pos[None, :])[0]
    pr = rayleigh_phase(g["cos_angle"])
    pm, e_pm = mie_phase(atm, g["cos_angle"])
    u, v, e_u, e_v = transmittance_uv(g["height"], g["zenith_cos"], g["e_height"], g["e_zen"])
    ext_sun, e_es = fetch(atm.tm, u, v, e_u, e_v)
    st, e_st, m = step_transmittance(atm, g["height"], flat(step_size))
    pts = m["scat_r"] * pr[:, None] + (m["scat_m"] * pm)[:, None]
    S_lit = ext_sun * pts * la
    S = S_lit * g["shadow"][:, None]
    # what a sample's height, known to e_height, does to the densities: counted once per term, since scattering and extinction move together and
    # (1 - step_t) / extinction moves against them by less than they do
    hi, lo = medium(atm, g["height"] + g["e_height"]), medium(atm, g["height"] - g["e_height"])
    rel = np.maximum(np.maximum(np.abs(hi["ext"] - m["ext"]), np.abs(lo["ext"] - m["ext"])) / m["ext"],
                     np.maximum(np.abs(hi["scat"] - m["scat"]), np.abs(lo["scat"] - m["scat"])) / m["scat"]) + m["rel"][:, None] + 16.0 * U
    one_minus = 1.0 - st
    ss = S * one_minus / m["ext"]
    msi = m["scat"] * one_minus / m["ext"]
    e_om = 6.0 * U   # the exponential's own rounding and the difference's
    e_other = e_es * pts * la * g["shadow"][:, None] + (e_pm * m["scat_m"])[:, None] * ext_sun * la + np.where(g["shadow_decided"], 0.0, 1.0)[:, None] * S_lit
    e_ss = np.abs(ss) * rel + (e_other * one_minus + np.abs(S) * e_om) / m["ext"]
    e_msi = np.abs(msi) * rel + m["scat"] * e_om / m["ext"]
    shape = (256, steps, 8)
    st3, e_st3 = st.reshape(shape), e_st.reshape(shape)
    T_before = np.concatenate([np.ones((256, 1, 8)), np.cumprod(st3, axis=1)[:, :-1]], axis=1)
    rel_T = np.concatenate([np.zeros((256, 1, 8)), np.cumsum(e_st3 / np.maximum(st3, TINY) + U, axis=1)[:, :-1]], axis=1)
    okk = ok[:, None, None]
    L_dir = np.where(okk, ss.reshape(shape) * T_before, 0.0)
    M_dir = np.where(okk, msi.reshape(shape) * T_before, 0.0)
    e_L = np.where(okk, e_ss.reshape(shape) * T_before + np.abs(L_dir) * (rel_T + (steps + 2.0) * U), 0.0).sum(axis=(0, 1)) / 256.0
    e_M = np.where(okk, e_msi.reshape(shape) * T_before + np.abs(M_dir) * (rel_T + (steps + 2.0) * U), 0.0).sum(axis=(0, 1)) / 256.0
    lum, msum = L_dir.sum(axis=(0, 1)) / 256.0, M_dir.sum(axis=(0, 1)) / 256.0
    e_L, e_M = e_L + 10.0 * U * lum, e_M + 10.0 * U * msum
    contribution = 1.0 / (1.0 - msum)
    L = lum * contribution * atm.multiscattering_factor
    bound = (e_L * contribution + lum * e_M * contribution ** 2 + 4.0 * U * lum * contribution) * atm.multiscattering_factor
    return L, bound


class _SunAt:
    """an atmosphere whose sun stands where a multiscattering texel puts it"""
    def __init__(self, atm, sun_pos):
        self.__dict__.update(atm.__dict__)
        self.sun_pos = sun_pos


def check_texels(name, table, truth_fn, texels, yardstick=None, factor=4.0):
    """table [2, h, w, 4] binary32 values; truth_fn(x, y) -> (values [8], bound [8]). Returns (fail: name -> list of offending texels, fig)"""
    fail, fig = {}, {}
    key_u = name + " | in units of the texel's bound"
    for (x, y) in texels:
        want, bound = truth_fn(x, y)
        got = np.concatenate([table[0][y, x], table[1][y, x]]).astype(np.float64)
        scale = max(float(np.abs(want).max()), 1e-30)
        d = np.abs(got - want)
        unit = np.maximum(bound, ULP4 * scale)
        fig[name] = max(fig.get(name, 0.0), float((d / scale).max()))
        fig[key_u] = max(fig.get(key_u, 0.0), float((d / unit).max()))
        if not np.isfinite(got).all():
            fail.setdefault(name + " is no number", []).append((x, y))
        if not (d <= CEILING * unit + TINY).all():
            fail.setdefault(name + " beyond %g x its bound" % CEILING, []).append((x, y))
        if yardstick is not None:
            allowed = np.maximum(np.minimum(factor * yardstick.get(name, 0.0) * scale, factor * yardstick.get(key_u, 0.0) * unit), unit)
            if not (d <= allowed + TINY).all():
                fail.setdefault(name + " beyond %g x the yardstick" % factor, []).append((x, y))
    return fail, fig
