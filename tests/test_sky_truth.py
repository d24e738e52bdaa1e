"""The procedural sky's ray march (csrc/device/dev_sky.h sky_compute_path, sky_compute_atmosphere, sky_get_color, sky_trace_inscattering, through k_sky_probe) and its
two tables against the float64 truth of tests/sky_truth.py, in both flavours.

What is held, per ray and stage by stage on the words the answer itself reports for the stage before: the path through the shell, the marched distance, the step
count, light_angle, and per step reach, height, cos_angle, zenith_cos, u, v, the shadow, the two phases, extinction_sun, ms_tex, step_t, result and transmittance; the
final spectrum, the colour, the dimmed record of aerial perspective; the sun, earth and moon hit distances, whether the moon point is lit, the star cell and the
stars' sum; and that the probe's second walk is the real call's, word for word. Of the tables, chosen texels against the same 2501-point trapezoid and the same
256 x 500 integration in float64.

Families (one to two thousand rays each, run under three atmospheres of test_sky.py: default, no_ozone with mie_diameter 20, dense_high_camera): generic directions
from 106 m; the horizon from 0.5 m, 106 m, 3 km and 50 km at the earth's tangent and 1, 4, 16, 64, 1024 and 4096 units to either side, a unit being the angle that
moves the discriminant by one ulp of R^2 (16 and 1024 are added to the issue's list so that a quarter of the rays is decided on either side); origins below and on
the earth radius, on the shell and an ulp either side, 120 km and 1000 km up looking in, beside the earth and past the shell; the sun's rim at 0 ... 2 disk radii
under four sun altitudes; the march's edges (random_offset 0 and 0.999, 1, 3 and 8 steps, aerial perspective with sky.steps 0, 5, 6 and 40, five limits, primary and
secondary, four step_random, steps astride the density kinks); the forward peak of the largest g_hg the host's fit gives over mie_diameter in (0, 50]; the star grid's
corner cells and a ray at a star; the panorama lookup (sky_hdri_color on a given panorama of 32 x 32 distinct texels) at +-x, +-z, +-y exactly, ray.y = +-(1 + ulp),
the seam at -x from either side, 420 directions and the sun's rim, with and without a state that sees emitters; the moon's centre and rim from five origins, lit and in the earth's shadow. sky.steps 40 with a limit of two base ranges gives 12 steps, the most the probe reports.

The sun's next-event estimation (sample_sun through k_sun_probe, 64 words per (vertex, sample id), sky_truth.Sun) on four families of caller-made vertices: the
bounce truth's materials and views at sun altitudes 0.5 and 0.03; a mirror at the sun (roughness 20 and 51 / 1023, the mirror image at 0, 0.5 and 0.99 disk radii);
the sun at altitude 0, on the vertex's own horizon and 0.2 below it; translucent vertices with the sun in front of, behind and beside the surface.

Tolerances: the oracle's binary32 distance from the truth on the same family is the yardstick of every continuous word (computed here on the CPU, written to
profiles/sky_truth.json under "oracle"); the device may be 4 x that away (floor 4 ulp), the factor and reasoning of tests/test_light_sample_truth.py. Where the bound
the truth propagates is larger, the bound applies. Every answer, the oracle's too, is held to 4 x the thread's bound (16 ulp at least) whatever the yardstick says.
The factor's reasoning does not cover v_exp_f32, v_sin_f32 and v_cos_f32: they are measured alone against float64 (test_the_hardware_instructions_alone), sampled
over the binary32 arguments of [-126, 0] and of [0, 1] revolutions with the maximum doubled, written under "hardware", and v_exp_f32's relative error is a term of the
fast flavour's bound of every word that contains an exp (step_t, result), the larger of the other two a term of the stars' directions (the star sum's hit decisions).

Caps (conditions, not measurements): a family leaves at most 0.10 of its rays undecided; horizon, origins and sun rim, built on an edge, at most 0.50, with a quarter
decided on either side.

CPU tests: known answers of the truth; the oracle's probe alone passes the acceptor within the caps; oracle_sky_color is the probe's colour bit for bit and
oracle_sky_generate_luts' texels pass the texel acceptor; an answer synthesised from the truth's own stages passes and mutated ones are rejected by name.
GPU tests: the exact flavour equals the oracle word for word; both flavours pass the acceptor; fast and exact take the same decision wherever the truth is decisive;
the downloaded tables' texels pass the acceptor; the hardware instructions alone.
"""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest

import oracle_lib
import sky_truth as st
from luminary_amd import SKY_MODE_DEFAULT, SKY_MODE_HDRI, scenes

PROFILE = os.path.join(oracle_lib.ROOT, "profiles", "sky_truth.json")
ATMOSPHERES = ("default", "no_ozone", "dense_high_camera")
FAMILIES = ("generic", "horizon", "origins", "sun rim", "march edges", "stars", "moon", "panorama")
ON_AN_EDGE = {"horizon": "earth hit", "origins": "height <= min_height", "sun rim": "sun rim"}
SUN_ALTITUDES = (0.5, 0.03, 0.0, -0.2)
UP = np.array([0.0, 1.0, 0.0])


# ---- scenes ----
def _host(atmosphere, altitude=None, mie_diameter=None, panorama=False):
    """the example scene under one of test_sky.py's atmospheres (test_sky_variants_match_the_oracle), without clouds"""
    host = scenes.example_scene(32, 18, 2, sphere_segments=6, ground_res=4, num_objects=6, num_lights=4)
    sky = host.get_sky()
    sky.mode = SKY_MODE_DEFAULT
    sky.altitude, sky.azimuth = 0.5, 3.141
    if atmosphere == "no_ozone":
        sky.ozone_absorption = False
        sky.mie_diameter = 20.0
    elif atmosphere == "dense_high_camera":
        sky.base_density, sky.rayleigh_density, sky.mie_density, sky.ground_visibility = 1.5, 1.2, 2.0, 20.0
        sky.geometry_offset.x, sky.geometry_offset.y, sky.geometry_offset.z = 5.0, 3.0, -2.0
        sky.sun_strength, sky.multiscattering_factor, sky.mie_diameter = 2.0, 0.5, 0.5
        sky.altitude, sky.azimuth = 0.15, 1.0
    else:
        assert atmosphere in ("default", "forward peak")
    if mie_diameter is not None:
        sky.mie_diameter = mie_diameter
    if altitude is not None:
        sky.altitude = altitude
    sky.stars_intensity = 50.0
    if panorama:
        sky.mode, sky.hdri_dim, sky.hdri_samples = SKY_MODE_HDRI, PANORAMA_DIM, 2
    host.set_sky(sky)
    return host


PANORAMA_DIM = 32


@functools.lru_cache(maxsize=None)
def panorama():
    """a panorama of distinct texels (so that a wrong texel shows), given to oracle and device alike instead of a bake"""
    rng = np.random.RandomState(11)
    p = (0.1 + 2.0 * rng.rand(PANORAMA_DIM, PANORAMA_DIM, 4)).astype(np.float32)
    p[:, :, 3] = 1.0
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def panorama_view(atmosphere):
    v = oracle_lib.with_sky_hdri(_host(atmosphere, panorama=True).device_scene(), panorama())
    assert v.sky_mode == SKY_MODE_HDRI and not v.cloud_active and v.sky_hdri_dim == PANORAMA_DIM
    return v


@functools.lru_cache(maxsize=None)
def largest_g_hg():
    """the mie_diameter in (0, 50] at which the host's Jendersie-Eon fit gives the largest g_hg, and that g_hg"""
    host = _host("default")
    sky = host.get_sky()
    best = (0.0, 0.0)
    for d in np.concatenate([np.linspace(0.05, 5.0, 12), np.linspace(5.0, 50.0, 28)]):
        sky.mie_diameter = float(d)
        host.set_sky(sky)
        best = max(best, (float(host.device_scene().sky_mie_phase[0]), float(d)))
    return best[1], best[0]


@functools.lru_cache(maxsize=None)
def _tables(atmosphere):
    """the oracle's two tables of an atmosphere; they do not depend on where the scene's sun stands"""
    host = _host(atmosphere, mie_diameter=largest_g_hg()[0] if atmosphere == "forward peak" else None)
    tm, ms = oracle_lib.sky_luts(host.device_scene())
    tm.setflags(write=False)
    ms.setflags(write=False)
    return tm, ms


@functools.lru_cache(maxsize=None)
def view_of(atmosphere, altitude=None):
    host = _host(atmosphere, altitude, mie_diameter=largest_g_hg()[0] if atmosphere == "forward peak" else None)
    v = oracle_lib.with_luts(host.device_scene())
    assert not v.cloud_active
    tm, ms = _tables(atmosphere)
    v.sky_lut_transmittance, v.sky_lut_multiscattering = tm.ctypes.data, ms.ctypes.data
    v._sky_keep = (tm, ms, host)
    return v


def atmosphere_of(atmosphere, altitude=None):
    v = view_of(atmosphere, altitude)
    return st.Atmosphere(v, *_tables(atmosphere))


# ---- rays ----
def _frame(n):
    n = n / np.linalg.norm(n)
    a = np.cross(n, [0.0, 0.0, 1.0] if abs(n[2]) < 0.9 else [1.0, 0.0, 0.0])
    a = a / np.linalg.norm(a)
    return n, a, np.cross(n, a)


def _cone(axis, angle, turns):
    """unit vectors at `angle` from `axis`, one per turn about it"""
    n, a, b = _frame(np.asarray(axis, dtype=np.float64))
    angle, turns = np.asarray(angle, dtype=np.float64)[..., None], np.asarray(turns, dtype=np.float64)[..., None]
    return np.cos(angle) * n + np.sin(angle) * (np.cos(turns) * a + np.sin(turns) * b)


def _sphere_dirs(count, seed):
    rng = np.random.RandomState(seed)
    v = rng.randn(count, 3)
    return v / np.linalg.norm(v, axis=-1)[:, None]


def _rows(rows):
    """rows of (tag, origin, direction, limit, flags, steps, random_offset, step_random)"""
    tags, o, d, limit, flags, steps, ro, sr = zip(*rows)
    return st.Rays(np.array(o), np.array(d), np.array(limit), np.array(flags), np.array(steps), np.array(ro), np.array(sr)), np.asarray(tags)


def _rays(family, atm):
    sky = st.CELESTIALS
    far = st.FLT_MAX
    ground = (st.R_E + 0.106) * UP
    sun_dir = atm.sun_pos / np.linalg.norm(atm.sun_pos)
    rows = []
    if family == "generic":
        dirs = [("zenith", UP), ("nadir", -UP), ("towards the sun", (atm.sun_pos - ground) / np.linalg.norm(atm.sun_pos - ground)), ("opposite the sun", -sun_dir)]
        dirs += [("direction %d" % k, d) for k, d in enumerate(_sphere_dirs(64, 1))]
        for tag, d in dirs:
            for steps in (1, 3, 8):
                for ro in (0.0, 0.125, 0.3, 0.5, 0.75, 0.999):
                    rows.append(("%s, %d steps, offset %g" % (tag, steps, ro), ground, d, far, sky, steps, ro, 0.0))
    elif family == "horizon":
        for h in (0.0005, 0.106, 3.0, 50.0):
            r = st.R_E + h
            tangent = np.arcsin(st.R_E / r)                        # from the nadir
            unit = 4.0 / (2.0 * r * r * np.sin(tangent) * np.cos(tangent))   # the angle that moves r^2 sin^2 by one ulp of R^2 (4 km^2)
            for k in (0, 1, 4, 16, 64, 1024, 4096):
                for side in ((1,) if k == 0 else (1, -1)):
                    for turn in np.arange(24) * (2.0 * np.pi / 24) + 0.1:
                        d = _cone(-UP, tangent + side * k * unit, turn)
                        rows.append(("%g km, tangent %+d units, turn %.2f" % (h, side * k, turn), r * UP, d, far, sky, 4, 0.5, 0.0))
    elif family == "origins":
        tilt = np.array([0.3, 0.9, 0.1]) / np.linalg.norm([0.3, 0.9, 0.1])
        one = lambda x: float(np.spacing(np.float32(x)))
        origins = [("1 km below the radius", 6370.0 * tilt), ("371 km below the radius", 6000.0 * tilt), ("halfway to the centre", 3000.0 * tilt),
                   ("500 m below the radius", 6370.5 * tilt), ("10 m below the radius", 6370.99 * tilt), ("71 km below the radius", 6300.0 * tilt),
                   ("on the radius", st.R_E * UP), ("an ulp above the radius", (st.R_E + one(st.R_E)) * UP), ("an ulp below the shell", (st.R_A - one(st.R_A)) * UP),
                   ("on the shell", st.R_A * UP), ("an ulp above the shell", (st.R_A + one(st.R_A)) * UP), ("120 km up", (st.R_E + 120.0) * tilt), ("1000 km up", (st.R_E + 1000.0) * tilt),
                   # (sixteen origins in all: the five on an edge, and eleven decided ones so that the five stay below half of the family)
                   ("10 m above the radius", (st.R_E + 0.01) * tilt), ("3 km up", (st.R_E + 3.0) * tilt), ("50 km up", (st.R_E + 50.0) * tilt)]
        for tag, o in origins:
            n = o / np.linalg.norm(o)
            r = np.linalg.norm(o)
            dirs = [("in", -n), ("up", n)] + [("random %d" % k, d) for k, d in enumerate(_sphere_dirs(8, 2))]
            for name, rt in (("beside the earth", 0.5 * (st.R_E + st.R_A)), ("grazing the earth", st.R_E + 1.0), ("past the shell", st.R_A + 50.0), ("grazing the shell", st.R_A - 1.0)):
                if r > rt:
                    dirs += [("%s, turn %d" % (name, k), _cone(-n, np.arcsin(rt / r), 0.3 + 2.1 * k)) for k in range(2)]
            for name, d in dirs:
                for ro in (0.0, 0.125, 0.25, 0.5, 0.75, 0.875, 0.999):
                    rows.append(("%s, looking %s, offset %g" % (tag, name, ro), o, d, far, sky, 6, ro, 0.0))
    elif family == "sun rim":
        to_sun = atm.sun_pos - ground
        disk = np.arcsin(st.R_SUN / np.linalg.norm(to_sun))
        for f in (0.0, 0.5, 0.99, 0.9999, 1.0001, 1.01, 2.0):
            for turn in np.arange(16) * (2.0 * np.pi / 16) + 0.05:
                for steps, ro in ((8, 0.5), (3, 0.0), (1, 0.999)):
                    rows.append(("%g radii, turn %.2f, %d steps" % (f, turn, steps), ground, _cone(to_sun, f * disk, turn), far, sky, steps, ro, 0.0))
    elif family == "march edges":
        dirs = [("up", UP), ("level", _cone(UP, np.pi / 2, 0.4)), ("at the sun", sun_dir), ("down", _cone(-UP, 0.5, 1.0))]
        for name, d in dirs + [("direction %d" % k, x) for k, x in enumerate(_sphere_dirs(4, 3))]:
            for ro in (0.0, 0.999):
                for steps in (1, 3, 8):
                    rows.append(("sky, %s, %d steps, offset %g" % (name, steps, ro), ground, d, far, sky, steps, ro, 0.0))
        for name, d in dirs:
            for sky_steps in (0, 5, 6, 40):
                for limit in (1e-4, 0.04, 40.0, 80.0, 1000.0):
                    for primary in (st.PRIMARY, 0):
                        for sr in (0.0, 0.49, 0.5, 0.999):
                            for ro in (0.0, 0.999):
                                rows.append(("aerial, %s, sky.steps %d, limit %g, %s, step_random %g, offset %g" % (name, sky_steps, limit, "primary" if primary else "secondary", sr, ro),
                                             ground, d, limit, st.AERIAL | primary, sky_steps, ro, sr))
        for kink in (2.0, 3.0, 25.0, 25.0 - atm.ozone_layer_thickness, 25.0 + atm.ozone_layer_thickness):
            for span in (1.0, 1e-3):
                for ro in (0.0, 0.5, 0.999):
                    rows.append(("astride %g km within %g km, offset %g" % (kink, span, ro), (st.R_E + kink - 0.5 * span) * UP, UP, span, sky, 8, ro, 0.0))
    elif family == "forward peak":
        for h in (0.106, 3.0, 50.0):
            o = (st.R_E + h) * UP
            to_sun = atm.sun_pos - o
            for off in (0.0, 1e-3, 0.05):
                for turn in np.arange(32) * (2.0 * np.pi / 32) + 0.05:
                    for steps, ro in ((8, 0.5), (8, 0.0), (3, 0.3), (1, 0.999)):
                        rows.append(("%g km, %g off the sun, turn %.2f, %d steps" % (h, off, turn, steps), o, _cone(to_sun, off, turn), far, sky, steps, ro, 0.0))
    elif family == "stars":
        # looking outward from 20 000 km, so that no ray meets the earth; cell (x, y) holds azimuth x / 10 and altitude y / 10 - pi / 2
        def towards(alt, az):
            return np.array([np.cos(az) * np.cos(alt), np.sin(alt), np.sin(az) * np.cos(alt)])
        cells = [("corner cell (%d, %d)" % (x, y), towards((y + 0.5) / 10.0 - st.REF_PI / 2, (x + 0.5) / 10.0 - st.REF_PI)) for x in (0, 63) for y in (0, 31)]
        cells += [("the poles' cell, %s" % k, d) for k, d in (("+y", UP), ("-y", -UP))]
        k = int(np.argmax(atm.stars[:, 3] * (np.abs(atm.stars[:, 0]) < 1.0)))
        cells += [("at star %d" % k, towards(atm.stars[k, 0], atm.stars[k, 1]))]
        cells += [("at star %d" % j, towards(atm.stars[j, 0], atm.stars[j, 1])) for j in range(0, len(atm.stars), 40)]
        cells += [("direction %d" % j, d) for j, d in enumerate(_sphere_dirs(700, 4))]
        for tag, d in cells:
            rows.append((tag, 20000.0 * d, d, far, sky, 2, 0.5, 0.0))
    elif family == "panorama":
        # world-space origins; the steps word is the path state (0: no emitters seen, 2 camera direction, 8 emission allowed)
        eye = np.array([0.0, 6.0, 28.0])
        one = float(np.spacing(np.float32(1.0)))
        axes = [("+x", (1, 0, 0)), ("-x", (-1, 0, 0)), ("+z", (0, 0, 1)), ("-z", (0, 0, -1)), ("+y", (0, 1, 0)), ("-y", (0, -1, 0)), ("ray.y = 1 + ulp", (0, 1.0 + one, 0)),
                ("-x from below", (-1, 0, -1e-30)), ("ray.y = -1 - ulp", (0, -1.0 - one, 0))]
        dirs = axes + [("direction %d" % k, d) for k, d in enumerate(_sphere_dirs(420, 5))]
        to_sun = atm.sun_pos - (eye * 0.001 + np.array([0.0, st.R_E, 0.0]) + atm.geometry_offset)
        disk = np.arcsin(st.R_SUN / np.linalg.norm(to_sun))
        dirs += [("%g radii from the sun's centre, turn %.2f" % (f, t), _cone(to_sun, f * disk, t)) for f in (0.0, 0.5, 0.99, 0.9999, 1.0001, 1.01, 2.0)
                 for t in np.arange(8) * (2.0 * np.pi / 8) + 0.05]
        for tag, d in dirs:
            for state in (0, 2, 8):
                rows.append(("%s, state %d" % (tag, state), eye, d, far, st.PANORAMA, state, 0.0, 0.0))
    elif family == "moon":
        # the moon's centre and rim seen from the ground, from above the shell on the moon's side, and from behind the earth, where the moon point the ray meets lies
        # in the earth's shadow or, near the terminator of that shadow, is lit; two thirds of the rays hit
        for tag, o in (("from the ground", ground), ("from 1000 km up", (st.R_E + 1000.0) * UP), ("from the moon's side", atm.moon_pos / np.linalg.norm(atm.moon_pos) * 7000.0),
                       ("from the sun's side", sun_dir * 7000.0), ("from the night side", -sun_dir * 7000.0)):
            to_moon = atm.moon_pos - o
            disk = np.arcsin(st.R_MOON / np.linalg.norm(to_moon))
            for f in (0.0, 0.3, 0.6, 0.9, 0.99, 0.9999, 1.0001, 1.01, 2.0):
                for turn in np.arange(12) * (2.0 * np.pi / 12) + 0.05:
                    for steps, ro in ((4, 0.5), (2, 0.0)):
                        rows.append(("%s, %g radii, turn %.2f, %d steps" % (tag, f, turn, steps), o, _cone(to_moon, f * disk, turn), far, sky, steps, ro, 0.0))
    else:
        raise KeyError(family)
    return _rows(rows)


class Family:
    def __init__(self, family, atmosphere):
        self.name, self.atmosphere = family, atmosphere
        self.parts = []   # (altitude, Atmosphere, Rays, tags, Truth, oracle words)
        self.views = []
        for altitude in (SUN_ALTITUDES if family == "sun rim" else (None,)):
            view = panorama_view(atmosphere) if family == "panorama" else view_of(atmosphere, altitude)
            atm = st.Atmosphere(view, *_tables(atmosphere))
            rays, tags = _rays(family, atm)
            assert 1 <= len(rays) <= 4000
            oracle = oracle_lib.sky_stages(view, rays.words())
            oracle.setflags(write=False)
            truth = st.Panorama(atm, rays, panorama()) if family == "panorama" else st.Truth(atm, rays)
            self.views.append(view)
            self.parts.append((altitude, atm, rays, tags if altitude is None else np.char.add("sun altitude %g, " % altitude, tags), truth, oracle))
        self.tags = np.concatenate([p[3] for p in self.parts])

    def check(self, outs, **kw):
        """the acceptor over the family's parts: outs one array per part"""
        fails, fig = [], {}
        for (_, _, _, _, truth, _), out in zip(self.parts, outs):
            f, g = truth.check(out, **kw)
            fails.append(f)
            for k, v in g.items():
                fig[k] = max(fig.get(k, 0.0), v)
        keys = sorted(set().union(*fails))
        fail = {k: np.concatenate([f.get(k, np.zeros(p[4].N, dtype=bool)) for f, p in zip(fails, self.parts)]) for k in keys}
        return fail, fig

    def shares(self):
        keys = self.parts[0][4].shares().keys()
        n = sum(p[4].N for p in self.parts)
        return {k: sum(p[4].shares()[k] * p[4].N for p in self.parts) / n for k in keys}

    def decision(self, name):
        value = np.concatenate([p[4].decisions[name][0] for p in self.parts])
        decided = np.concatenate([p[4].decisions[name][1] for p in self.parts])
        return value, decided


@functools.lru_cache(maxsize=None)
def family(name, atmosphere):
    return Family(name, atmosphere)


@functools.lru_cache(maxsize=None)
def yardstick(name, atmosphere):
    fam = family(name, atmosphere)
    return fam.check([p[5] for p in fam.parts])


CASES = [(f, a) for a in ATMOSPHERES for f in FAMILIES] + [("forward peak", "forward peak")]


def _describe(fam, fail, limit=3):
    lines = []
    for name, bad in fail.items():
        if bad.any():
            idx = np.nonzero(bad)[0][:limit]
            lines.append("%s: %d | first at %s" % (name, int(bad.sum()), [str(fam.tags[i]) if len(bad) == len(fam.tags) else int(i) for i in idx]))
    return "\n".join(lines)


def _record(section, name, figures):
    try:
        data = json.load(open(PROFILE))
    except (OSError, ValueError):
        data = {}
    new = {k: float("%.3e" % v) for k, v in sorted(figures.items())}
    if data.get(section, {}).get(name) == new:
        return
    data.setdefault(section, {})[name] = new
    try:
        with open(PROFILE, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


def _groups(fig):
    """the figures that go on record: per word the relative distance and the distance in units of the thread's bound"""
    return {k: v for k, v in fig.items() if "ill-conditioned" not in k or v > 0.0}


def test_the_sky_probes_layout_is_one_layout():
    from luminary_amd.core import Core

    def defines(path, prefix):
        text = open(os.path.join(oracle_lib.ROOT, path)).read()
        return {k: int(v) for k, v in re.findall(r"#define %s_(\w+) (\d+)" % prefix, text)}
    want = {"RAY_WORDS": st.RAY_WORDS, "WORDS": st.WORDS, "HEAD_WORDS": st.HEAD, "STEP_WORDS": st.STEP_WORDS, "MAX_STEPS": st.MAX_STEPS}
    assert defines("include/lum_core.h", "LUMC_SKY_PROBE") == defines("oracle/oracle.h", "ORACLE_SKY_PROBE") == want
    assert (Core.SKY_PROBE_RAY_WORDS, Core.SKY_PROBE_WORDS, Core.SKY_PROBE_HEAD_WORDS, Core.SKY_PROBE_STEP_WORDS, Core.SKY_PROBE_MAX_STEPS) == tuple(want.values())
    assert (oracle_lib.SKY_PROBE_RAY_WORDS, oracle_lib.SKY_PROBE_WORDS, oracle_lib.SKY_PROBE_HEAD_WORDS, oracle_lib.SKY_PROBE_STEP_WORDS, oracle_lib.SKY_PROBE_MAX_STEPS) == tuple(want.values())
    assert st.WORDS == st.HEAD + st.MAX_STEPS * st.STEP_WORDS
    device = os.path.join(oracle_lib.ROOT, "luminary_amd", "csrc", "device")
    # the sky's probes are members of the one probe table, filled by member name in the probe units' header
    decl = open(os.path.join(device, "wavefront_table.h")).read()
    probes = decl[decl.index("struct WavefrontProbes {"):decl.index("};", decl.index("struct WavefrontProbes {"))]
    pointers = re.findall(r"\(\*(\w+)\)\(", "\n".join(line.split("//")[0] for line in probes.splitlines()))
    impl = open(os.path.join(device, "kernels_probe.h")).read()
    body = impl[impl.index("make_probes() {"):impl.index("return p;")]
    assigned = dict(re.findall(r"\bp\.(\w+) = ([^;]+);", body))
    assert pointers[-3:] == ["sky_probe", "sun_probe", "sky_math_probe"] and sorted(assigned) == sorted(pointers) and all(assigned[p] == p for p in pointers)
    # one definition per word count: probe_layout.h, which the kernels and the host layer include; neither states a number of its own
    layout = open(os.path.join(device, "probe_layout.h")).read()
    assert re.search(r"kSkyProbeRayWords = %d, kSkyProbeHeadWords = %d, kSkyProbeStepWords = %d, kSkyProbeMaxSteps = %d;" % (st.RAY_WORDS, st.HEAD, st.STEP_WORDS, st.MAX_STEPS), layout)
    assert re.search(r"kSkyProbeWordsPerThread = kSkyProbeHeadWords \+ kSkyProbeMaxSteps \* kSkyProbeStepWords;", layout) and st.WORDS == st.HEAD + st.MAX_STEPS * st.STEP_WORDS
    assert re.search(r"kSunProbeWordsPerThread = %d;" % st.SUN_WORDS, layout)
    host = open(os.path.join(oracle_lib.ROOT, "luminary_amd", "csrc", "host", "probes.hip")).read()
    for text in (decl, impl, host):
        assert not re.search(r"constexpr[^;\n]*k(Sky|Sun)Probe\w*Words\w* =", text)
    assert '#include "probe_layout.h"' in impl and '#include "../device/probe_layout.h"' in host
    assert "LUMC_SKY_PROBE_WORDS == kSkyProbeWordsPerThread && LUMC_SKY_PROBE_RAY_WORDS == kSkyProbeRayWords" in host
    core_h = open(os.path.join(oracle_lib.ROOT, "include", "lum_core.h")).read()
    enum = re.search(r"LUMC_SKY_PROBE_CELESTIALS = (\d), LUMC_SKY_PROBE_PRIMARY_RAY = (\d), LUMC_SKY_PROBE_AERIAL = (\d)", core_h)
    assert [int(x) for x in enum.groups()] == [st.CELESTIALS, st.PRIMARY, st.AERIAL]


# ---- CPU: known answers of the truth ----
def test_the_sphere_tests_against_closed_forms():
    """From the distance D on the axis: looking at the centre the near hit is D - r and the far one D + r; at the angle a off the axis the chord's near end is
    D cos a - sqrt(r^2 - D^2 sin^2 a), and there is no hit beyond asin(r / D); from inside the one hit is the far end."""
    rng = np.random.RandomState(5)
    D, r = 7000.0 + 500.0 * rng.rand(400), 6371.0
    a = rng.rand(400) * 1.3 * np.arcsin(r / D)
    o = np.stack([0 * D, D, 0 * D], axis=-1)
    d = _cone(-UP, a, rng.rand(400) * 6.28)
    near, far = st.sphere(d, o, 0.0, r), st.sphere(d, o, 0.0, r, back=True)
    inside = a < np.arcsin(r / D)
    root = np.sqrt(np.maximum(r * r - (D * np.sin(a)) ** 2, 0.0))
    assert inside.sum() > 100 and (~inside).sum() > 50
    assert np.abs(near["t"][inside] - (D * np.cos(a) - root)[inside]).max() < 1e-6 and np.abs(far["t"][inside] - (D * np.cos(a) + root)[inside]).max() < 1e-6
    assert (near["t"][~inside] == st.FLT_MAX).all() and (far["t"][~inside] == st.FLT_MAX).all() and np.array_equal(near["hit"], inside)
    # about a centre that is not the origin, and from inside
    c = np.array([1.0e5, -2.0e5, 3.0e5])
    moved = st.sphere(d, o + c, c, r)
    assert np.abs(moved["t"][inside] - near["t"][inside]).max() < 1e-4 and np.array_equal(moved["hit"], inside)
    oi = np.stack([0 * D, 0.5 * r + 0 * D, 0 * D], axis=-1)
    assert np.abs(st.sphere(d, oi, 0.0, r)["t"] - (-0.5 * r * d[:, 1] + np.sqrt(r * r - (0.5 * r) ** 2 * (1.0 - d[:, 1] ** 2)))).max() < 1e-6
    # the bound: the discriminant's at the earth's radius is a few ulp of R^2, about the sun some 1e-4 of its r^2
    g = st.sphere(d, o, 0.0, r)
    assert 4.0 < g["e_disc"].max() < 40.0
    sun = np.array([-1.3e8, 7.2e7, 7.8e4])
    s = st.sphere(_cone(sun, 0.004, rng.rand(400) * 6.28), o, sun, st.R_SUN)
    assert 1e6 < s["e_disc"].max() < 2e8


def _over_the_sphere(fn, g):
    """the integral of fn(cos) over the sphere by Gauss-Legendre panels in s = 1 - cos that widen geometrically away from the forward peak, whose width is (1 - g)^2"""
    x, w = np.polynomial.legendre.leggauss(200)
    edges = [0.0] + [e for e in (1.0 - g) ** 2 * 30.0 ** np.arange(0, 12) if e < 2.0] + [2.0]
    total = 0.0
    for lo, hi in zip(edges[:-1], edges[1:]):
        s = lo + (x + 1.0) * 0.5 * (hi - lo)
        total += 2.0 * np.pi * np.dot(w * 0.5 * (hi - lo), fn(1.0 - s))
    return total


def test_each_phase_function_integrates_to_one_over_the_sphere():
    assert abs(_over_the_sphere(st.rayleigh_phase, 0.0) - 1.0) < 1e-12
    for g in (0.0, 0.5, 0.918, 0.99, largest_g_hg()[1], 0.999):
        total = _over_the_sphere(lambda c: st.hg_phase(c, g)[0], g)
        assert abs(total - 1.0) < 1e-9, (g, total)
    for name in ATMOSPHERES + ("forward peak",):
        a = st.Atmosphere(_host(name, mie_diameter=largest_g_hg()[0] if name == "forward peak" else None).device_scene())
        total = _over_the_sphere(lambda c: st.mie_phase(a, c)[0], a.g_hg)
        assert abs(total - 1.0) < 1e-7, (name, total)   # Jendersie-Eon: (1 - w_d) HG + w_d Draine, each a density
    assert largest_g_hg()[1] > 0.997 and largest_g_hg()[0] == 50.0


def test_the_forward_peaks_conditioning_is_what_the_issue_measured():
    """hg_phase in binary32 against float64 of the same formula, looking at the sun: some 2.5e-4 relative at g = 0.99 and 10 % at g = 0.999 were measured; the bound
    covers both and is not an order of magnitude above them"""
    for g, lo, hi in ((0.99, 1e-5, 1e-2), (0.999, 3e-3, 1.0)):
        g32 = np.float32(g)
        c = np.float32(1.0) - np.float32(2.0 ** -24) * np.arange(0, 64, dtype=np.float32)
        den = np.float32(1.0) + g32 * g32 - np.float32(2.0) * g32 * c
        got = (np.float32(1.0) - g32 * g32) / (np.float32(4.0) * np.float32(np.pi) * (den * np.sqrt(den)))
        want, bound = st.hg_phase(c.astype(np.float64), float(g32))
        rel = np.abs(got.astype(np.float64) - want) / want
        assert (rel <= bound / want).all() and lo < (bound / want).max() < hi, (g, rel.max(), (bound / want).max())


def test_the_trapezoid_against_a_hundred_times_finer_quadrature():
    """the 2501-point trapezoid of the optical depth against 250 001 points of the same integrand in float64: the rule's own error, on record, is far below the
    distance of any binary32 table from it"""
    atm = st.Atmosphere(_host("default").device_scene())
    worst = 0.0
    for r, mu in ((st.R_E, 1.0), (st.R_E, 0.0), (st.R_E + 0.1, 0.02), (st.R_E + 3.0, -0.02), (st.R_E + 50.0, 0.5), (st.R_A - 1.0, -0.1)):
        coarse, _ = st.optical_depth(atm, r, mu, with_bound=False)
        fine, _ = st.optical_depth(atm, r, mu, steps=250000, with_bound=False)
        worst = max(worst, float((np.abs(coarse - fine) / fine).max()))
    _record("known answers", "trapezoid of 2501 points against 250001, relative", {"largest": worst})
    assert worst < 1e-4   # (3.5e-6 on a level ray from the ground, where the Mie profile's kinks at 2 and 3 km cost the rule its second order)
    # ... and end weights of 1 are further away than that
    ones, _ = st.optical_depth(atm, st.R_E, 1.0, end_weight=1.0, with_bound=False)
    coarse, _ = st.optical_depth(atm, st.R_E, 1.0, with_bound=False)
    assert (np.abs(ones - coarse) / coarse > 2e-3).all()


def test_the_caps_exact_solid_angle_beside_the_references_form():
    atm = st.Atmosphere(_host("default").device_scene())
    o = ((st.R_E + 0.106) * UP)[None, :]
    ref, exact = st.sphere_solid_angle(atm.sun_pos, st.R_SUN, o)[0], st.sphere_solid_angle(atm.sun_pos, st.R_SUN, o, exact=True)[0]
    a = np.arcsin(st.R_SUN / np.linalg.norm(atm.sun_pos - o[0]))
    assert abs(ref - 2.0 * np.pi * a * a) < 1e-18 and abs(exact - 2.0 * np.pi * (1.0 - np.cos(a))) < 1e-18
    diff = (ref - exact) / exact
    _record("known answers", "the cap's solid angle, 2 pi a^2 against 2 pi (1 - cos a), relative", {"difference": diff})
    # the reference's form is TWICE the cap: 2 pi (1 - cos a) = pi a^2 (1 - a^2 / 12 ...), so 2 pi a^2 / it - 1 = 1 + a^2 / 6 at a = 4.65 mrad. The sun's
    # single scattering and the moon's light are twice what the radiance and the disk's size give; restated as it is (cuda/math.cuh:1436-1438), not fixed
    assert abs(diff - (1.0 + a * a / 6.0)) < 1e-9 and 1.0 < diff < 1.00001
    assert st.sphere_solid_angle(atm.sun_pos, st.R_SUN, atm.sun_pos[None, :] + 1.0)[0] == 2.0 * np.pi   # inside the sphere, math.cuh:1432


def test_a_path_from_the_ground_ends_on_the_shell_and_one_from_above_skips_the_gap():
    o = np.array([[0.0, st.R_E + 0.106, 0.0], [0.0, st.R_E + 1000.0, 0.0], [0.0, st.R_E + 1000.0, 0.0], [0.0, st.R_E - 1.0, 0.0]])
    d = np.array([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    p = st.compute_path(o, d)
    assert abs(p["distance"][0] - (100.0 - 0.106)) < 1e-9 and p["start"][0] == 0.0
    assert abs(p["start"][1] - 900.0) < 1e-9 and abs(p["distance"][1] - 100.0) < 1e-9
    assert p["start"][2] == st.FLT_MAX and p["distance"][2] == 0.0, "FLT_MAX - FLT_MAX past the shell"
    assert p["start"][3] == 0.0 and p["distance"][3] == -st.FLT_MAX
    assert p["decided"].all()


# ---- CPU: the oracle alone ----
@pytest.mark.parametrize("name,atmosphere", CASES)
def test_the_oracles_probe_passes_the_acceptor_within_the_caps(name, atmosphere):
    fam = family(name, atmosphere)
    fail, fig = yardstick(name, atmosphere)
    shares = fam.shares()
    figures = _groups(fig)
    figures.update({"undecided share | " + k: v for k, v in shares.items()})
    _record("oracle", "%s | %s" % (name, atmosphere), figures)
    print(name, atmosphere, json.dumps({k: float("%.3g" % v) for k, v in figures.items()}, indent=1))
    bad = _describe(fam, fail)
    assert not bad, bad
    cap = 0.50 if name in ON_AN_EDGE else 0.10
    assert shares["all"] <= cap, shares
    if name in ON_AN_EDGE:
        value, decided = fam.decision(ON_AN_EDGE[name])
        assert (value & decided).mean() >= 0.25 and (~value & decided).mean() >= 0.25, ((value & decided).mean(), (~value & decided).mean())


def test_the_older_entry_points_return_what_the_probe_reports():
    """oracle_sky_color is sky_get_color of the same ray with sky.steps steps: the probe's colour of it, bit for bit; the probe is the function the renders call"""
    v = view_of("default")
    atm = atmosphere_of("default")
    dirs = np.concatenate([_sphere_dirs(40, 7), [UP, -UP, atm.sun_pos / np.linalg.norm(atm.sun_pos)]]).astype(np.float32)
    world = np.array([0.0, 6.0, 28.0], dtype=np.float32)
    origin = (world * np.float32(0.001) + np.array([0.0, st.R_E, 0.0], dtype=np.float32)) + np.array(list(v.sky_geometry_offset), dtype=np.float32)   # world_to_sky
    for sun in (1, 0):
        rays = st.Rays(np.tile(origin, (len(dirs), 1)), dirs, st.FLT_MAX, sun * st.CELESTIALS, v.sky_steps, 0.5, 0.0)
        words = oracle_lib.sky_stages(v, rays.words())
        for k, d in enumerate(dirs):
            out = (C.c_float * 3)()
            oracle_lib.lib().oracle_sky_color(C.byref(v), (C.c_float * 3)(*world), (C.c_float * 3)(*[float(x) for x in d]), C.c_int(sun), C.c_float(0.5), out)
            assert np.array_equal(np.array(list(out), dtype=np.float32).view(np.uint32), words[k, 5:8]), (sun, k)
        assert abs(float(origin[1]) - (st.R_E + 0.106)) < 1e-3 and float(origin[1]) != st.R_E + 0.106   # world y = 6 m is 105.96 m in binary32 at this radius


TM_TEXELS = [(0, 0), (255, 0), (0, 63), (255, 63), (128, 0), (128, 63), (0, 32), (255, 32), (1, 0), (254, 0), (1, 63), (254, 63)] + [
    (17 + 14 * k, 3 + (11 * k) % 58) for k in range(16)]
# (columns below 13 have the sun so far below the horizon that the texel is 0 or 1e-13: the interior texels sit between twilight and the zenith)
MS_TEXELS = [(0, 0), (31, 0), (0, 31), (31, 31), (13, 4), (15, 10), (17, 16), (20, 28), (22, 3), (24, 28), (26, 10), (28, 22)]


@functools.lru_cache(maxsize=None)
def table_yardstick(atmosphere):
    atm = atmosphere_of(atmosphere)
    tm, ms = _tables(atmosphere)
    f1, g1 = st.check_texels("transmittance texel", tm.reshape(2, 64, 256, 4), lambda x, y: st.transmittance_texel(atm, x, y), TM_TEXELS)
    f2, g2 = st.check_texels("multiscattering texel", ms.reshape(2, 32, 32, 4), lambda x, y: st.multiscattering_texel(atm, x, y), MS_TEXELS)
    f1.update(f2)
    g1.update(g2)
    return f1, g1


@pytest.mark.parametrize("atmosphere", ATMOSPHERES)
def test_the_oracles_tables_pass_the_texel_acceptor(atmosphere):
    fail, fig = table_yardstick(atmosphere)
    _record("oracle", "tables | %s" % atmosphere, fig)
    print(atmosphere, fig)
    assert not fail, fail


# ---- CPU: mutations ----
def test_a_synthesised_answer_passes_and_mutated_ones_are_rejected_by_name():
    """An answer made of the truth's own stages, each rounded to binary32 and handed to the next, passes; the same with one stage computed wrongly fails, and fails
    in the word that is wrong."""
    fam = family("generic", "default")
    _, atm, rays, tags, truth, _ = fam.parts[0]
    yard = yardstick("generic", "default")[1]
    fail, _ = truth.check(truth.synthesize(), yardstick=yard)
    assert not _describe(fam, fail), _describe(fam, fail)
    sun_fam = family("sun rim", "default")
    expected = {"pi for 2 pi in the Rayleigh phase": "Rayleigh phase", "shadow dropped": "result", "u and v swapped": "extinction_sun", "ms_tex omitted": "result", "pi for 2 pi in the cap's solid angle": "light_angle",
                "2 pi for 4 pi in the Mie phase": "Mie phase", "HG and Draine weights swapped": "Mie phase", "sun radius off by 1 %": ("light_angle", "sun hit"),
                "reach at i + 0.5 random_offset": "reach"}
    assert set(expected) == set(st.MUTATIONS)
    # under a sun 0.2 below the horizon part of every march lies in the earth's shadow: there every mutation shows; with the sun at 0.5 no step is shadowed
    night, night_yard = sun_fam.parts[3][4], yardstick("sun rim", "default")[1]
    assert sun_fam.parts[3][0] == -0.2
    fail, _ = night.check(night.synthesize(), yardstick=night_yard)
    assert not any(bad.any() for bad in fail.values()), [k for k, bad in fail.items() if bad.any()]
    for mutation, word in expected.items():
        for t, y, must in ((night, night_yard, True), (truth, yard, mutation != "shadow dropped")):
            fail, _ = t.check(t.synthesize(mutation), yardstick=y)
            named = [k for k, bad in fail.items() if bad.any()]
            assert bool(named) == must and all(k.startswith(word) for k in named), (mutation, named)   # (startswith takes a tuple too)
    # the sun's radius also moves its rim: rays at 1.0001 and 1.01 radii hit a disk that is 1 % larger
    day = sun_fam.parts[0][4]
    fail, _ = day.check(day.synthesize("sun radius off by 1 %"), yardstick=night_yard)
    assert fail["sun hit is not the truth's FLT_MAX"].sum() >= 16, "the rays between 1 and 1.01 radii"


def test_a_synthesised_panorama_lookup_passes_and_mutated_ones_are_rejected_by_name():
    fam = family("panorama", "default")
    truth, yard = fam.parts[0][4], yardstick("panorama", "default")[1]
    fail, _ = truth.check(truth.synthesize(), yardstick=yard)
    assert not any(bad.any() for bad in fail.values()), [k for k, bad in fail.items() if bad.any()]
    expected = {"u and v of the panorama swapped": "texel", "the panorama's v not flipped": ("panorama v", "texel"),
                "the sun's disk added to a ray that may not see emitters": ("words of a sun that was not asked for", "sun colour of a ray that does not see the disk", "panorama colour")}
    assert set(expected) == set(st.PANORAMA_MUTATIONS)
    for mutation, word in expected.items():
        fail, _ = truth.check(truth.synthesize(mutation), yardstick=yard)
        named = [k for k, bad in fail.items() if bad.any()]
        assert named and all(k.startswith(word) for k in named), (mutation, named)
    # the family reaches what it is for: the pole through the clamp of 1 - y^2, the seam at -x from either side, the sun's disk seen and not seen
    words = fam.parts[0][5]
    tags = fam.tags
    up, over = words[tags == "+y, state 0"][0], words[tags == "ray.y = 1 + ulp, state 0"][0]
    assert np.array_equal(up[11:17], over[11:17]) and up[16] == 0, "ray.y = 1 + ulp looks up the zenith's texel"
    seam = [int(words[tags == k + ", state 0"][0, 15]) for k in ("-x", "-x from below")]
    assert seam == [0, 0] or sorted(seam) == [0, PANORAMA_DIM - 1], seam
    assert (words[:, 34:37].any(axis=-1)).sum() >= 32 and (words[:, 25] == 2).sum() >= 32


def test_mutated_tables_are_rejected_by_name():
    atm = atmosphere_of("default")
    yard = table_yardstick("default")[1]
    some_tm, some_ms = TM_TEXELS[:6] + TM_TEXELS[12:16], [(31, 31), (20, 28), (24, 28), (28, 22)]

    def table_of(fn, texels, shape):
        t = np.zeros(shape)
        for (x, y) in texels:
            v = fn(x, y)[0]
            t[0][y, x], t[1][y, x] = v[:4], v[4:]
        return t.astype(np.float32)
    good = table_of(lambda x, y: st.transmittance_texel(atm, x, y), some_tm, (2, 64, 256, 4))
    assert not st.check_texels("transmittance texel", good, lambda x, y: st.transmittance_texel(atm, x, y), some_tm, yard)[0]
    ones = table_of(lambda x, y: st.transmittance_texel(atm, x, y, end_weight=1.0), some_tm, (2, 64, 256, 4))
    fail = st.check_texels("transmittance texel", ones, lambda x, y: st.transmittance_texel(atm, x, y), some_tm, yard)[0]
    assert fail and all(k.startswith("transmittance texel beyond") for k in fail), fail
    good = table_of(lambda x, y: st.multiscattering_texel(atm, x, y), some_ms, (2, 32, 32, 4))
    assert not st.check_texels("multiscattering texel", good, lambda x, y: st.multiscattering_texel(atm, x, y), some_ms, yard)[0]
    half = table_of(lambda x, y: st.multiscattering_texel(atm, x, y, offset=0.5), some_ms, (2, 32, 32, 4))
    fail = st.check_texels("multiscattering texel", half, lambda x, y: st.multiscattering_texel(atm, x, y), some_ms, yard)[0]
    assert fail and all(k.startswith("multiscattering texel beyond") for k in fail), fail


# ---- the sun's next-event estimation on caller-made vertices ----
SUN_SAMPLES = 24
SUN_FAMILIES = ("sun materials", "sun mirror", "sun horizon", "sun translucent")
NONE = 0xFFFFFFFF


def _sun_vertices(family, atm, altitude):
    import light_truth as lt
    import test_bounce_truth as tb
    eye = np.array([0.0, 6.0, 28.0])
    sky_eye = eye * 0.001 + np.array([0.0, st.R_E, 0.0]) + atm.geometry_offset
    to_sun = atm.sun_pos - sky_eye
    sun_dir = to_sun / np.linalg.norm(to_sun)
    disk = np.arcsin(st.R_SUN / np.linalg.norm(to_sun))
    rows = []   # (tag, normal, view, material)
    if family == "sun materials":
        # the bounce truth's materials and views about a normal that faces the sun halfway, so that the solid-angle candidate is above the surface
        n = sun_dir + np.array([0.3, 0.9, -0.2])
        rows = [("%s, %s" % (mk, vk), n, tb._view(n, c), tb.MATERIALS[mk]) for mk in tb.MATERIALS for vk, c in tb.VIEWS.items()]
    elif family == "sun mirror":
        # reflect(V) is the sun's centre, or a point at 0.5 or 0.99 disk radii: the BSDF candidate hits the disk in a large share of the ids
        for q in (20, 51):
            for mk in ("metallic", "opaque smooth"):
                a, o, _, i, f = tb.MATERIALS[mk]
                for off in (0.0, 0.5, 0.99):
                    for k, v in enumerate((tb._view(sun_dir, 0.8), tb._view(sun_dir, 0.3, turn=2.0), tb._view(sun_dir, -0.2, turn=4.0))):
                        L = _cone(to_sun, off * disk, 1.0 + k)
                        rows.append(("%s at %d/1023, mirror image %g radii off the centre, view %d" % (mk, q, off, k), v + L, v, (a, o, q / 1023, i, f)))
    elif family == "sun horizon":
        n = np.array([0.1, 1.0, 0.05])
        rows = [("%s, %s" % (mk, vk), n, tb._view(n, c), tb.MATERIALS[mk]) for mk in ("opaque rough", "metallic", "glass above", "half") for vk, c in list(tb.VIEWS.items())[:3]]
    elif family == "sun translucent":
        # normals towards and away from the sun: with the sun behind the surface the refraction branch of sun_bsdf_pdf runs
        for q in (153, 307, 818):
            for mk in ("glass above", "glass below", "glass one", "glass zero"):
                a, o, _, i, f = tb.MATERIALS[mk]
                for nk, n in (("towards", sun_dir + np.array([0.2, 0.3, 0.1])), ("away", -sun_dir + np.array([0.2, 0.3, 0.1])), ("sideways", np.cross(sun_dir, [0.3, 0.2, 0.9]) + 0.2 * sun_dir)):
                    for vk, c in (("N.V 0.5", 0.5), ("N.V 0.02", 0.02), ("V = N", 1.0)):
                        rows.append(("%s at %d/1023, normal %s the sun, %s" % (mk, q, nk, vk), n, tb._view(n, c), (a, o, q / 1023, i, f)))
    tags, nrm, view, m = zip(*rows)
    n = len(rows)
    v = lt.Vertices(np.tile(eye, (n, 1)), nrm, view, [x[0] for x in m], [x[1] for x in m], [x[2] for x in m], [x[3] for x in m], [x[4] for x in m],
                    [(NONE, NONE)] * n, [[(3 * k) % 16, (5 * k + 1) % 16] for k in range(n)])
    return v, np.asarray(tags)


def _tangent_altitude():
    """the sun altitude at which the sun's centre lies on the horizon of a vertex 106 m above the radius"""
    return float(-np.arccos(st.R_E / (st.R_E + 0.106)))


class SunFamily:
    def __init__(self, family, atmosphere):
        self.name, self.atmosphere = family, atmosphere
        # the horizon family: the sun's centre on the vertex's own horizon (undecided by construction, a twentieth of the family), at altitude 0 just above it,
        # and 0.2 below it
        altitudes = {"sun materials": (0.5, 0.03), "sun horizon": (0.0, -0.2, _tangent_altitude())}.get(family, (None,))
        self.parts, self.views = [], []
        for altitude in altitudes:
            view = view_of(atmosphere, altitude)
            atm = st.Atmosphere(view, *_tables(atmosphere))
            vertices, tags = _sun_vertices(family, atm, altitude)
            if family == "sun horizon" and altitude == _tangent_altitude():
                keep = np.arange(len(vertices)) < 1
                import light_truth as lt
                vertices = lt.Vertices(vertices.position[keep], vertices.normal[keep], vertices.V[keep], vertices.albedo[keep], vertices.opacity[keep], vertices.roughness[keep],
                                       vertices.ior[keep], vertices.flags[keep], vertices.self_handles[keep], vertices.pixels[keep])
                tags = tags[keep]
            assert len(vertices) * SUN_SAMPLES <= 4000
            truth = st.Sun(atm, oracle_lib.golden_luts(), vertices, 0, SUN_SAMPLES)
            oracle = oracle_lib.sun_stages(view, vertices.words(), 0, SUN_SAMPLES)
            oracle.setflags(write=False)
            t = tags if altitude is None else np.char.add("sun altitude %.4g, " % altitude, tags)
            self.views.append(view)
            self.parts.append((altitude, atm, vertices, t, truth, oracle))
        self.tags = np.concatenate([np.repeat(p[3], SUN_SAMPLES) for p in self.parts])

    check = Family.check
    shares = Family.shares
    decision = Family.decision


@functools.lru_cache(maxsize=None)
def sun_family(name, atmosphere):
    return SunFamily(name, atmosphere)


@functools.lru_cache(maxsize=None)
def sun_yardstick(name, atmosphere):
    fam = sun_family(name, atmosphere)
    return fam.check([p[5] for p in fam.parts])


SUN_CASES = [(f, a) for a in ATMOSPHERES for f in SUN_FAMILIES]


def test_the_sun_probes_layout_is_one_layout():
    from luminary_amd.core import Core
    text = lambda path: open(os.path.join(oracle_lib.ROOT, path)).read()
    assert re.search(r"#define LUMC_SUN_PROBE_WORDS %d\b" % st.SUN_WORDS, text("include/lum_core.h")) and re.search(r"#define ORACLE_SUN_PROBE_WORDS %d\b" % st.SUN_WORDS, text("oracle/oracle.h"))
    assert Core.SUN_PROBE_WORDS == oracle_lib.SUN_PROBE_WORDS == st.SUN_WORDS
    assert re.search(r"kSunProbeWordsPerThread = %d;" % st.SUN_WORDS, text("luminary_amd/csrc/device/probe_layout.h"))
    assert "static_assert(LUMC_SUN_PROBE_WORDS == kSunProbeWordsPerThread" in text("luminary_amd/csrc/host/probes.hip")
    assert "kSunProbeWordsPerThread" in text("luminary_amd/csrc/device/kernels_probe.h") and "kSunProbeWordsPerThread =" not in text("luminary_amd/csrc/device/kernels_probe.h")
    dev = text("luminary_amd/csrc/device/dev_sky.h")
    assert re.search(r"kRndSunBsdf = %d, kRndSunBsdfMethod = %d, kRndSunRay = %d, kRndSunResampling = %d;" % (st.RT_SUN_BSDF, st.RT_SUN_BSDF_METHOD, st.RT_SUN_RAY, st.RT_SUN_RESAMPLING), dev)


def test_the_suns_solid_angle_sample_covers_the_reference_cap_uniformly():
    """sample_sphere (math.cuh:1393-1419): the directions lie within 0.999 asin(r / d) of the centre, and sqrt(r1) makes their density uniform in the small-angle
    disk (the mean squared angle is half the largest); the returned area is the reference's 2 pi a^2, twice the cap."""
    rng = np.random.RandomState(9)
    rnd = rng.rand(20000, 2)
    sun = np.array([-1.3e8, 7.2e7, 7.8e4])
    o = np.tile([0.0, st.R_E + 0.106, 0.0], (20000, 1))
    d, area = st.sample_sphere(sun, st.R_SUN, o, rnd)
    a = np.arcsin(st.R_SUN / np.linalg.norm(sun - o[0]))
    ang = np.arccos(np.clip(d @ ((sun - o[0]) / np.linalg.norm(sun - o[0])), -1.0, 1.0))
    assert ang.max() <= np.sqrt(0.999) * a * (1.0 + 1e-9) and abs((ang ** 2).mean() / (0.999 * a * a) - 0.5) < 0.02
    assert np.abs(area - 2.0 * np.pi * a * a).max() < 1e-18 and np.abs(np.linalg.norm(d, axis=-1) - 1.0).max() < 1e-12


@pytest.mark.parametrize("name,atmosphere", SUN_CASES)
def test_the_oracles_sun_probe_passes_the_acceptor_within_the_caps(name, atmosphere):
    fam = sun_family(name, atmosphere)
    fail, fig = sun_yardstick(name, atmosphere)
    shares = fam.shares()
    figures = _groups(fig)
    figures.update({"undecided share | " + k: v for k, v in shares.items()})
    words = np.concatenate([p[5].reshape(-1, st.SUN_WORDS) for p in fam.parts])
    figures["share of BSDF candidates on the disk"] = float((words[:, 34] == 1).mean())
    figures["share of refracted pdf directions"] = float(np.concatenate([st.analyze_direction(p[4].mat, p[4].nrm, p[4].view, st._f(p[5].reshape(-1, st.SUN_WORDS)[:, 41:44]))[0]["isr"] for p in fam.parts]).mean())
    _record("oracle", "%s | %s" % (name, atmosphere), figures)
    print(name, atmosphere, json.dumps({k: float("%.3g" % v) for k, v in figures.items()}, indent=1))
    bad = _describe(fam, fail)
    assert not bad, bad
    assert shares["all"] <= 0.10, shares
    if name == "sun mirror":
        assert figures["share of BSDF candidates on the disk"] >= 0.25, "the family exists so that the BSDF candidate hits the disk"
    if name == "sun translucent":
        assert figures["share of refracted pdf directions"] >= 0.25, "the refraction branch of sun_bsdf_pdf"
    if name == "sun horizon":
        value, decided = fam.decision("below horizon")
        assert (value & decided).mean() >= 0.25 and (~value & decided).mean() >= 0.25


def test_mutated_sun_answers_are_rejected_by_name():
    fam = sun_family("sun mirror", "default")
    truth, oracle, yard = fam.parts[0][4], fam.parts[0][5], sun_yardstick("sun mirror", "default")[1]
    expected = {"1 / (pdf Omega) for Omega / (pdf Omega + 1)": "MIS term", "the solid-angle candidate's weight without its MIS term": "weight, solid-angle candidate",
                "the BSDF candidate kept off the disk": ("weight, BSDF candidate", "returned")}
    assert set(expected) == set(st.SUN_MUTATIONS)
    for mutation, word in expected.items():
        fail, _ = truth.check(truth.mutate(oracle, mutation), yardstick=yard)
        named = [k for k, bad in fail.items() if bad.any()]
        assert named and all(k.startswith(word) for k in named), (mutation, named)
    # ... and a direction, a pdf and a colour that are off by a part in a thousand, on the materials' family (at the mirror family's roughness clamp the words that
    # contain ggx_d are ill-conditioned and held to D's interval alone)
    fam = sun_family("sun materials", "default")
    truth, oracle, yard = fam.parts[0][4], fam.parts[0][5], sun_yardstick("sun materials", "default")[1]
    for k, word in ((41, "solid-angle direction"), (52, "sun_bsdf_pdf, solid-angle candidate"), (45, "sun colour, solid-angle candidate"), (48, "eval_bsdf, solid-angle candidate")):
        wrong = np.array(oracle, dtype=np.uint32).reshape(-1, st.SUN_WORDS)
        w = wrong.view(np.float32)
        w[:, k] = w[:, k] * np.float32(1.001) + (np.float32(1e-3) if k == 41 else np.float32(0))
        fail, _ = truth.check(wrong, yardstick=yard)
        named = [n for n, bad in fail.items() if bad.any()]
        assert any(n.startswith(word) for n in named), (word, named)


# ---- GPU ----
@functools.lru_cache(maxsize=None)
def hardware_terms():
    """v_exp_f32, v_sin_f32 and v_cos_f32 alone against float64. The binary32 arguments of [-126, 0] are 1.1e9 and those of [0, 1] revolutions 1.07e9: too many to
    exhaust within a test's seconds, so every 509th bit pattern is taken (2.1 million each, every exponent, the ends included) and the maximum doubled."""
    from luminary_amd.core import Core
    core = Core(0)
    try:
        neg = np.arange(int(np.float32(-126.0).view(np.uint32)), int(np.float32(-0.0).view(np.uint32)) - 1, -509, dtype=np.int64).astype(np.uint32)
        x = np.concatenate([neg.view(np.float32), np.float32([-126.0, -0.0, -1.0, -0.5])])
        y = core.sky_math_probe("exp2", x).astype(np.float64)
        want = np.exp2(x.astype(np.float64))
        out = {"v_exp_f32 on [-126, 0], relative": 2.0 * float((np.abs(y - want) / want).max())}
        rev = np.concatenate([np.arange(0, int(np.float32(1.0).view(np.uint32)) + 1, 509, dtype=np.int64).astype(np.uint32).view(np.float32), np.float32([1.0, 0.25, 0.5, 0.75])])
        for op, fn in (("sin", np.sin), ("cos", np.cos)):
            y = core.sky_math_probe(op, rev).astype(np.float64)
            out["v_%s_f32 on [0, 1] revolutions, absolute" % op] = 2.0 * float(np.abs(y - fn(2.0 * np.pi * rev.astype(np.float64))).max())
        out["arguments sampled per instruction"] = float(min(len(x), len(rev)))
        assert len(x) > 2000000 and len(rev) > 2000000
    finally:
        core.close()
    return out


@pytest.mark.gpu
def test_the_hardware_instructions_alone():
    hw = hardware_terms()
    _record("hardware", "MI355X", hw)
    print(hw)
    # what the fast flavour may rest on, from the precision of the format and not from this measurement: an instruction that is not within 4 ulp (exp) or 4 ulp of 1
    # (sin, cos of an argument given in revolutions) is no basis for the 4 x factor at all
    assert hw["v_exp_f32 on [-126, 0], relative"] <= 2.0 * 4.0 * 2.0 ** -23
    assert hw["v_sin_f32 on [0, 1] revolutions, absolute"] <= 2.0 * 4.0 * 2.0 ** -23 and hw["v_cos_f32 on [0, 1] revolutions, absolute"] <= 2.0 * 4.0 * 2.0 ** -23


def _device_words(core, fam, atmosphere):
    outs = []
    for view, (_, _, rays, _, _, _) in zip(fam.views, fam.parts):
        core.upload(view)
        outs.append(core.sky_probe(rays.words()))
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("name,atmosphere", CASES)
def test_both_flavours_against_the_oracle_and_the_truth(name, atmosphere):
    """The exact flavour equals the oracle word for word; both flavours pass the acceptor (the fast one with v_exp_f32's measured error as a term of its bounds);
    fast and exact take the same decision wherever the truth is decisive."""
    from luminary_amd.core import Core
    fam = family(name, atmosphere)
    yard = yardstick(name, atmosphere)[1]
    hw_exp = hardware_terms()["v_exp_f32 on [-126, 0], relative"]
    hw_sincos = max(hardware_terms()["v_%s_f32 on [0, 1] revolutions, absolute" % k] for k in ("sin", "cos"))
    core = Core(0)
    try:
        core.set_flavour("exact")
        exact = _device_words(core, fam, atmosphere)
        core.set_flavour("fast")
        fast = _device_words(core, fam, atmosphere)
    finally:
        core.close()
    for part, words in zip(fam.parts, exact):
        diff = words != part[5]
        assert not diff.any(), "exact flavour against the oracle: %d words differ, first at ray %d word %d (%s)" % (
            diff.sum(), np.nonzero(diff)[0][0], np.nonzero(diff)[1][0], part[3][np.nonzero(diff)[0][0]])
    fail, _ = fam.check(exact, yardstick=yard)
    assert not _describe(fam, fail), "exact:\n" + _describe(fam, fail)
    fail, fig = fam.check(fast, yardstick=yard, hw_exp=hw_exp, hw_sincos=hw_sincos)
    _record("fast", "%s | %s" % (name, atmosphere), _groups(fig))
    print(name, atmosphere, json.dumps({k: float("%.3g" % v) for k, v in _groups(fig).items()}, indent=1))
    assert not _describe(fam, fail), "fast:\n" + _describe(fam, fail)
    # the decisions, where the truth is decisive
    for part, e, f in zip(fam.parts, exact, fast):
        truth = part[4]
        dec = truth.decisive
        assert np.array_equal(e[dec, 3], f[dec, 3]), "step count"
        assert np.array_equal(e[dec, 2].view(np.float32) > 0, f[dec, 2].view(np.float32) > 0), "marches or not"
        for k in (0, 1, 25, 26, 27):
            assert np.array_equal(e[dec, k] == np.float32(st.FLT_MAX).view(np.uint32), f[dec, k] == np.float32(st.FLT_MAX).view(np.uint32)), "hit or no hit, word %d" % k
        assert np.array_equal(e[dec, 28], f[dec, 28]) and np.array_equal(e[dec, 29], f[dec, 29]), "moon point, star cell"
        if isinstance(truth, st.Panorama):
            assert np.array_equal(e[dec][:, [15, 16, 25, 26]], f[dec][:, [15, 16, 25, 26]]), "texel, sun's disk, earth"
        for i in range(st.MAX_STEPS):
            assert np.array_equal(e[dec, st.HEAD + i * st.STEP_WORDS + 6], f[dec, st.HEAD + i * st.STEP_WORDS + 6]), "shadow of step %d" % i


@pytest.mark.gpu
@pytest.mark.parametrize("atmosphere", ATMOSPHERES)
def test_the_devices_tables_pass_the_texel_acceptor(atmosphere):
    """the tables the upload generates (the exact kernels of scene_device.hip, for both flavours), downloaded, at the texels the oracle's were held at"""
    from luminary_amd.core import Core
    host = _host(atmosphere)
    atm = st.Atmosphere(host.device_scene())
    yard = table_yardstick(atmosphere)[1]
    core = Core(0)
    try:
        core.upload(oracle_lib.with_luts(host.device_scene()))   # sky table pointers NULL: generated on the GPU
        tm, ms = core.download_sky_luts()
    finally:
        core.close()
    atm.set_tables(tm, ms)
    f1, g1 = st.check_texels("transmittance texel", tm.reshape(2, 64, 256, 4), lambda x, y: st.transmittance_texel(atm, x, y), TM_TEXELS, yard)
    f2, g2 = st.check_texels("multiscattering texel", ms.reshape(2, 32, 32, 4), lambda x, y: st.multiscattering_texel(atm, x, y), MS_TEXELS, yard)
    g1.update(g2)
    _record("device tables", atmosphere, g1)
    assert not f1 and not f2, (f1, f2)


@pytest.mark.gpu
@pytest.mark.parametrize("name,atmosphere", SUN_CASES)
def test_the_sun_probe_in_both_flavours_against_the_oracle_and_the_truth(name, atmosphere):
    """sample_sun: the exact flavour equals the oracle word for word; both flavours pass the acceptor (the fast one with v_sin_f32's and v_cos_f32's measured error as
    a term of the sampled directions' bounds); fast and exact take the same decision wherever the truth is decisive."""
    from luminary_amd.core import Core
    fam = sun_family(name, atmosphere)
    yard = sun_yardstick(name, atmosphere)[1]
    hw_sincos = max(hardware_terms()["v_%s_f32 on [0, 1] revolutions, absolute" % k] for k in ("sin", "cos"))
    core = Core(0)
    try:
        outs = {}
        for flavour in ("exact", "fast"):
            core.set_flavour(flavour)
            outs[flavour] = []
            for view, part in zip(fam.views, fam.parts):
                core.upload(view)
                outs[flavour].append(core.sun_probe(part[2].words(), 0, SUN_SAMPLES))
    finally:
        core.close()
    for part, words in zip(fam.parts, outs["exact"]):
        diff = words.reshape(-1, st.SUN_WORDS) != part[5].reshape(-1, st.SUN_WORDS)
        assert not diff.any(), "exact flavour against the oracle: %d words differ, first at thread %d word %d" % (diff.sum(), np.nonzero(diff)[0][0], np.nonzero(diff)[1][0])
    fail, _ = fam.check(outs["exact"], yardstick=yard)
    assert not _describe(fam, fail), "exact:\n" + _describe(fam, fail)
    fail, fig = fam.check(outs["fast"], yardstick=yard, hw_sincos=hw_sincos)
    _record("fast", "%s | %s" % (name, atmosphere), _groups(fig))
    print(name, atmosphere, json.dumps({k: float("%.3g" % v) for k, v in _groups(fig).items()}, indent=1))
    assert not _describe(fam, fail), "fast:\n" + _describe(fam, fail)
    for part, e, f in zip(fam.parts, outs["exact"], outs["fast"]):
        dec = part[4].decisive
        e, f = e.reshape(-1, st.SUN_WORDS), f.reshape(-1, st.SUN_WORDS)
        assert np.array_equal(e[dec][:, [10, 11, 30, 34, 63]], f[dec][:, [10, 11, 30, 34, 63]]), "below horizon, inside earth, technique, disk, seen"
