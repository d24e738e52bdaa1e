"""The bounce and the BSDF-driven light direction (csrc/device/dev_bsdf.h sample_bounce, csrc/device/dev_light.h sample_light_direction, through k_bounce_probe)
against the float64 truth of tests/bsdf_truth.py, in both flavours.

What is held, per (vertex, sample id) and stage by stage on the words the answer itself reports for the stage before: the shading frame (quaternion, local V, face
normal), the energy terms, the opacity draw, and per technique the sampled microfacet normal and ray, the six terms and the Fresnel term, the hinted evaluation, the
three pdfs, mis, w, weight_sum, prob and the pick's recurrence, the chosen technique and the final weight; for the light direction the roulette, the sampling
roughness, m, ray, terms, pdf, the weight before and after 1 / rr, the probability and the world ray; and that the probe's second walk is the real call's.

Families (at most 48 sample ids per vertex, one to three thousand threads each): eleven materials (opaque rough and smooth, metallic, translucent with an ior ratio
above 1, below 1 (inside), exactly 1 and quantised to 0, opacity 0.5 with and without coloured transparency, opacity 0 and 254 / 255) under five views (V = N, N.V =
0.5, 0.02, 3e-4, V below the surface); nine roughnesses 20 .. 1023 (/1023: the clamp, 102 and 511 / 512 at the ends of light_dir_rr's ramp); normals +-x, +-y, +z,
-z exactly and just either side of -1 + kEps, and a generic one (and a family of its own on that edge); and views at the critical angle. The issue that asked for these tests names the ior ratio 0.67 for
the critical-angle family; refract's discriminant b = 1 - ior^2 (1 - d^2) is at least 1 - 0.67^2 = 0.55 there, so total reflection and its critical angle exist for
the ratio above 1 only: the family takes both ratios at the views where the ratio above 1 has |b| <= 1e-6 at the mirror normal, and the ratio below 1 is pinned to
never reflect totally.

Tolerances: the oracle's binary32 distance from the truth on the same family is the yardstick of every continuous word (computed here on the CPU, printed, written to
profiles/bounce_truth.json under "oracle"); the device may be 4 x that away (floor 4 ulp), the factor and reasoning of tests/test_light_sample_truth.py: the fast
flavour replaces correctly rounded divisions and roots by 1-ulp ones in at most three chained normalisations, contraction only removes roundings, a factor two is
spare. Where the bound the truth propagates (bsdf_truth.py: ggx_d at low roughness, short vectors, the critical angle) is larger, the bound applies. Every answer, the
oracle's too, is held to a ceiling of 4 x the thread's bound (16 ulp at least) whatever the yardstick says, so an error that oracle and kernel share is not excused.

CPU tests: known answers of the truth; its pdfs integrate to 1; the oracle's probe alone passes the acceptor with the caps on decisive and ill-conditioned shares; the
older oracle_probe_bsdf_sample returns the new probe's head; mutated answers are rejected by name; the layout's statements agree.
GPU tests: the exact flavour equals the oracle word for word; both flavours pass the acceptor; the fast flavour's estimators are unbiased; fast and exact choose the
same technique wherever the truth is decisive.
"""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest

import bsdf_truth as bt
import light_truth as lt
import oracle_lib
from luminary_amd import scenes
from test_oracle_analytic import ProbeMaterial, _f3

SAMPLES = 48
NONE = 0xFFFFFFFF
PROFILE = os.path.join(oracle_lib.ROOT, "profiles", "bounce_truth.json")
ROUGHNESSES = [20, 51, 102, 153, 307, 511, 512, 818, 1023]
#            albedo             opacity      roughness    ior    flags
MATERIALS = {"opaque rough": ((0.8, 0.7, 0.6), 1.0, 818 / 1023, 1.0, 0), "opaque smooth": ((0.9, 0.9, 0.9), 1.0, 153 / 1023, 1.0, 0),
             "metallic": ((0.95, 0.8, 0.5), 1.0, 307 / 1023, 1.0, 4), "glass above": ((0.9, 0.95, 1.0), 1.0, 307 / 1023, 1.5, 1),
             "glass below": ((0.9, 0.95, 1.0), 1.0, 307 / 1023, 0.67, 1 | 2), "glass one": ((0.9, 0.95, 1.0), 1.0, 307 / 1023, 1.0, 1),
             "glass zero": ((0.9, 0.95, 1.0), 1.0, 307 / 1023, 0.0, 1), "half": ((0.8, 0.6, 0.4), 0.5, 307 / 1023, 1.0, 0),
             "half coloured": ((0.8, 0.6, 0.4), 0.5, 307 / 1023, 1.0, 8), "clear": ((0.8, 0.6, 0.4), 0.0, 307 / 1023, 1.0, 8),
             "nearly opaque": ((0.8, 0.6, 0.4), 254 / 255, 307 / 1023, 1.0, 0)}
VIEWS = {"V = N": 1.0, "N.V 0.5": 0.5, "N.V 0.02": 0.02, "N.V 3e-4": 3e-4, "below": -0.3}
GENERIC = (0.3, 0.9, -0.2)


def _view(normal, cos, turn=0.7):
    """a unit vector with N.V = cos (float64; the vertex holds its binary32 rounding)"""
    n = np.asarray(normal, dtype=np.float64)
    n = n / np.linalg.norm(n)
    if cos == 1.0:
        return np.asarray(normal, dtype=np.float64)   # the same binary32 vector: V = N exactly
    a = np.cross(n, [0.0, 0.0, 1.0] if abs(n[2]) < 0.9 else [1.0, 0.0, 0.0])
    a = a / np.linalg.norm(a)
    b = np.cross(n, a)
    t = np.cos(turn) * a + np.sin(turn) * b
    return cos * n + np.sqrt(1.0 - cos * cos) * t


def _families():
    fams = {}

    def make(rows):
        tags, nrm, view, mats = zip(*rows)
        m = [MATERIALS[k] if isinstance(k, str) else k for k in mats]
        n = len(rows)
        v = lt.Vertices(np.zeros((n, 3)), nrm, view, [x[0] for x in m], [x[1] for x in m], [x[2] for x in m], [x[3] for x in m], [x[4] for x in m],
                        [(NONE, NONE)] * n, [[(3 * k) % 16, (5 * k + 1) % 16] for k in range(n)])
        return v, np.asarray(tags)
    fams["materials"] = make([("%s, %s" % (mk, vk), GENERIC, _view(GENERIC, c), mk) for mk in MATERIALS for vk, c in VIEWS.items()])
    for q in ROUGHNESSES:
        rows = []
        for mk in ("opaque rough", "metallic", "glass above", "glass below"):
            a, o, _, i, f = MATERIALS[mk]
            rows += [("%s at %d/1023, %s" % (mk, q, vk), GENERIC, _view(GENERIC, c), (a, o, q / 1023, i, f)) for vk, c in VIEWS.items()]
        fams["roughness %d" % q] = make(rows)
    eps = 2.0 ** -23
    normals = {"+x": (1, 0, 0), "-x": (-1, 0, 0), "+y": (0, 1, 0), "-y": (0, -1, 0), "+z": (0, 0, 1), "-z": (0, 0, -1), "generic": GENERIC, "downward": (0.1, -0.2, -0.97)}
    three = ("opaque smooth", "glass above", "half")
    def tilted(nz, turn):
        s = np.sqrt(1.0 - nz * nz)
        return (s * np.cos(turn), s * np.sin(turn), nz)
    # (one vertex each of a normal just either side of -1 + kEps, undecided by construction: 2 of 50 vertices, the family stays above 0.95)
    near = [("just %s -1 + kEps, glass above, N.V 0.5" % side, n, _view(n, 0.5), "glass above")
            for side, n in (("above", tilted(-1.0 + 3.0 * eps, 2.1)), ("below", tilted(-1.0 + 0.5 * eps, 4.0)))]
    fams["normals"] = make([("%s, %s, N.V %g" % (nk, mk, c), n, _view(n, c), mk) for nk, n in normals.items() for mk in three for c in (0.5, 0.02)] + near)
    # on the edge of rotation_to_z's branch, as the critical-angle family is on refract's: -z itself and 6 kEps above the threshold are decided, a normal between
    # them is not (a component of a normalised vector carries 4 kEps)
    edge = {"-z": (0, 0, -1), "6 kEps above -1 + kEps": tilted(-1.0 + 7.0 * eps, 0.3), "just above -1 + kEps": tilted(-1.0 + 3.0 * eps, 0.0),
            "just below -1 + kEps": tilted(-1.0 + 0.5 * eps, 0.9)}
    fams["normals at -1 + kEps"] = make([("%s, %s, N.V %g" % (nk, mk, c), n, _view(n, c), mk) for nk, n in edge.items() for mk in three for c in (0.5, 0.02)])
    # the critical angle of the mirror normal: b = 1 - ior^2 (1 - d^2) = 0 at d0; |b| <= 1e-6 within 1e-6 / (2 ior^2 d0) of it
    ior = float(np.float32(np.float32(128) * np.float32(1.0 / 255)) * np.float32(3.0))
    d0 = np.sqrt(1.0 - 1.0 / (ior * ior))
    step = 1e-6 / (2.0 * ior * ior * d0)
    rows = []
    for q in (20, 51):
        for nk, n in (("+z", (0, 0, 1)), ("generic", GENERIC)):
            for k in (-1000.0, -0.7, -0.3, 0.0, 0.3, 0.7, 1000.0):
                rows.append(("ratio above 1 at %d/1023, normal %s, d0 %+g steps" % (q, nk, k), n, _view(n, d0 + k * step), ((0.9, 0.95, 1.0), 1.0, q / 1023, 1.5, 1)))
            rows.append(("ratio below 1 at %d/1023, normal %s, d0" % (q, nk), n, _view(n, d0), ((0.9, 0.95, 1.0), 1.0, q / 1023, 0.67, 1 | 2)))
    fams["critical angle"] = make(rows)
    return fams


@functools.lru_cache(maxsize=None)
def _view_with_luts():
    host = scenes.example_scene(32, 18, 2, sphere_segments=6, ground_res=4, num_objects=6, num_lights=6)
    return oracle_lib.with_luts(host.device_scene())


class Family:
    def __init__(self, name, vertices, tags):
        self.name, self.vertices, self.tags = name, vertices, tags
        assert len(vertices) * SAMPLES <= 4000
        self.truth = bt.Truth(oracle_lib.golden_luts(), vertices, 0, SAMPLES)
        self.oracle = oracle_lib.bounce_stages(_view_with_luts(), vertices.words(), 0, SAMPLES)
        self.oracle.setflags(write=False)
        self.rows = self.truth.rows


@functools.lru_cache(maxsize=None)
def families():
    return {k: Family(k, v, t) for k, (v, t) in _families().items()}


FAMILY_NAMES = ["materials"] + ["roughness %d" % q for q in ROUGHNESSES] + ["normals", "normals at -1 + kEps", "critical angle"]
# inputs placed on one decision's edge: that decision is decided on half of the threads at least, every other decision on 0.95 as everywhere
ON_AN_EDGE = {"normals at -1 + kEps": "rotation_to_z's branch", "critical angle": "total_reflection"}


@functools.lru_cache(maxsize=None)
def yardstick(name):
    fam = families()[name]
    return fam.truth.check(fam.oracle)


def _describe(fam, fail, limit=3):
    lines = []
    for name, bad in fail.items():
        if bad.any():
            idx = np.nonzero(bad)[0][:limit]
            lines.append("%s: %d | first at %s" % (name, int(bad.sum()), ["vertex %d (%s) sample %d" % (i // SAMPLES, fam.tags[i // SAMPLES], i % SAMPLES) for i in idx]))
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


def test_the_bounce_probes_layout_is_one_layout():
    """The words per thread and per part, as include/lum_core.h, oracle/oracle.h, probe_layout.h, luminary_amd/core.py, tests/oracle_lib.py and the
    truth state them."""
    from luminary_amd.core import Core

    def defines(path, prefix):
        text = open(os.path.join(oracle_lib.ROOT, path)).read()
        return {k: int(v) for k, v in re.findall(r"#define %s_(\w+) (\d+)" % prefix, text)}
    want = {"WORDS": bt.WORDS, "HEAD_WORDS": bt.HEAD, "TECH_WORDS": bt.TECH_WORDS, "LIGHT_DIR_WORDS": bt.LD_WORDS}
    assert defines("include/lum_core.h", "LUMC_BOUNCE_PROBE") == defines("oracle/oracle.h", "ORACLE_BOUNCE_PROBE") == want
    assert (Core.BOUNCE_PROBE_WORDS, Core.BOUNCE_PROBE_HEAD_WORDS, Core.BOUNCE_PROBE_TECH_WORDS, Core.BOUNCE_PROBE_LIGHT_DIR_WORDS) == tuple(want.values())
    assert (oracle_lib.BOUNCE_PROBE_WORDS, oracle_lib.BOUNCE_PROBE_HEAD_WORDS, oracle_lib.BOUNCE_PROBE_TECH_WORDS, oracle_lib.BOUNCE_PROBE_LIGHT_DIR_WORDS) == tuple(want.values())
    assert bt.WORDS == bt.HEAD + 3 * bt.TECH_WORDS + bt.LD_WORDS and bt.LD0 == bt.HEAD + 3 * bt.TECH_WORDS
    device = os.path.join(oracle_lib.ROOT, "luminary_amd", "csrc", "device")
    layout = open(os.path.join(device, "probe_layout.h")).read()  # the one definition: the kernels (kernels_probe.h) and the host layer (probes.hip) include it
    assert re.search(r"kBounceProbeHeadWords = %d, kBounceProbeTechWords = %d, kBounceProbeLightDirWords = %d;" % (bt.HEAD, bt.TECH_WORDS, bt.LD_WORDS), layout)
    assert re.search(r"kBounceProbeWordsPerThread = kBounceProbeHeadWords \+ 3 \* kBounceProbeTechWords \+ kBounceProbeLightDirWords;", layout)
    host = open(os.path.join(oracle_lib.ROOT, "luminary_amd", "csrc", "host", "probes.hip")).read()
    assert "static_assert(LUMC_BOUNCE_PROBE_WORDS == kBounceProbeWordsPerThread" in host  # lum_core.h's WORDS is bt.WORDS (above)
    for f in ("wavefront_table.h", "kernels_probe.h"):
        assert not re.search(r"constexpr[^;\n]*kBounceProbe\w*Words\w* =", open(os.path.join(device, f)).read()), f
    core_h = open(os.path.join(oracle_lib.ROOT, "include", "lum_core.h")).read()
    enum = re.search(r"enum \{ LUMC_BOUNCE_PROBE_NOT_TAKEN = (\d), LUMC_BOUNCE_PROBE_TAKEN = (\d), LUMC_BOUNCE_PROBE_TOTAL_REFLECTION = (\d) \}", core_h)
    assert [int(x) for x in enum.groups()] == [bt.NOT_TAKEN, bt.TAKEN, bt.TOTAL_REFLECTION]
    enum = re.search(r"LUMC_BOUNCE_PROBE_LD_REFUSED = (\d), LUMC_BOUNCE_PROBE_LD_REFLECTION = (\d), LUMC_BOUNCE_PROBE_LD_REFRACTION = (\d), LUMC_BOUNCE_PROBE_LD_REFRACTION_TOTAL = (\d)", core_h)
    assert [int(x) for x in enum.groups()] == [bt.LD_REFUSED, bt.LD_REFLECTION, bt.LD_REFRACTION, bt.LD_REFRACTION_TOTAL]


# ---- CPU: known answers of the truth ----
def test_a_head_on_view_at_roughness_one_reflects_uniformly():
    """V = N at roughness 1: r^4 = 1, the bounded cap is the whole upper hemisphere (k = 0), the sampled normal is the half vector of +z and (st cos, st sin, 1 - u2),
    so the reflected ray is that vector, uniform on the hemisphere, and its pdf 1 / (2 pi)."""
    rng = np.random.RandomState(3)
    rnd = rng.rand(2000, 2)
    V = np.tile([0.0, 0.0, 1.0], (2000, 1))
    m, _ = bt.sample_vndf_bounded(V, np.ones(2000), rnd)
    ray = bt.reflect(V, m)
    z = 1.0 - rnd[:, 1]
    st = np.sqrt(1.0 - z * z)
    want = np.stack([st * np.cos(2 * np.pi * rnd[:, 0]), st * np.sin(2 * np.pi * rnd[:, 0]), z], axis=-1)
    assert np.abs(ray - want).max() < 1e-12
    assert np.abs(bt.pdf_vndf_bounded(V, np.ones(2000), m[:, 2], np.ones(2000)) - 1.0 / (2.0 * np.pi)).max() < 1e-15
    n = np.maximum(rnd[:, 0], 0.01)   # (G1 clamps the squared cosine at 1e-4)
    assert np.abs(bt.ggx_g1(np.ones(2000), n) - 2.0 * n / (1.0 + n)).max() < 1e-15 and np.abs(bt.ggx_d(rnd[:, 1], np.ones(2000)) - 1.0 / np.pi).max() < 1e-15


def test_an_ior_ratio_of_one_refracts_straight_through_with_term_one():
    fam = families()["materials"]
    t = fam.truth
    sel = np.char.startswith(fam.tags, "glass one")[fam.rows]
    V = bt.qapply(t.q, t.view)[sel]
    m, _ = bt.sample_vndf_caps(V, t.mat.roughness[sel], t.rnd[sel, 2])
    ray, total, b, _ = bt.refract(V, m, np.ones(sel.sum()))
    assert not total.any() and np.abs(ray + V).max() < 1e-12 and np.abs(b - np.abs(bt._dot(m, V)) ** 2).max() < 1e-12
    assert (t.mat.ior[sel] == 1.0).all()
    # the dielectric lobe under the refraction hint is G2 / G1 (1 - F) / energy; F = 0 at ratio 1
    front = V[:, 2] > 0.01
    assert np.abs(bt.fresnel_dielectric(m, V, ray, 1.0))[front].max() < 1e-12
    # ... and the chosen refraction of such a vertex passes through (is_pass_through: ior == 1)
    chosen_refr = sel & (t.chosen == 2)
    assert chosen_refr.sum() > 20 and t.pass_through[chosen_refr].all() and t.transparent_pass[chosen_refr].all()


def test_the_dielectric_lobe_reads_the_roughness_as_ior():
    """The reference's quirk (bsdf_utils.cuh:517), pinned: the lobe's `ior == 1` case, a refraction with term 1, fires at ROUGHNESS 1 whatever the ior ratio is - the
    refracted evaluation of a translucent vertex at roughness 1023 / 1023 is its albedo (or 0 behind the face normal) - and not at the ior ratio 1."""
    fam = families()["roughness 1023"]
    t = fam.truth
    assert (t.mat.roughness == 1.0).all() and (t.mat.ior[t.mat.translucent] != 1.0).all()
    N = t.N
    c = {"f": np.full(N, 0.3), "ndh": np.full(N, 0.9), "ndl": np.full(N, 0.7), "ndv": np.full(N, 0.6), "hdl": np.full(N, 0.8), "hdv": np.full(N, 0.75), "isr": np.ones(N, dtype=bool)}
    ev = bt.eval_layers(t.mat, (np.ones(N), np.zeros(N), np.full(N, 0.9)), c, np.tile([0.8, 0.0, 0.6], (N, 1)), bt.REFRACTION, np.ones(N))
    assert np.array_equal(ev[t.mat.translucent], t.mat.albedo[t.mat.translucent]) and not ev[~t.mat.translucent].any()
    ev = bt.eval_layers(t.mat, (np.ones(N), np.zeros(N), np.full(N, 0.9)), c, np.tile([0.8, 0.0, 0.6], (N, 1)), bt.GENERAL, np.ones(N))
    assert not ev.any()
    one = families()["materials"]
    sel = np.char.startswith(one.tags, "glass one")[one.rows]
    w = one.oracle.reshape(-1, bt.WORDS)[sel, bt.HEAD + 2 * bt.TECH_WORDS:]
    taken = w[:, 0] == bt.TAKEN
    evals = bt._f(w[taken, 14:17])
    lit = evals.any(axis=-1)
    assert lit.sum() > 100 and (evals[lit] != one.truth.mat.albedo[sel][taken][lit]).all(), "at the ior ratio 1 the term is G2 / G1 (1 - F) / energy, not 1"


def test_a_metal_takes_only_the_reflection_and_an_opacity_of_zero_always_passes():
    fam = families()["materials"]
    t = fam.truth
    metal = np.char.startswith(fam.tags, "metallic")[fam.rows]
    assert metal.any() and t.taken[0][metal].all() and not t.taken[1][metal].any() and not t.taken[2][metal].any() and (t.chosen[metal] == 0).all()
    clear = np.char.startswith(fam.tags, "clear")[fam.rows]
    assert clear.any() and t.passes[clear].all() and (t.chosen[clear] == bt.NO_TECHNIQUE).all() and t.pass_through[clear].all()
    half = np.char.startswith(fam.tags, "half")[fam.rows]
    assert 0.4 < t.passes[half].mean() < 0.6
    nearly = np.char.startswith(fam.tags, "nearly opaque")[fam.rows]
    assert t.passes[nearly].mean() < 0.03
    below = np.char.startswith(fam.tags, "glass below")[fam.rows]
    assert not t.total_reflection[below].any(), "an ior ratio below 1 never reflects totally: b >= 1 - ior^2"


REFERENCE_REFRACTION_PDF_INTEGRAL = {(153, 0.95): 0.04498, (307, 0.95): 0.04765, (818, 0.95): 0.09883, (153, 0.5): 0.17408, (307, 0.5): 0.17351, (818, 0.5): 0.13658}


@pytest.mark.parametrize("q", [153, 307, 818])
@pytest.mark.parametrize("cos", [0.95, 0.5])
def test_the_truths_pdfs_integrate_to_one(q, cos):
    """Quadrature over the sphere of directions L. The bounded-VNDF pdf over the directions its cap reaches; the diffuse pdf over the hemisphere; the refraction pdf
    over the lower hemisphere for a ratio below 1 (no total reflection: every microfacet normal refracts)."""
    r = q / 1023.0
    r2, r4 = r * r, r ** 4
    V = np.array([np.sqrt(1.0 - cos * cos), 0.0, cos])
    nt, nphi = 2400, 1200
    ct = (np.arange(nt) + 0.5) / nt * 2.0 - 1.0   # uniform in cos(theta): equal solid angles
    ph = (np.arange(nphi) + 0.5) / nphi * 2.0 * np.pi
    cz, pp = np.meshgrid(ct, ph, indexing="ij")
    st = np.sqrt(1.0 - cz * cz)
    L = np.stack([st * np.cos(pp), st * np.sin(pp), cz], axis=-1)
    dw = 4.0 * np.pi / (nt * nphi)
    Vb = np.broadcast_to(V, L.shape)
    with np.errstate(all="ignore"):
        H = bt._unit(L + V)
        # the cap sample that gives H: the reflection of the stretched view about the stretched normal
        v = bt._unit(np.array([r2 * V[0], r2 * V[1], V[2]]))
        h = np.stack([H[..., 0] / r2, H[..., 1] / r2, H[..., 2]], axis=-1)
        c = h * (2.0 * bt._dot(h, v) / bt._dot(h, h))[..., None] - v
        s = 1.0 + np.sqrt(V[0] ** 2 + V[1] ** 2)
        k = (1.0 - r4) * s * s / (s * s + r4 * V[2] ** 2)
        reached = (c[..., 2] >= -k * v[2]) & (H[..., 2] > 0)
        pdf = bt.pdf_vndf_bounded(Vb, r, H[..., 2], cos)
        total = float(np.sum(np.where(reached, pdf, 0.0)) * dw)
    print("roughness %d/1023, N.V %g: bounded VNDF %.5f" % (q, cos, total))
    assert abs(total - 1.0) < 5e-3
    assert abs(float(np.sum(bt.pdf_diffuse(L[..., 2])) * dw) - 1.0) < 1e-3
    ior = 0.67
    with np.errstate(all="ignore"):
        down = L[..., 2] < 0
        H = bt._unit(L + V * ior)
        H = H * np.where(H[..., 2] < 0, -1.0, 1.0)[..., None]
        # a refraction has V and L on opposite sides of the microfacet
        valid = down & (bt._dot(H, Vb) > 0) & (bt._dot(H, L) < 0)
        hdv, hdl = np.abs(bt._dot(H, Vb)), np.abs(bt._dot(H, L))
        pdf = bt.pdf_refraction(r, H[..., 2], cos, hdv, hdl, ior)
        raw = float(np.sum(np.where(valid, pdf, 0.0)) * dw)
        # the reference's denominator is (ior H.V + H.L)^2 of the two absolute cosines (bsdf_utils.cuh:296) where the change of variables from the microfacet
        # normal to the refracted direction has their difference: its own model, restated as it is. With the difference the same terms are a density.
        total = float(np.sum(np.where(valid, pdf * (ior * hdv + hdl) ** 2 / (ior * hdv - hdl) ** 2, 0.0)) * dw)
    print("roughness %d/1023, N.V %g: refraction %.5f with the Jacobian's denominator, %.5f with the reference's" % (q, cos, total, raw))
    assert abs(total - 1.0) < 5e-3
    # pinned: what the reference's form integrates to (this quadrature, whose error is the 5e-5 seen in `total`)
    assert abs(raw - REFERENCE_REFRACTION_PDF_INTEGRAL[(q, cos)]) < 5e-4, raw


# ---- CPU: the oracle alone ----
MIN_DECISIVE, MIN_DECISIVE_ON_AN_EDGE = 0.95, 0.5


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_the_oracle_passes_and_the_truth_decides(name):
    fam = families()[name]
    fail, fig = yardstick(name)
    t = fam.truth
    shares = t.shares()
    print("%s: %d threads | decisive shares: %s" % (name, t.N, ", ".join("%s %.4f" % kv for kv in sorted(shares.items()))))
    print("  oracle against the truth: " + ", ".join("%s %.3g" % kv for kv in sorted(fig.items()) if " | " not in kv[0]))
    ill = {k: v for k, v in fig.items() if "ill-conditioned" in k}
    print("  ill-conditioned shares: " + ", ".join("%s %.3g" % kv for kv in sorted(ill.items()) if kv[1] > 0))
    _record("oracle", name, dict(fig, **{"decisive share: " + k: v for k, v in shares.items()}))
    assert not any(b.any() for b in fail.values()), "the oracle's probe rejected by the truth:\n" + _describe(fam, fail)
    edge = ON_AN_EDGE.get(name)
    for k, v in shares.items():
        assert v >= (MIN_DECISIVE_ON_AN_EDGE if k in (edge, "all") and edge else MIN_DECISIVE), (k, v)
    if edge:
        others = np.all([v for k, v in t.decisions.items() if k not in (edge, "lut_axis' cell")], axis=0)
        print("  decisive in every decision but %s: %.4f" % (edge, others.mean()))
        assert others.mean() >= MIN_DECISIVE
    if name == "critical angle":
        dec = t.tr_decided & t.taken[2]
        assert (t.total_reflection & dec).sum() >= 50 and (~t.total_reflection & dec).sum() >= 50, "both outcomes among the decisive threads"
        print("  undecided total reflections: %d" % int((~t.tr_decided).sum()))
        assert (~t.tr_decided).sum() >= 3, "some threads at the critical angle are undecided"
    if name == "normals at -1 + kEps":
        o = fam.oracle.reshape(-1, bt.WORDS)
        minus = (o[:, 9:13] == _bits([1.0, 0.0, 0.0, 0.0])).all(axis=-1)
        assert (minus & t.q_decided).sum() >= 50 and (~minus & t.q_decided).sum() >= 50 and (~t.q_decided).any(), "both branches among the decisive threads"
    if name.startswith("roughness") and int(name.split()[1]) >= 153:
        d_words = {k: v for k, v in ill.items() if "pdf" in k or "eval" in k or "weight" in k}
        assert d_words and not any(v > 0 for v in d_words.values()), {k: v for k, v in d_words.items() if v > 0}
        # the oracle's own binary32 pdfs lie within 1e-3 of float64 on their own inputs from this roughness up (measured before these tests were written)
        assert max(v for k, v in fig.items() if "pdf" in k and " | " not in k) < 1e-3


def test_every_status_occurs():
    counts = {}
    for name in FAMILY_NAMES:
        fam = families()[name]
        o = fam.oracle.reshape(-1, bt.WORDS)
        for t, kind in enumerate(bt.TECH_NAMES):
            for s in range(3 if t == 2 else 2):
                counts[(kind, s)] = counts.get((kind, s), 0) + int((o[:, bt.HEAD + bt.TECH_WORDS * t] == s).sum())
        for s in range(4):
            counts[("light direction", s)] = counts.get(("light direction", s), 0) + int((o[:, bt.LD0] == s).sum())
        translucent = (fam.vertices.flags & 1) != 0
        if translucent.any():
            per_vertex = (o[:, bt.HEAD + 2 * bt.TECH_WORDS] != 0).reshape(len(fam.vertices), SAMPLES).any(axis=1)
            opaque_enough = fam.vertices.opacity > 0
            assert per_vertex[translucent & opaque_enough].all(), "a translucent vertex without a taken refraction in " + name
    print(counts)
    assert all(v >= 50 for v in counts.values()), counts


def test_the_older_bsdf_sample_probe_returns_the_new_probes_head():
    fam = families()["materials"]
    v = fam.vertices
    o = fam.oracle
    view = _view_with_luts()
    for k in range(len(v)):
        m = ProbeMaterial(tuple(float(x) for x in v.albedo[k]), float(v.opacity[k]), float(v.roughness[k]), float(v.ior[k]), int(v.flags[k]))
        rays, weights, flags = np.zeros((SAMPLES, 3), np.float32), np.zeros((SAMPLES, 3), np.float32), np.zeros(SAMPLES, np.uint32)
        oracle_lib.lib().oracle_probe_bsdf_sample(C.byref(view), C.byref(m), _f3(v.normal[k]), _f3(v.V[k]), int(v.pixels[k, 0]), int(v.pixels[k, 1]), 0, SAMPLES,
                                                  rays.ctypes.data_as(C.c_void_p), weights.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p))
        assert np.array_equal(rays.view(np.uint32), o[k, :, 3:6]) and np.array_equal(weights.view(np.uint32), o[k, :, 6:9]), fam.tags[k]
        assert np.array_equal(flags, o[k, :, 0] | (o[k, :, 1] << 1)), fam.tags[k]


# ---- CPU: mutants ----
def _mutated(fam):
    return np.array(fam.oracle).reshape(-1, bt.WORDS)


def _f32(words):
    return np.ascontiguousarray(words).view(np.float32)


def _bits(values):
    return np.ascontiguousarray(values, dtype=np.float32).view(np.uint32)


def _rejected(fam, mutated, name, where, minimum=20, with_yardstick=True):
    """every rule whose name begins with `name` (a word's ceiling and its yardstick are two) rejects every mutated answer"""
    fail, _ = fam.truth.check(mutated, yardstick=yardstick(fam.name)[1] if with_yardstick else None, factor=4.0)
    key = [k for k in fail if k.startswith(name)]
    assert 1 <= len(key) <= 2, (name, sorted(fail))
    bad = np.all([fail[k] for k in key], axis=0)
    assert where.sum() >= minimum, "%d answers to mutate for: %s" % (int(where.sum()), name)
    assert bad[where].all(), "%s: %d of %d mutated answers pass" % (name, int((~bad[where]).sum()), int(where.sum()))


def _tech(m, t):
    return m[:, bt.HEAD + bt.TECH_WORDS * t: bt.HEAD + bt.TECH_WORDS * (t + 1)]


def test_mutated_pdfs_and_weights_are_rejected():
    fam = families()["roughness 307"]
    t = fam.truth
    # refraction pdf with ior and 1 / ior swapped (the reflection technique's pdf of the refraction technique, on translucent vertices)
    m = _mutated(fam)
    w = _tech(m, 0)
    c = _f32(w[:, 7:13]).astype(np.float64)
    with np.errstate(all="ignore"):
        swapped = bt.pdf_refraction(t.mat.roughness, c[:, 1], c[:, 3], c[:, 5], c[:, 4], 1.0 / t.mat.ior)
        old = _f32(w[:, 19]).astype(np.float64)
        where = (w[:, 0] != 0) & t.mat.translucent & np.isfinite(swapped) & (np.abs(swapped - old) > 0.05 * np.abs(old)) & (old > 0)
    w[:, 19] = np.where(where, _bits(swapped), w[:, 19])
    _rejected(fam, m, "reflection: pdf of the refraction technique beyond", where)
    # mis -> 1 - mis
    for tech in (0, 1):
        m = _mutated(fam)
        w = _tech(m, tech)
        mis = _f32(w[:, 20])
        where = (w[:, 0] != 0) & (np.abs(mis - 0.5) > 1e-3)
        w[:, 20] = np.where(where, _bits(np.float32(1.0) - mis), w[:, 20])
        _rejected(fam, m, "%s: mis is not the own pdf over the sum" % bt.TECH_NAMES[tech], where)
    # pick not renormalised after a rejection
    for tech in (1, 2):
        m = _mutated(fam)
        w = _tech(m, tech)
        before = _f32(_tech(m, tech - 1)[:, 23]) if tech == 1 else np.where(_tech(m, 1)[:, 0] != 0, _f32(_tech(m, 1)[:, 23]), _f32(_tech(m, 0)[:, 23]))
        prob = _f32(w[:, 22])
        where = (w[:, 0] != 0) & (before >= prob) & (prob > 1e-3)
        w[:, 23] = np.where(where, _bits(before), w[:, 23])
        _rejected(fam, m, "%s: pick after the decision" % bt.TECH_NAMES[tech], where)
    # the neighbour technique's eval reported as the chosen one's; the weight without weight_sum / importance
    for which in ("neighbour", "bare"):
        m = _mutated(fam)
        chosen = m[:, 28]
        ev = np.stack([_f32(_tech(m, k)[:, 14:17]) for k in range(3)], axis=1).astype(np.float64)   # [N, 3 techniques, 3]
        wsum = _f32(m[:, 27]).astype(np.float64)
        rows = np.arange(len(m))
        live = chosen < 3
        own = ev[rows, np.minimum(chosen, 2)]
        if which == "neighbour":
            other = np.where(chosen == 0, np.where(_tech(m, 1)[:, 0] != 0, 1, 2), 0)
            taken = np.stack([_tech(m, k)[:, 0] != 0 for k in range(3)], axis=1)[rows, other]
            e = ev[rows, other]
            with np.errstate(all="ignore"):
                new = e * (wsum / e.max(axis=-1))[:, None]
            old = _f32(m[:, 29:32]).astype(np.float64)
            where = live & taken & np.isfinite(new).all(axis=-1) & (np.abs(new - old).max(axis=-1) > 1e-3 * np.abs(old).max(axis=-1)) & (wsum > 0)
        else:
            new = own
            with np.errstate(all="ignore"):
                where = live & (wsum > 0) & (np.abs(wsum / own.max(axis=-1) - 1.0) > 1e-3)
        m[:, 29:32] = np.where(where[:, None], _bits(new), m[:, 29:32])
        m[:, 6:9] = m[:, 29:32]
        _rejected(fam, m, "final weight is not chosen_eval * (weight_sum / importance)", where)
    # refr_prob 0 on a translucent vertex; probability without rr
    m = _mutated(fam)
    L = m[:, bt.LD0:]
    prob = _f32(L[:, 23])
    where = (L[:, 0] == bt.LD_REFLECTION) & t.mat.translucent & (prob > 0) & np.isfinite(prob)
    L[:, 23] = np.where(where, _bits(prob * np.float32(2.0)), L[:, 23])
    m[:, 43] = L[:, 23]
    _rejected(fam, m, "light direction: probability is not", where)
    m = _mutated(fam)
    L = m[:, bt.LD0:]
    prob, rr = _f32(L[:, 23]), _f32(L[:, 1])
    where = (L[:, 0] != bt.LD_REFUSED) & (prob > 0) & np.isfinite(prob) & (rr < 0.999)
    with np.errstate(all="ignore"):
        L[:, 23] = np.where(where, _bits(prob / rr), L[:, 23])
    m[:, 43] = L[:, 23]
    _rejected(fam, m, "light direction: probability is not", where)


def test_self_consistent_mutants_are_rejected_without_a_yardstick():
    """An answer whose error is carried through every later stage, as a transcription error shared by the oracle and the kernel would be: only the stage's own
    comparison with the float64 truth can tell. Judged as the oracle itself is, with no yardstick."""
    fam = families()["roughness 307"]
    t = fam.truth
    # every evaluation 1 % too large: w, weight_sum and the final weight follow, mis, prob and pick are ratios and stay
    m = _mutated(fam)
    live = m[:, 28] < 3
    scale = np.float32(1.01)

    def scaled(cols):
        m[:, cols] = np.where(live[:, None], _bits(_f32(m[:, cols]) * scale), m[:, cols])
    for k in range(3):
        lo = bt.HEAD + bt.TECH_WORDS * k
        scaled(slice(lo + 14, lo + 17)); scaled(slice(lo + 21, lo + 22))
    scaled(slice(25, 28)); scaled(slice(29, 32)); scaled(slice(6, 9))
    fail, _ = t.check(m)
    named = sorted(k for k, b in fail.items() if b.any())
    assert named and all("eval beyond %g x its bound" % bt.CEILING in k for k in named), named   # (products of rounded products: nothing else notices)
    for k, kind in enumerate(bt.TECH_NAMES):
        w = _tech(m, k)
        where = (w[:, 0] != 0) & _f32(w[:, 14:17]).any(axis=-1)
        _rejected(fam, m, "%s: eval beyond %g x its bound" % (kind, bt.CEILING), where, with_yardstick=False)
    # the reflection's microfacet normal and ray turned about the local view by a milliradian, seen head-on (V = N): every cosine, pdf and weight stays, the
    # reflected ray is the turned normal's, the world ray follows
    m = _mutated(fam)
    head_on = np.char.endswith(fam.tags, "V = N")[fam.rows] & (m[:, bt.HEAD] != 0)
    w = _tech(m, 0)
    Vl, q = bt._f(m[:, 13:16]), bt._f(m[:, 9:13])
    assert np.abs(Vl[head_on] - [0.0, 0.0, 1.0]).max() < 1e-6
    a = 1e-3
    turn = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    mm = bt._f(w[:, 1:4]) @ turn.T
    ray = bt.reflect(Vl, mm)
    w[:, 1:4] = np.where(head_on[:, None], _bits(mm), w[:, 1:4])
    w[:, 4:7] = np.where(head_on[:, None], _bits(ray), w[:, 4:7])
    chosen = head_on & (m[:, 28] == 0)
    world = _bits(bt._unit(bt.qapply(bt.qinv(q), bt._f(w[:, 4:7]))))
    m[:, 32:35] = np.where(chosen[:, None], world, m[:, 32:35])
    m[:, 3:6] = m[:, 32:35]
    sideways = head_on & (np.abs(bt._f(fam.oracle.reshape(-1, bt.WORDS)[:, bt.HEAD + 1:bt.HEAD + 3])).max(axis=-1) > 0.05)   # (a normal on the axis does not turn)
    fail, _ = t.check(m)
    named = sorted(k for k, b in fail.items() if b.any())
    assert named == ["reflection: m beyond %g x its bound" % bt.CEILING], named
    _rejected(fam, m, "reflection: m beyond %g x its bound" % bt.CEILING, sideways, with_yardstick=False)
    # ... and the ray alone, turned away from the reflection of the reported normal
    m = _mutated(fam)
    w = _tech(m, 0)
    on = m[:, bt.HEAD] != 0
    ray = bt._unit(bt._f(w[:, 4:7]) + np.array([1e-4, -1e-4, 1e-4]))
    w[:, 4:7] = np.where(on[:, None], _bits(ray), w[:, 4:7])
    _rejected(fam, m, "reflection: ray beyond %g x its bound" % bt.CEILING, on, with_yardstick=False)


def test_an_inverted_total_reflection_is_rejected_on_decisive_threads():
    fam = families()["critical angle"]
    t = fam.truth
    m = _mutated(fam)
    w = _tech(m, 2)
    c = bt._f(w[:, 1:4])
    Vl = bt._f(m[:, 13:16])
    _, _, b, eb = bt.refract(Vl, c, t.mat.ior)
    where = (w[:, 0] != 0) & (np.abs(b) > eb)
    w[:, 0] = np.where(where, np.where(w[:, 0] == bt.TAKEN, bt.TOTAL_REFLECTION, bt.TAKEN), w[:, 0]).astype(np.uint32)
    _rejected(fam, m, "refraction: total_reflection differs on a decisive thread", where, minimum=200)
    assert ((fam.oracle.reshape(-1, bt.WORDS)[where, bt.HEAD + 2 * bt.TECH_WORDS]) == bt.TOTAL_REFLECTION).sum() >= 50


def test_the_plus_z_quaternion_on_a_minus_z_normal_is_rejected():
    fam = families()["normals at -1 + kEps"]
    m = _mutated(fam)
    where = (np.char.startswith(fam.tags, "-z") | np.char.startswith(fam.tags, "just below"))[fam.rows]
    assert (m[where, 9:13] == _bits([1.0, 0.0, 0.0, 0.0])).all(), "the -z branch of rotation_to_z"
    above = np.char.startswith(fam.tags, "just above")[fam.rows]
    assert above.any() and not (m[above, 9:13] == _bits([1.0, 0.0, 0.0, 0.0])).all(axis=-1).any(), "the general branch just above -1 + kEps"
    m[:, 9:13] = np.where(where[:, None], _bits([0.0, 0.0, 0.0, 1.0]), m[:, 9:13])
    _rejected(fam, m, "quaternion does not take the normal to +z", where)


def test_words_that_are_no_numbers_are_rejected():
    fam = families()["roughness 307"]
    t = fam.truth
    base = fam.oracle.reshape(-1, bt.WORDS)
    live = base[:, 28] < 3
    cases = [(w, live & ~t.q_minus) for w in range(3, 22)] + [(w, live) for w in (25, 26, 27, 29, 30, 31, 32, 33, 34)]
    for tech in range(3):
        s = base[:, bt.HEAD + bt.TECH_WORDS * tech]
        for w in list(range(1, 13)) + list(range(14, 24)):
            where = s != 0
            if w == 7:
                where = where & t.mat.translucent
            if 17 <= w <= 19 and tech == 2:
                where = where & (s == bt.TOTAL_REFLECTION)
            if w >= 22 and tech == 0:
                continue
            cases.append((bt.HEAD + bt.TECH_WORDS * tech + w, where))
    s = base[:, bt.LD0]
    cases += [(bt.LD0 + w, (s != 0) & (t.mat.translucent if w == 9 else True)) for w in list(range(1, 15)) + list(range(16, 27))]
    cases += [(w, s != 0) for w in range(37, 44)]
    for word, where in cases:
        where = where & np.isfinite(_f32(base[:, word]))
        if not where.any():
            continue
        for bits in (0x7FC00000, 0x7F800000):
            m = _mutated(fam)
            m[:, word] = np.where(where, np.uint32(bits), m[:, word])
            fail, _ = t.check(m, yardstick=yardstick(fam.name)[1], factor=4.0)
            assert fail["non-finite word"][where].all(), "word %d = %08x passes on %d of %d threads" % (word, bits, int((~fail["non-finite word"][where]).sum()), int(where.sum()))


# ---- GPU ----
@functools.lru_cache(maxsize=None)
def _device_all(flavour):
    """every family's words from one context of the flavour"""
    from luminary_amd.core import Core
    core = Core(0)
    try:
        core.upload(_view_with_luts())
        core.set_flavour(flavour)
        out = {k: core.bounce_probe_host(families()[k].vertices.words(), 0, SAMPLES) for k in FAMILY_NAMES}
    finally:
        core.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_gpu_exact_flavour_is_the_oracles_probe(name):
    fam = families()[name]
    got = _device_all("exact")[name]
    diff = got != fam.oracle
    assert not diff.any(), "%s: %d words differ from the oracle's probe, first at (vertex, sample, word) %s" % (name, int(diff.sum()), np.argwhere(diff)[:8].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILY_NAMES)
@pytest.mark.parametrize("flavour", ["exact", "fast"])
def test_gpu_bounces_against_the_truth(flavour, name):
    fam = families()[name]
    got = _device_all(flavour)[name]
    fail, fig = fam.truth.check(got, yardstick=yardstick(name)[1], factor=4.0, bitwise_walks=flavour == "exact")
    print("%s, %s flavour: %s" % (name, flavour, ", ".join("%s %.3g" % kv for kv in sorted(fig.items()) if " | " not in kv[0])))
    if flavour == "fast":
        _record("fast", name, fig)
    assert not any(b.any() for b in fail.values()), "%s, %s flavour rejected:\n%s" % (name, flavour, _describe(fam, fail))


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_gpu_fast_and_exact_choose_the_same_technique_where_the_truth_decides(name):
    fam = families()[name]
    e, f = _device_all("exact")[name].reshape(-1, bt.WORDS), _device_all("fast")[name].reshape(-1, bt.WORDS)
    dec = fam.truth.decisive
    differ = (e[:, 28] != f[:, 28]) | (e[:, 0:3] != f[:, 0:3]).any(axis=-1)
    print("%s: %d of %d threads decisive, the flavours' techniques differ on %d threads" % (name, int(dec.sum()), len(dec), int(differ.sum())))
    assert not (differ & dec).any(), np.nonzero(differ & dec)[0][:8].tolist()


@pytest.mark.gpu
def test_gpu_fast_flavour_estimators_are_unbiased():
    """40 000 sample ids on four vertices: the mean of the bounce weight per channel, of the light direction's weight per channel and of its probability in the fast
    flavour against the oracle's on the same ids, within three standard errors of the difference of the two means (sqrt(s_a^2 / n + s_b^2 / n)). That is the error
    of two independent samples. These two share their ids and are almost perfectly correlated, so the bound is loose by orders of magnitude: it catches a flavour
    whose estimator has another mean, not one that is off by its roundings. The paired figure, mean(a - b) over its own standard error, is printed beside it and not
    asserted: both flavours round every sample, one of them with reciprocals that err to one side, and a difference of 1e-8 of the mean is no bias of the estimator."""
    from luminary_amd.core import Core
    n = 40_000
    mats = [MATERIALS["opaque smooth"], ((0.9, 0.95, 1.0), 1.0, 153 / 1023, 1.5, 1), MATERIALS["metallic"], ((0.8, 0.6, 0.4), 0.5, 307 / 1023, 0.67, 1 | 2 | 8)]
    views = [0.5, 0.85, 0.3, 0.6]
    v = lt.Vertices(np.zeros((4, 3)), [GENERIC] * 4, [_view(GENERIC, c) for c in views], [m[0] for m in mats], [m[1] for m in mats], [m[2] for m in mats],
                    [m[3] for m in mats], [m[4] for m in mats], [(NONE, NONE)] * 4, [(4, 9), (7, 2), (11, 13), (1, 5)])
    core = Core(0)
    try:
        core.upload(_view_with_luts())
        core.set_flavour("fast")
        got = core.bounce_probe_host(v.words(), 0, n)
    finally:
        core.close()
    ref = oracle_lib.bounce_stages(_view_with_luts(), v.words(), 0, n)
    for k in range(4):
        for what, words in (("bounce weight", slice(6, 9)), ("light direction weight", slice(40, 43)), ("light direction probability", slice(43, 44))):
            a, b = got[k][:, words].copy().view(np.float32).astype(np.float64), ref[k][:, words].copy().view(np.float32).astype(np.float64)
            assert np.isfinite(a).all() and np.isfinite(b).all()
            diff = a.mean(axis=0) - b.mean(axis=0)
            se = np.sqrt(a.var(axis=0, ddof=1) / n + b.var(axis=0, ddof=1) / n)
            paired = (a - b).std(axis=0, ddof=1) / np.sqrt(n)
            print("vertex %d, %s: fast mean %s, oracle mean %s, difference %s, standard error %s, paired standard error %s" % (
                k, what, a.mean(axis=0), b.mean(axis=0), diff, se, paired))
            assert (np.abs(diff) <= 3.0 * se).all(), (k, what, diff, se)
            assert (b.mean(axis=0) > 0).all(), "the estimator is not empty"


@pytest.mark.gpu
def test_gpu_a_switched_context_runs_the_probe_of_a_fresh_context_in_that_flavour(monkeypatch):
    """Each flavour's probes are a unit of their own with a sampler seed table of their own (kernels_probe.h), chosen per launch from the context's flavour
    (context.h probes_of). One context switched exact -> fast -> exact answers, bit for bit, what a context created in that flavour answers; the exact words are the
    oracle's, so a seed table that was never filled does not pass as two equal wrong answers."""
    from luminary_amd.core import Core
    mats = [MATERIALS["opaque smooth"], MATERIALS["glass above"], MATERIALS["metallic"], MATERIALS["half coloured"]]
    v = lt.Vertices(np.zeros((4, 3)), [GENERIC] * 4, [_view(GENERIC, c) for c in (0.5, 0.85, 0.3, 0.6)], [m[0] for m in mats], [m[1] for m in mats], [m[2] for m in mats],
                    [m[3] for m in mats], [m[4] for m in mats], [(NONE, NONE)] * 4, [(4, 9), (7, 2), (11, 13), (1, 5)]).words()
    fresh = {}
    for flavour in ("exact", "fast"):
        monkeypatch.setenv("LUM_FLAVOUR", flavour)  # read by lumc_context_create: no lumc_set_flavour on this context
        core = Core(0)
        try:
            assert core.flavour == flavour
            core.upload(_view_with_luts())
            fresh[flavour] = core.bounce_probe_host(v, 0, 2)
        finally:
            core.close()
    assert fresh["exact"].shape == (4, 2, bt.WORDS) and (fresh["exact"] == oracle_lib.bounce_stages(_view_with_luts(), v, 0, 2)).all()
    assert (fresh["fast"] != fresh["exact"]).any() and (fresh["fast"][..., 28] == fresh["exact"][..., 28]).all()  # another arithmetic, the same random numbers
    core = Core(0)
    try:
        core.upload(_view_with_luts())
        for flavour in ("exact", "fast", "exact"):
            core.set_flavour(flavour)
            got = core.bounce_probe_host(v, 0, 2)
            diff = got != fresh[flavour]
            assert not diff.any(), "after the switch to %s: %d words differ from a fresh context's, first at (vertex, sample, word) %s" % (flavour, int(diff.sum()), np.argwhere(diff)[:8].tolist())
    finally:
        core.close()
