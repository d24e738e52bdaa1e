"""The sampled-light half of next-event estimation (csrc/device/dev_light.h sample_light, through k_light_sample_probe) against the float64 truth of
tests/light_truth.py, in both flavours and both forms of the shading kernel.

What is held, per (vertex, sample id): the root pass's eight continuation words (picked child, 20-bit probability) and root_sum; per lane the tree's light and weight
(descent included), the candidate's status, ray, solid angle, distance, emitted colour, direction probability, MIS weight and reservoir target; the outer reservoir's
choice and the sample's colour. The BSDF weight is held to oracle_probe_bsdf_eval on the device's own directions and, with the same tolerance, to the float64
evaluation of tests/bsdf_truth.py (eval_bsdf under the general hint) on them, away from the horizon where the packed face normal decides.

Families: one mesh of flat emissive triangles over a small floor, identity instance, 1 .. 300 lights (7 / 8 / 9: the root's padding; 127 / 128: the key's last index;
129 .. 300: nodes below the root; 257 / 300: lights past the LDS stage), powers over four decades (up to 64 lights) and some a million times below the strongest, one-sided and bidirectional emitters;
vertices in front of and behind the panels, beyond all importance, on a child's mean, on a light with self named and not named, with grazing normals, 0.1 .. 1e4 away;
opaque rough and smooth, translucent with ior above and below 1, metallic.

Tolerances of the quantities that go through sin, cos, atan2: the oracle's binary32 result against the truth on the same inputs is the yardstick (computed here on the
CPU, printed, written to profiles/light_sample_truth.json); the fast flavour may be 4 x that away (floor 4 ulp): it replaces correctly rounded divisions and roots by
1-ulp ones in at most three chained normalisations, contraction only removes roundings, a factor two is spare.

CPU tests: known answers; the oracle's probes alone pass the acceptor with the decisive shares at or above their caps; mutated answers are rejected by name; the
binary32 models of tests/test_root_pass_forms.py never leave the truth's pick on a decisive lane.
GPU tests: the exact flavour equals the oracle word for word in both forms; both flavours pass the acceptor; staged and unstaged lights give the same words; the
resampling weights of the fast flavour are unbiased.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import light_truth as lt
import oracle_lib
import test_root_pass_forms as forms
from luminary_amd import Host, scenes
from test_oracle_analytic import ProbeMaterial, _f3

NONE = 0xFFFFFFFF
COUNTS = [1, 2, 7, 8, 9, 64, 127, 128, 129, 256, 257, 300]
ONE_SIDED_ONLY = (7, 127)   # every panel one-sided: behind them no candidate survives
SAMPLES = 24
MIN_DECISIVE = {1: 0.9, 2: 0.9, 7: 0.9, 8: 0.9, 9: 0.9, 64: 0.5, 127: 0.25, 128: 0.25}
MIN_OUTER = 0.8
ROUGH, SMOOTH, GLASS_IN, GLASS_OUT, METAL = range(5)
#             albedo            opacity roughness ior  flags
MATERIALS = [((0.8, 0.7, 0.6), 1.0, 0.8, 1.0, 0), ((0.9, 0.9, 0.9), 1.0, 0.15, 1.0, 0), ((0.9, 0.95, 1.0), 1.0, 0.3, 1.5, 1), ((0.9, 0.95, 1.0), 1.0, 0.35, 0.7, 1 | 2),
             ((0.95, 0.8, 0.5), 1.0, 0.4, 1.0, 4)]
PROFILE = os.path.join(oracle_lib.ROOT, "profiles", "light_sample_truth.json")
# the fast flavour's largest relative distance of a lane's BSDF weight from oracle_probe_bsdf_eval on the same direction, measured on the MI355X over all families
# (profiles/light_sample_truth.json "fast"); asserted at 4 x
FAST_MEASURED = 5.66e-4


def _panel(cx, cz, y, size, facing_down):
    a, b, c = [cx - size, y, cz - size], [cx + size, y, cz - size], [cx, y, cz + size]
    return [a, b, c] if facing_down else [a, c, b]


def _scene(n):
    """n panels at height ~3 over a floor, facing down. Up to 64 lights: powers over four decades and every fifth a million times below the strongest (the tree's
    builder gives such a light one quantum of power, never 0). The builder orders the lights by what they add, so the lights with the highest ids - root index 127,
    the lights past the LDS stage - are the weakest; with 127 and more lights the powers stay within two decades, above 256 within one, so that those get picked."""
    rng = np.random.RandomState(1000 + n)
    host = Host()
    scenes.apply_benchmark_settings(host, 16, 16, 2, sky=(0.5, 0.5, 0.5))
    powers = [0.05, 0.5, 5.0, 50.0, 500.0, 0.0005] if n <= 64 else [5.0, 15.0, 50.0, 150.0, 500.0, 8.0] if n <= 256 else [50.0, 100.0, 200.0, 350.0, 500.0, 75.0]
    mats = []
    for k, p in enumerate(powers):
        for bidirectional in (False, True):
            m = scenes._material((0.9, 0.5, 0.25), 0.7, emission=(p, 0.8 * p, 0.6 * p), bidirectional=bidirectional and n not in ONE_SIDED_ONLY)
            mats.append(host.add_material(m))
    floor = host.add_material(scenes._material((0.7, 0.7, 0.7), 0.9))
    side = int(np.ceil(np.sqrt(n)))
    tris, ids = [], []
    for k in range(n):
        cx, cz = 1.25 * (k % side) - 0.625 * (side - 1), 1.25 * (k // side) - 0.625 * (side - 1)
        # (the second panel is tiny: from afar its solid angle falls below 1e-7)
        tris.append(_panel(cx + rng.uniform(-0.2, 0.2), cz + rng.uniform(-0.2, 0.2), 3.0 + rng.uniform(-0.25, 0.25), 0.002 if k == 1 else 0.4, True))
        level = 5 if (k % 5 == 4 and n > 2) else int(rng.randint(0, 5))
        if k == 0:
            level = 4
        ids.append(mats[2 * level + (k % 2)])
    ext = 0.7 * side + 2.0
    tris += [[[-ext, 0, -ext], [ext, 0, -ext], [ext, 0, ext]], [[-ext, 0, -ext], [ext, 0, ext], [-ext, 0, ext]]]
    ids += [floor, floor]
    mesh = host.add_mesh(np.asarray(tris, dtype=np.float32).reshape(len(tris), 9), np.asarray(ids, dtype=np.uint16))
    host.new_instance(mesh, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    scenes.set_camera(host, (0.0, 1.0, 10.0), (0.0, 0.0, 0.0))
    return host, oracle_lib.with_luts(host.device_scene())


class Family:
    def __init__(self, n):
        self.n = n
        self.host, self.view = _scene(n)
        assert self.view.num_lights == n, "every panel is a light: %d of %d" % (self.view.num_lights, n)
        self.scene = sc = lt.scene_of_view(self.view)
        # the root shape the family is there for
        if n <= 128:
            assert sc.num_root_lights == n and sc.num_children == 8 * ((n + 7) // 8) and sc.num_nodes == 0, (sc.num_root_lights, sc.num_children, sc.num_nodes)
        else:
            assert sc.num_nodes > 0 and sc.num_children <= 128 and sc.num_root_lights < sc.num_children, (sc.num_root_lights, sc.num_children, sc.num_nodes)
        rng = np.random.RandomState(2000 + n)
        ext = 0.625 * int(np.ceil(np.sqrt(n)))
        pos, nrm, view, mat, selfs, tags = [], [], [], [], [], []

        def add(p, nr, tag, m=None, handle=(NONE, NONE)):
            pos.append(p); nrm.append(nr); view.append(rng.normal(size=3) * 0.3 + np.asarray(nr)); tags.append(tag)
            mat.append(len(pos) % len(MATERIALS) if m is None else m); selfs.append(handle)
        for _ in range(10):   # in front of the panels
            add([rng.uniform(-ext, ext), rng.uniform(0.1, 2.2), rng.uniform(-ext, ext)], [rng.uniform(-0.4, 0.4), 1.0, rng.uniform(-0.4, 0.4)], "front")
        for k in range(4):    # behind the panels, looking down at their backs
            add([rng.uniform(-ext, ext), 5.0 + k, rng.uniform(-ext, ext)], [0.1 * k, -1.0, 0.0], "behind")
        for k in range(2):    # beyond all importance: the squared distance overflows binary32, its reciprocal is 0 and so is every child's importance
            add([3e19, -3e19 * (k + 1), 1e19], [0.0, 1.0, 0.0], "beyond", m=(ROUGH, GLASS_IN)[k])
        # exactly on a child's mean that has no variance: 0 * inf, the NaN the maximum must drop. The tree's builder gives every real child a standard deviation and
        # a power of at least one quantum; the children that pad the root to a multiple of eight have neither, and their mean is the root's base point.
        zero_var = np.nonzero(sc.sd == 0)[0]
        assert (sc.power[zero_var] == 0).all() and np.array_equal(zero_var, np.nonzero(sc.power == 0)[0]) and (n > 128 or len(zero_var) == (-n) % 8)
        if len(zero_var):
            c = int(zero_var[0])
            add(sc.mean[c], [0.0, -1.0, 0.0], "on_mean", m=ROUGH)
            add(sc.mean[c], [0.3, -1.0, 0.2], "on_mean", m=SMOOTH)
        for k, light in enumerate([n - 1, n - 1, 0, n // 2]):   # on a light (the last one: index 127, or light 256), self named and not named; tilted normals
            p = sc.p0[light] + 0.3 * sc.e1[light] + 0.25 * sc.e2[light]
            add(np.float32(p), [0.8 if k % 2 else -0.8, -1.0, 0.3], "on_light", handle=tuple(int(x) for x in sc.handles[light]) if k != 1 else (NONE, NONE))
        for k, m in enumerate((GLASS_IN, GLASS_OUT)):   # translucent, in front of the panels and facing away from them: every light is seen through the surface (N.L < 0)
            add([rng.uniform(-ext, ext), 1.0 + 0.5 * k, rng.uniform(-ext, ext)], [0.2 * k, -1.0, 0.1], "through", m=m)
        if n > 256:           # on light 256, naming light 255 as self: an implementation that answers light 255's handle for light 256 skips the light it stands on
            p = sc.p0[256] + 0.3 * sc.e1[256] + 0.25 * sc.e2[256]
            add(np.float32(p), [0.8, -1.0, 0.3], "wrong_self", m=SMOOTH, handle=tuple(int(x) for x in sc.handles[255]))
        for k in range(3):    # grazing normals
            add([rng.uniform(-ext, ext), 1.5, rng.uniform(-ext, ext)], [1.0, 0.002 * (k - 1), 0.05 * k], "grazing")
        add(np.float32(sc.p0[0] + 0.3 * sc.e1[0] + 0.3 * sc.e2[0]) - np.float32([0.0, 0.1, 0.0]), [0.0, 1.0, 0.1], "near")   # 0.1 below a panel
        for d in (30.0, 1e3, 1e4):
            add([0.3 * d, 3.0 - d, 0.1 * d], [0.0, 1.0, 0.0], "far")
        V = len(pos)
        m = [MATERIALS[k] for k in mat]
        self.tags = np.asarray(tags)
        self.vertices = lt.Vertices(pos, nrm, view, [x[0] for x in m], [x[1] for x in m], [x[2] for x in m], [x[3] for x in m], [x[4] for x in m], selfs,
                                    [[(3 * k) % 16, (5 * k + n) % 16] for k in range(V)])
        assert V * SAMPLES <= 20000
        self.truth = lt.Truth(sc, self.vertices, 0, SAMPLES)
        self.oracle = oracle_lib.light_sample_stages(self.view, self.vertices.words(), 0, SAMPLES)
        self.oracle.setflags(write=False)
        self.rows = np.repeat(np.arange(V), SAMPLES)   # thread -> vertex


@functools.lru_cache(maxsize=None)
def family(n):
    return Family(n)


@functools.lru_cache(maxsize=None)
def yardstick(n):
    fam = family(n)
    fail, fig = fam.truth.check(fam.oracle, luts=oracle_lib.golden_luts(), bsdf_tolerance=4.0 * FAST_MEASURED)
    return fail, fig


def _bsdf_reference(fam, out):
    """oracle_probe_bsdf_eval on the directions the answer itself holds: [N, 8, 3]"""
    v = fam.vertices
    o = np.ascontiguousarray(out, dtype=np.uint32).reshape(len(v), SAMPLES, lt.WORDS)
    rays = o[:, :, lt.HEAD:].reshape(len(v), SAMPLES * lt.LANES, lt.LANE_WORDS)[:, :, 3:6].copy().view(np.float32)
    ref = np.zeros_like(rays)
    for k in range(len(v)):
        m = ProbeMaterial(tuple(float(x) for x in v.albedo[k]), float(v.opacity[k]), float(v.roughness[k]), float(v.ior[k]), int(v.flags[k]))
        L = np.ascontiguousarray(rays[k])
        oracle_lib.lib().oracle_probe_bsdf_eval(C.byref(fam.view), C.byref(m), _f3(v.normal[k]), _f3(v.V[k]), len(L), L.ctypes.data_as(C.c_void_p), C.c_float(1.0),
                                                ref[k].ctypes.data_as(C.c_void_p))
    return ref.reshape(len(v) * SAMPLES, lt.LANES, 3).astype(np.float64)


def _describe(fam, fail, limit=4):
    lines = []
    for name, bad in fail.items():
        if bad.any():
            idx = np.argwhere(bad)[:limit]
            lines.append("%s: %d | first at %s" % (name, int(bad.sum()), ["vertex %d (%s) sample %d%s" % (
                i[0] // SAMPLES, fam.tags[i[0] // SAMPLES], i[0] % SAMPLES, (" lane %d" % i[1]) if len(i) > 1 else "") for i in idx]))
    return "\n".join(lines)


def _record(section, name, figures):
    try:
        data = json.load(open(PROFILE))
    except (OSError, ValueError):
        data = {}
    new = {k: float("%.3e" % v) for k, v in sorted(figures.items())}
    if data.get(section, {}).get(name) == new:
        return  # the record stands: a run that measures what is written leaves the file alone
    data.setdefault(section, {})[name] = new
    try:
        with open(PROFILE, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass  # a read-only tree: the figures are printed


def test_the_probes_layout_is_one_layout():
    """The words per vertex and per thread, as include/lum_core.h, oracle/oracle.h, luminary_amd/core.py, the truth and the kernel's header state them."""
    import re
    from luminary_amd.core import Core

    def defines(path, prefix):
        text = open(os.path.join(oracle_lib.ROOT, path)).read()
        return {k: int(v) for k, v in re.findall(r"#define %s_(\w+) (\d+)" % prefix, text)}
    core_h, oracle_h = defines("include/lum_core.h", "LUMC_LIGHT_PROBE"), defines("oracle/oracle.h", "ORACLE_LIGHT_PROBE")
    assert core_h == oracle_h == {"VERTEX_WORDS": 20, "WORDS": lt.WORDS} == {"VERTEX_WORDS": Core.LIGHT_PROBE_VERTEX_WORDS, "WORDS": Core.LIGHT_PROBE_WORDS}
    assert (oracle_lib.LIGHT_PROBE_VERTEX_WORDS, oracle_lib.LIGHT_PROBE_WORDS) == (20, lt.WORDS) and lt.WORDS == lt.HEAD + lt.LANES * lt.LANE_WORDS
    assert lt.Vertices([[0, 0, 0]], [[0, 1, 0]], [[0, 1, 0]], [[1, 1, 1]], [1], [1], [1], [0], [(0, 0)], [(0, 0)]).words().shape == (1, 20)
    csrc = os.path.join(oracle_lib.ROOT, "luminary_amd", "csrc")
    layout = open(os.path.join(csrc, "device", "probe_layout.h")).read()  # the one definition: the kernels (kernels_probe.h) and the host layer (probes.hip) include it
    assert re.search(r"kLightProbeVertexWords = 20, kLightProbeLaneWords = %d, kLightProbeHeadWords = %d, kLightProbeLanes = %d;" % (lt.LANE_WORDS, lt.HEAD, lt.LANES), layout)
    assert re.search(r"kLightProbeWords = kLightProbeHeadWords \+ kLightProbeLanes \* kLightProbeLaneWords;", layout)
    assert "static_assert(kLightProbeLanes == kLightTreeOutputs" in open(os.path.join(csrc, "device", "kernels_probe.h")).read()
    assert "LUMC_LIGHT_PROBE_VERTEX_WORDS == kLightProbeVertexWords && LUMC_LIGHT_PROBE_WORDS == kLightProbeWords" in open(os.path.join(csrc, "host", "probes.hip")).read()
    assert "ProbeWords =" not in open(os.path.join(csrc, "device", "wavefront_table.h")).read()
    enum = re.search(r"enum \{ LUMC_LIGHT_PROBE_NO_PICK = (\d), LUMC_LIGHT_PROBE_SELF = (\d), LUMC_LIGHT_PROBE_REFUSED = (\d), LUMC_LIGHT_PROBE_MISSED = (\d), LUMC_LIGHT_PROBE_EVALUATED = (\d) \}",
                     open(os.path.join(oracle_lib.ROOT, "include", "lum_core.h")).read())
    assert [int(x) for x in enum.groups()] == [lt.NO_PICK, lt.SELF, lt.REFUSED, lt.MISSED, lt.EVALUATED]


# ---- CPU: known answers of the truth ----
def test_one_light_is_every_lanes_pick():
    fam = family(1)
    t = fam.truth
    front = np.isin(fam.tags, ("front", "near"))[fam.rows]
    assert (t.pick[front] == 0).all() and t.decisive[front].all() and (t.p[front] == 1.0).all() and (t.q[front] == 1048575).all()
    assert np.allclose(t.weight[front], 0.125, rtol=0, atol=0)
    beyond = (fam.tags == "beyond")[fam.rows]
    assert (t.T[beyond] == 0).all() and (t.pick[beyond] == -1).all() and (t.root_sum[beyond] == 0).all()


def test_two_equal_lights_split_at_one_half():
    w = np.array([[3.0], [3.0]]) * np.ones((1, 64))
    u = (np.arange(64, dtype=np.float64)[:, None] + 0.5) / 64.0
    pick, dec, T, eT, r, er = lt.scan(w, np.zeros_like(w), u)
    assert (pick[:, 0] == np.where(u[:, 0] < 0.5, 1, 0)).all() and dec.all() and (T == 6.0).all()
    # the second light is accepted with p = 1/2 when r < 1/2 and leaves r / p; a rejected r leaves (r - p) / (1 - p)
    assert np.allclose(r[:, 0], np.where(u[:, 0] < 0.5, 2.0 * u[:, 0], 2.0 * u[:, 0] - 1.0))
    # at u = 1/2 exactly the decision is not decided
    assert not lt.scan(w[:, :1], np.zeros((2, 1)), np.array([[0.5]]))[1].any()


def test_a_vertex_on_the_lights_plane():
    """po lies in the plane through the child's mean that the normal is normal to: the cosine is 0 and the importance is the variance term alone, power * var / (d^2 +
    var)^2; for a translucent vertex it is power / (d^2 + var); on the mean of a padding child (no power, no variance) it is the NaN the root pass drops."""
    fam = family(7)
    sc = fam.scene
    light = 3
    p = sc.mean[light] + np.array([0.3, 0.0, 0.1])
    up = np.array([[0.0, -1.0, 0.0]])
    den = 0.3 * 0.3 + 0.1 * 0.1 + sc.sd[light] ** 2
    w, e = lt.importance(p[None, :], up, np.array([False]), sc.mean[None, light], sc.sd[None, light], sc.power[None, light])
    assert abs(w[0] - sc.power[light] * sc.sd[light] ** 2 / den ** 2) < 1e-12 * w[0] and 0 < e[0] < 1e-5 * w[0]
    w, e = lt.importance(p[None, :], up, np.array([True]), sc.mean[None, light], sc.sd[None, light], sc.power[None, light])
    assert abs(w[0] - sc.power[light] / den) < 1e-12 * w[0] and 0 < e[0] < 1e-6 * w[0]
    pad = 7
    assert sc.power[pad] == 0 and sc.sd[pad] == 0
    w, e = lt.importance(sc.mean[None, pad], up, np.array([False]), sc.mean[None, pad], sc.sd[None, pad], sc.power[None, pad])
    assert w[0] == 0.0 and e[0] == 0.0
    on_mean = (fam.tags == "on_mean")[fam.rows]
    assert on_mean.any() and np.isfinite(fam.truth.T[on_mean]).all() and (fam.truth.T[on_mean] > 0).all()


def test_the_truths_direction_probability_is_the_oracles():
    """light_direction_probability on its own (oracle_probe_light_direction_probability), reflections and - for the translucent materials - refractions: the float64
    restatement in world space against the oracle's binary32 in the shading frame."""
    rng = np.random.RandomState(21)
    nrm = np.float32([0.3, 0.9, -0.2])
    view = np.float32([0.5, 0.7, 0.4])
    n64, v64 = lt._unit(nrm.astype(np.float64)), lt._unit(view.astype(np.float64))
    L = lt._unit(rng.normal(size=(4000, 3))).astype(np.float32)
    L64 = lt._unit(L.astype(np.float64))
    cos = L64 @ n64
    clear = np.abs(cos) > 0.05   # away from the horizon, where the sign of N.L decides the technique
    for (albedo, opacity, roughness, ior, flags) in MATERIALS:
        v = lt.Vertices([[0, 0, 0]], [nrm], [view], [albedo], [opacity], [roughness], [ior], [flags], [(NONE, NONE)], [(0, 0)])
        ro, io = v.material_words()
        want, refr = lt.direction_probability(n64[None, :], v64[None, :], L64, ro[0], io[0], bool(flags & 1))
        got = np.zeros(len(L), dtype=np.float32)
        m = ProbeMaterial(albedo, opacity, roughness, ior, flags)
        oracle_lib.lib().oracle_probe_light_direction_probability(C.byref(m), _f3(nrm), _f3(view), len(L), L.ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p))
        assert np.array_equal(refr, cos < 0) and (refr & clear).sum() > 1000
        if roughness >= 0.5:  # the roulette never draws a BSDF direction for such a surface: probability 0 everywhere
            assert not want.any() and not got.any()
            continue
        assert ((want[refr] == 0) == (not flags & 1)).all(), "only a translucent vertex gives a refracted direction a probability"
        rel = np.abs(got - want) / np.maximum(want, 1e-30)
        sel = clear & (want > 1e-12)
        print("roughness %.2f ior %.2f flags %d: largest relative distance %.3g over %d directions (%d refractions)" % (roughness, ior, flags, rel[sel].max(), sel.sum(), (sel & refr).sum()))
        assert sel.sum() > 1000 and rel[sel].max() < 1e-3 and (got[clear & (want == 0)] == 0).all()


# ---- CPU: the oracle alone ----
@pytest.mark.parametrize("n", COUNTS)
def test_the_oracle_passes_and_the_truth_decides(n):
    fam = family(n)
    fail, fig = yardstick(n)
    t = fam.truth
    share, outer = t.decisive_share(), float(t.outer_decisive.mean())
    print("%d lights, %d root children, %d nodes, %d threads | decisive share of the root lanes %.4f, of the outer reservoir %.4f" % (
        n, fam.scene.num_children, fam.scene.num_nodes, len(fam.rows), share, outer))
    print("  oracle against the truth: " + ", ".join("%s %.3g" % kv for kv in sorted(fig.items())))
    _record("oracle", str(n), fig)
    assert not any(b.any() for b in fail.values()), "the oracle's probes rejected by the truth:\n" + _describe(fam, fail)
    if n in MIN_DECISIVE:
        assert share >= MIN_DECISIVE[n], share
    assert outer >= MIN_OUTER, outer
    status = fam.oracle.reshape(-1, lt.WORDS)[:, lt.HEAD:].reshape(-1, lt.LANES, lt.LANE_WORDS)[:, :, 2]
    assert (status == lt.EVALUATED).any() and (status == lt.REFUSED).any() and (status == lt.SELF).any()
    # translucent vertices reach evaluated lanes whose direction goes through the surface, with a probability: where pdf_refraction and refr_prob act
    lanes = _lanes(fam.oracle.reshape(-1, lt.WORDS))
    rays = lanes[:, :, 3:6].copy().view(np.float32).astype(np.float64)
    through = (status == lt.EVALUATED) & ((fam.vertices.flags & 1) != 0)[fam.rows][:, None] & (np.sum(rays * t.nrm[fam.rows][:, None, :], axis=-1) < 0)
    with_prob = through & (lanes[:, :, 14].copy().view(np.float32) > 0)
    print("  refracted directions on translucent vertices: %d evaluated lanes, %d with a direction probability" % (int(through.sum()), int(with_prob.sum())))
    assert with_prob.sum() >= 50
    if n in ONE_SIDED_ONLY:  # behind one-sided panels no candidate survives
        behind = (fam.tags == "behind")[fam.rows]
        assert (fam.oracle.reshape(-1, lt.WORDS)[behind, 0] == NONE).all() and (status[behind] != lt.EVALUATED).all()
    if n > 256:
        light = fam.oracle.reshape(-1, lt.WORDS)[:, lt.HEAD:].reshape(-1, lt.LANES, lt.LANE_WORDS)[:, :, 0]
        assert ((light >= 256) & (light != NONE)).any(), "lights past the LDS stage are picked"


def _lanes(out):
    return out.reshape(-1, lt.WORDS)[:, lt.HEAD:].reshape(-1, lt.LANES, lt.LANE_WORDS)


def _mutated(fam):
    return np.array(fam.oracle).reshape(-1, lt.WORDS)


def _rejected(fam, mutated, name, where):
    fail, _ = fam.truth.check(mutated, yardstick=yardstick(fam.n)[1], factor=4.0)
    key = [k for k in fail if k.startswith(name)]
    assert len(key) == 1, (name, list(fail))
    bad = fail[key[0]]
    assert where.any(), "nothing to mutate for: " + name
    assert bad[where].all(), "%s: %d of %d mutated answers pass" % (name, int((~bad[where]).sum()), int(where.sum()))


@pytest.mark.parametrize("n", [9, 64, 128])
def test_mutated_root_answers_are_rejected(n):
    fam, t = family(n), family(n).truth
    N = len(fam.rows)
    # the neighbour's probability word (where the two words differ by more than the acceptor allows)
    m = _mutated(fam)
    cont = m[:, 9:17].astype(np.int64)
    child = (cont >> 1) & 0xFF
    nb = np.where(child + 1 < fam.scene.num_root_lights, child + 1, child - 1).clip(0)
    p_nb = lt.probability_of(t.ws, t.es, t.T, t.eT, nb)[0]
    q, q_nb = cont >> 9, np.maximum(np.rint(1048575.0 * p_nb), (p_nb > 0) * 1.0).astype(np.int64)
    where = (q > 0) & (np.abs(q - q_nb) > 2 + 2.0 ** -14 * q)
    m[:, 9:17] = np.where(where, (cont & 0x1FF) | (q_nb << 9), cont).astype(np.uint32)
    _rejected(fam, m, "probability word is not the picked child's", where)
    # the weight without the factor 8
    m = _mutated(fam)
    lanes = _lanes(m)
    where = lanes[:, :, 0] != NONE
    lanes[:, :, 1] = (lanes[:, :, 1].copy().view(np.float32) * np.float32(8.0)).view(np.uint32)
    _rejected(fam, m, "lane's weight outside its bound", where)
    if n == 128:  # index 127 -> 126
        m = _mutated(fam)
        cont = m[:, 9:17].astype(np.int64)
        where = (((cont >> 1) & 0xFF) == 127) & ((cont >> 9) > 0)
        m[:, 9:17] = np.where(where, (cont & ~(0xFF << 1)) | (126 << 1), cont).astype(np.uint32)
        fail, _ = t.check(m)
        caught = fail["pick differs from the truth's on a decisive lane"] | fail["probability word is not the picked child's"] | fail["picked child without importance"]
        assert where.sum() > 20 and caught[where].all()
        assert fail["pick differs from the truth's on a decisive lane"][where & t.decisive].all() and (where & t.decisive).any()


@pytest.mark.parametrize("n", [8, 257])
def test_mutated_candidate_answers_are_rejected(n):
    fam = family(n)
    # mis <-> 1 - mis
    m = _mutated(fam)
    lanes = _lanes(m)
    mis = lanes[:, :, 15].copy().view(np.float32)
    where = (lanes[:, :, 2] == lt.EVALUATED) & (np.abs(mis - 0.5) > 1e-3) & (_lanes(fam.oracle.reshape(-1, lt.WORDS))[:, :, 6].copy().view(np.float32) > 1e-6)
    lanes[:, :, 15] = np.where(where, (np.float32(1.0) - mis).view(np.uint32), lanes[:, :, 15])
    _rejected(fam, m, "MIS weight beyond", where)
    # self not skipped
    m = _mutated(fam)
    lanes = _lanes(m)
    where = lanes[:, :, 2] == lt.SELF
    lanes[:, :, 2] = np.where(where, lt.EVALUATED, lanes[:, :, 2])
    _rejected(fam, m, "self not skipped", where)
    if n == 257:  # the handle of light 255 answered for light 256: the vertex that names light 255 as self skips light 256, the light it stands on
        m = _mutated(fam)
        lanes = _lanes(m)
        where = (lanes[:, :, 0] == 256) & (fam.tags == "wrong_self")[fam.rows][:, None]
        assert where.sum() >= 10 and (lanes[:, :, 2][where] != lt.SELF).all()
        lanes[:, :, 2] = np.where(where, lt.SELF, lanes[:, :, 2])
        lanes[:, :, 3:] = np.where(where[:, :, None], 0, lanes[:, :, 3:])
        _rejected(fam, m, "skipped as self although it is not", where)
    # a word that is no number, stage by stage
    oracle_lanes = _lanes(fam.oracle.reshape(-1, lt.WORDS))
    evaluated = oracle_lanes[:, :, 2] == lt.EVALUATED
    for word, name in ((3, "ray"), (6, "solid angle"), (7, "dist"), (8, "colour"), (12, "BSDF weight"), (14, "direction probability"), (15, "MIS weight"), (16, "target")):
        for bits in (0x7FC00000, 0x7F800000):
            m = _mutated(fam)
            lanes = _lanes(m)
            lanes[:, :, word] = np.where(evaluated, np.uint32(bits), lanes[:, :, word])
            _rejected(fam, m, "non-finite word of an evaluated lane", evaluated)
    # ... and a kernel whose every target is a NaN and which therefore returns no sample
    m = _mutated(fam)
    lanes = _lanes(m)
    lanes[:, :, 16] = np.where(evaluated, np.uint32(0x7FC00000), lanes[:, :, 16])
    m[:, 0], m[:, 1:8] = NONE, 0
    _rejected(fam, m, "non-finite word of an evaluated lane", evaluated)
    m = _mutated(fam)
    m[:, 4] = 0x7FC00000
    _rejected(fam, m, "non-finite word of the sample or the root pass", np.ones(len(m), dtype=bool))
    # refr_prob 0 on a translucent vertex: the reflection's probability is not halved
    m = _mutated(fam)
    lanes = _lanes(m)
    translucent = ((fam.vertices.flags & 1) != 0)[fam.rows][:, None]
    dirp = lanes[:, :, 14].copy().view(np.float32)
    where = (lanes[:, :, 2] == lt.EVALUATED) & translucent & (dirp > 0) & (_lanes(fam.oracle.reshape(-1, lt.WORDS))[:, :, 6].copy().view(np.float32) > 1e-6)
    rays = lanes[:, :, 3:6].copy().view(np.float32).astype(np.float64)
    where &= np.sum(rays * fam.truth.nrm[fam.rows][:, None, :], axis=-1) > 0   # reflections
    lanes[:, :, 14] = np.where(where, (dirp * np.float32(2.0)).view(np.uint32), lanes[:, :, 14])
    _rejected(fam, m, "direction probability relative beyond", where)


def test_binary32_models_of_the_root_scan_keep_the_truths_pick_on_decisive_lanes():
    """4000 scans of 8 .. 128 children: the reference form, the same with reciprocals one ulp off, the threshold form, and the threshold form with the 7-bit key
    (tests/test_root_pass_forms.py) against the truth's scan of the same binary32 importances. This validates the bound before a kernel is involved."""
    rng = np.random.RandomState(11)
    n_cases, K = 4000, 128
    ws = np.zeros((K, n_cases))
    us = np.zeros((n_cases, 1))
    cases = []
    for i in range(n_cases):
        n = rng.randint(8, 129)
        w = (rng.gamma(0.5, 1.0, n) * (rng.rand(n) > 0.1)).astype(np.float32)
        u = np.float32(rng.rand())
        ws[:n, i], us[i, 0] = w, u
        cases.append((w, u))
    pick, dec, T, eT, _, _ = lt.scan(ws, np.zeros_like(ws), us)
    pick, dec = pick[:, 0], dec[:, 0]
    off = {"reference": 0, "reference, reciprocals off": 0, "threshold": 0, "threshold with key": 0}
    for i, (w, u) in enumerate(cases):
        got = {"reference": forms.reference_form(w, u, np.float32), "reference, reciprocals off": forms.reference_form(w, u, np.float32, recip_ulps=1),
               "threshold": forms.threshold_form(w, u, np.float32), "threshold with key": forms.threshold_form_key(w, u)[0]}
        for k, g in got.items():
            off[k] += g != pick[i]
            assert not dec[i] or g == pick[i], "scan %d (%d children, u = %r): the %s form picks %d, the truth %d on a decisive lane" % (i, len(w), float(u), k, g, pick[i])
    print("decisive share %.4f of %d scans | binary32 picks off the truth's over all scans: %s" % (dec.mean(), n_cases, off))
    assert dec.mean() > 0.25
    # the key carries the picked importance to 2^-16 of itself
    w, u = cases[0]
    k, target = forms.threshold_form_key(w, u)
    assert abs(float(target) - float(w[k])) <= 2.0 ** -16 * float(w[k])


# ---- GPU ----
def _device_runs(fam, flavour):
    """the probe's words in the general form and - where the shading kernel would take it - the plain form's on the vertices it can meet (spliced into the general
    answer: the plain form never shades a translucent vertex), and with nothing staged"""
    from luminary_amd.core import Core
    core = Core(0)
    try:
        core.upload(fam.view)
        core.set_flavour(flavour)
        w = fam.vertices.words()
        general = core.light_sample_probe_host(w, 0, SAMPLES, "general")
        unstaged = core.light_sample_probe_host(w, 0, SAMPLES, "unstaged")
        plain = None
        if core.get_plain_form():
            opaque = (fam.vertices.flags & 1) == 0
            plain = general.copy()
            plain[opaque] = core.light_sample_probe_host(w[opaque], 0, SAMPLES, "plain")
    finally:
        core.close()
    return general, unstaged, plain


@pytest.mark.gpu
@pytest.mark.parametrize("n", COUNTS)
def test_gpu_light_samples_against_the_truth(n):
    fam = family(n)
    _, stick = yardstick(n)
    e_general, e_unstaged, e_plain = _device_runs(fam, "exact")
    f_general, f_unstaged, f_plain = _device_runs(fam, "fast")
    assert (e_plain is not None) == (n <= 128), "the plain form shades the flat trees whose lights are all staged"
    for name, got in (("general", e_general), ("unstaged", e_unstaged), ("plain", e_plain)):
        if got is not None:
            diff = got != fam.oracle
            assert not diff.any(), "%d lights, exact flavour, %s form: %d words differ from the oracle's probes, first at (vertex, sample, word) %s" % (
                n, name, int(diff.sum()), np.argwhere(diff)[:5].tolist())
    assert np.array_equal(f_general, f_unstaged), "fast flavour: a light read from LDS and the same light read from memory give different words"
    worst = 0.0
    for flavour, runs in (("exact", (e_general, e_plain)), ("fast", (f_general, f_plain))):
        for name, got in zip(("general", "plain"), runs):
            if got is None:
                continue
            fail, fig = fam.truth.check(got, yardstick=stick, factor=4.0, bsdf_reference=_bsdf_reference(fam, got),
                                        bsdf_tolerance=(4.0 * FAST_MEASURED) if FAST_MEASURED is not None else None, luts=oracle_lib.golden_luts())
            print("%d lights, %s flavour, %s form: %s" % (n, flavour, name, ", ".join("%s %.3g" % kv for kv in sorted(fig.items()))))
            if flavour == "fast":
                _record("fast", "%d %s" % (n, name), fig)
                worst = max(worst, fig["BSDF weight relative to the oracle"])
            assert not any(b.any() for b in fail.values()), "%d lights, %s flavour, %s form rejected:\n%s" % (n, flavour, name, _describe(fam, fail))
    print("%d lights: fast flavour's largest relative distance of a BSDF weight from the oracle %.4g" % (n, worst))
    assert FAST_MEASURED is not None, "not yet measured on the GPU"


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["flat 12 lights", "300 lights"])
def test_gpu_fast_flavour_resampling_weights_are_unbiased(which):
    """test_oracle_analytic.test_light_tree_resampling_weights_are_unbiased on the device's fast flavour: E[sum over the lanes of weight * g(light)] = sum over the
    lights of g, for g = 1 and g = the indicator of each of the four most probable lights; the oracle's figures on the same inputs beside them."""
    from luminary_amd.core import Core
    if which == "300 lights":
        view = family(300).view
        points = (((0.0, 0.5, 0.0), (0.0, 1.0, 0.0)), ((6.0, 1.0, -4.0), (0.0, 1.0, 0.0)))
    else:
        host = scenes.example_scene(32, 18, 2, sphere_segments=6, ground_res=4, num_objects=6, num_lights=6)
        view = oracle_lib.with_luts(host.device_scene())
        assert view.num_lights == 12
        points = (((0.0, 0.5, 0.0), (0.0, 1.0, 0.0)), ((6.0, 1.0, -4.0), (0.0, 1.0, 0.0)))
    n = 40_000
    v = lt.Vertices([p for p, _ in points], [nr for _, nr in points], [(0.3, 0.9, 0.1)] * 2, [(0.8, 0.8, 0.8)] * 2, [1.0] * 2, [0.7] * 2, [1.0] * 2, [0] * 2,
                    [(0xFFFFFFF0, 0)] * 2, [(4, 9)] * 2)
    core = Core(0)
    try:
        core.upload(view)
        core.set_flavour("fast")
        got = core.light_sample_probe_host(v.words(), 0, n, "general")
    finally:
        core.close()
    ref = oracle_lib.light_sample_stages(view, v.words(), 0, n)
    for k in range(2):
        figures = []
        for out in (got[k], ref[k]):
            lanes = out[:, lt.HEAD:].reshape(n, lt.LANES, lt.LANE_WORDS)
            ids, w = lanes[:, :, 0], lanes[:, :, 1].copy().view(np.float32)
            valid = ids != NONE
            assert valid.any()
            chosen = np.unique(ids[valid])
            total = float((w * valid).sum(axis=1).mean())
            freq = np.array([(ids == l).mean() for l in chosen])
            top = chosen[np.argsort(-freq)[:4]]
            figures.append((total, len(chosen), [(int(l), float((w * (ids == l)).sum(axis=1).mean())) for l in top]))
        print("%s, vertex %d: device sum of weights %.4f for %d lights, per light %s | oracle %.4f for %d, %s" % ((which, k) + figures[0] + figures[1]))
        total, count, per_light = figures[0]
        assert abs(total - count) < 0.05 * count, (total, count)
        # the device reaches the lights the oracle reaches: a light that one of them chose 30 times and more in 320 000 lanes (the other expects as many: none
        # at all has a probability below e^-30) is chosen by both - self-consistent weights over a smaller set of lights would pass the sums above
        counts = []
        for out in (got[k], ref[k]):
            ids = out[:, lt.HEAD:].reshape(n, lt.LANES, lt.LANE_WORDS)[:, :, 0]
            counts.append(np.bincount(ids[ids != NONE].astype(np.int64), minlength=view.num_lights))
        often = (counts[0] >= 30) | (counts[1] >= 30)
        both = (counts[0] > 0) & (counts[1] > 0)
        assert often.sum() >= 6 and both[often].all(), np.nonzero(often & ~both)[0]
        for l, est in per_light:
            assert abs(est - 1.0) < 0.05, (l, est)
