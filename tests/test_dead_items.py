"""Items that end where they are loaded, in launches large enough for the work distribution of the persistent ray kernels to matter (dev_trace.h trace_items).

A wave reserves chunks of consecutive items and hands them to its idle lanes. A *dead* item ends at the load: a ray with a non-finite origin or direction
(k_trace_rays, k_shadow_rays, k_trace: ended as a miss), or a path that the query declines (k_trace_particles: every non-delta path). A wave that is handed 64 dead
items has nothing live afterwards; it must still trace the rest of its chunk and take further chunks. It used to leave the kernel instead, so beyond
waves x chunk items - 262 144 on a part of 4096 resident waves - the tail of a queue was traced only if enough waves survived, and from 532 480 items on (chunk
128) the second half of such a chunk was dropped outright (profiles/multi_round_pass_reproducibility.txt).

Every GPU parity test renders a few thousand paths; these launches hold 600 000 to a million items, almost all dead, around 4096 live ones:
  dead_prefix         2^20 dead items - at least waves x chunk for any chunk this n gives - then the 4096 live ones
  alternating_runs    runs of dead and of live items of 64, 65, 127, 128 and 192 items, aligned with and straddling the 64-item hand-outs; about 600 000 items
  all_dead_but_last   2^20 dead items and one live one
and the reference launch is the 4096 live items alone. Held: every item is answered (the outputs start as a sentinel), a dead ray gets the miss answer the
oracle gives it and a dead particle item stays untouched, every live item's words equal the same item's words from the reference launch bit for bit - a ray's
answer does not depend on the launch it is in - and in the exact flavour the live items equal the oracle bit for bit. The particle probe's first 40 answers
also pass the float64 brute force over the 25^3 cells (tests/particle_truth.py), in both flavours.

Scenes: the zoo (two-level kernels) and a small hall (one instance under the identity: the single-level forms in both flavours, and the coherent form by name)."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib
import particle_truth
from luminary_amd import scenes
from luminary_amd.core import Core

pytestmark = pytest.mark.gpu
FLAVOURS = ["exact", "fast"]
LIVE = 4096
PREFIX = 1 << 20
RUNS = (64, 65, 127, 128, 192)
SENTINEL = 0xDEADBEEF       # no instance, triangle or distance word of a scene this small
PARTICLE_SCALE = 4.0        # a power of two: origin / scale is exact whatever the flavour does with the reciprocal
HIT_PARTICLE_MIN = 0x80000000


# ---- layouts: (n, position of every live slot, the live item it holds) ----
def _layout(name):
    if name == "reference":
        return LIVE, np.arange(LIVE), np.arange(LIVE)
    if name == "dead_prefix":
        return PREFIX + LIVE, PREFIX + np.arange(LIVE), np.arange(LIVE)
    if name == "all_dead_but_last":
        return PREFIX + 1, np.array([PREFIX]), np.array([0])
    assert name == "alternating_runs"
    pos, at, run = [], 0, 0
    while at < 600_000:
        length = RUNS[run % len(RUNS)]
        if run % 2 == 1:  # dead, live, dead ... : ten runs until a length comes back in the same role
            pos.append(np.arange(at, at + length))
        at, run = at + length, run + 1
    pos = np.concatenate(pos)
    assert 532_480 < at < 700_000 and 250_000 < len(pos) < 350_000  # the chunk is 128 items; about half the items are live
    return at, pos, np.arange(len(pos)) % LIVE


LAYOUTS = ["dead_prefix", "alternating_runs", "all_dead_but_last"]


def _spread(live, dead, name):
    """The layout's arrays: the dead items (cycled) everywhere, the live ones at their slots. live / dead: tuples of arrays with the item on axis 0."""
    n, pos, item = _layout(name)
    out = []
    for lv, dd in zip(live, dead):
        a = np.ascontiguousarray(np.resize(dd, (n,) + dd.shape[1:]))
        a[pos] = lv[item]
        out.append(a)
    return n, pos, item, out


# ---- scenes and items, made once ----
@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "zoo":
        host = scenes.zoo_scene(64, 40, 5)
        p = host.get_particles()
        p.active, p.count, p.size, p.scale, p.speed, p.seed, p.phase_diameter = True, 48, 60.0, PARTICLE_SCALE, 0.0, 5, 50.0
        host.set_particles(p)
        eye = np.array([0.5, 3.2, 13.0])
    else:
        host = scenes.hall_scene(64, 40, 4, target_triangles=6000)
        eye = np.array([-40.0, 4.0, 0.0])
    return host, oracle_lib.with_luts(host.device_scene()), eye


@functools.lru_cache(maxsize=None)
def _rays(scene):
    """4096 finite rays from around the camera into and past the scene, their visibility segments, and the dead rays: the same rays with one component replaced
    by a NaN (direction) or an infinity (origin)."""
    _, _, eye = _scene(scene)
    rng = np.random.RandomState(11)
    o = (eye[None, :] + rng.uniform(-1.5, 1.5, (LIVE, 3))).astype(np.float32)
    half, centre, reach = ((10.0, 4.0, 10.0), (0.0, 2.0, 0.0), 40.0) if scene == "zoo" else ((48.0, 6.0, 14.0), (0.0, 6.0, 0.0), 90.0)
    target = rng.uniform(-1.0, 1.0, (LIVE, 3)) * np.array(half) + np.array(centre)
    d = target - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    dist = rng.uniform(1.0, reach, LIVE).astype(np.float32)
    ids = np.full((LIVE, 4), 0xFFFFFFFF, dtype=np.uint32)
    do, dd = o.copy(), d.copy()
    k = np.arange(LIVE) % 4
    dd[k == 0, 1] = np.nan
    do[k == 1, 0] = np.inf
    dd[k == 2, 2] = np.float32(-np.nan)
    do[k == 3, 2] = -np.inf
    assert np.isfinite(o).all() and np.isfinite(d).all() and not (np.isfinite(do).all(axis=1) & np.isfinite(dd).all(axis=1)).any()
    return (o, d, dist, ids), (do, dd, dist, ids)


@functools.lru_cache(maxsize=None)
def _closest_truth(scene):
    """The oracle's answers: to the live rays, and THE miss answer it gives to the dead ones."""
    _, view, _ = _scene(scene)
    live, dead = _rays(scene)
    want = oracle_lib.trace_closest(view, live[0], live[1])
    miss = oracle_lib.trace_closest(view, dead[0][:8], dead[1][:8])
    assert (miss == miss[0]).all() and miss[0, 0] == 0xFFFFFFFE and miss[0, 2] == np.float32(np.finfo(np.float32).max).view(np.uint32)
    assert 0.3 < (want[:, 0] != 0xFFFFFFFE).mean(), "the live rays are to hit the scene"
    return want, miss[0]


@functools.lru_cache(maxsize=None)
def _visibility_truth(scene):
    _, view, _ = _scene(scene)
    live, dead = _rays(scene)
    want = oracle_lib.trace_shadow(view, *live)
    miss = oracle_lib.trace_shadow(view, dead[0][:8], dead[1][:8], dead[2][:8], dead[3][:8])
    assert (miss == 1.0).all()
    blocked = (want == 0.0).all(axis=1).mean()
    assert 0.1 < blocked < 0.9, blocked
    return want, miss[0]


@functools.lru_cache(maxsize=None)
def _particle_items():
    """4096 delta paths through the lattice, and the dead items: the same entries without the delta flag."""
    rng = np.random.RandomState(23)
    o = rng.uniform(-20.0, 20.0, (LIVE, 3)).astype(np.float32)
    d = rng.normal(size=(LIVE, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    tmax = rng.uniform(5.0, 60.0, LIVE).astype(np.float32)
    pixel_samples = np.stack([rng.randint(0, 64, LIVE), rng.randint(0, 40, LIVE), rng.randint(0, 64, LIVE)], axis=1).astype(np.uint32)
    delta = np.where(np.arange(LIVE) % 2 == 0, 1, 1 | 8 | 16).astype(np.uint32)      # delta path, alone and beside other flags
    other = np.where(np.arange(LIVE) % 2 == 0, 0, 2 | 8 | 16).astype(np.uint32)      # no delta path
    return (o, d, tmax, delta, pixel_samples), (o, d, tmax, other, pixel_samples)


def _lattice_rays():
    """What ParticleQuery::load makes of the live items at speed 0: frac(origin / scale) and direction / scale, in float32."""
    o, d, tmax, _, _ = _particle_items()[0]
    inv = np.float32(1.0) / np.float32(PARTICLE_SCALE)
    p = o * inv
    return (p - np.floor(p)).astype(np.float32), (d * inv).astype(np.float32), tmax


@functools.lru_cache(maxsize=None)
def _particle_truth():
    """The oracle's lattice tracer on the live items as (t, hit word), and the float64 brute force's answers to the first 40."""
    _, view, _ = _scene("zoo")
    pos, d, tmax = _lattice_rays()
    out_t, out_tri = np.zeros(LIVE, dtype=np.float32), np.zeros(LIVE, dtype=np.uint32)
    oracle_lib.lib().oracle_probe_particle_trace(C.byref(view), C.c_uint32(LIVE), pos.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                                 tmax.ctypes.data_as(C.c_void_p), out_t.ctypes.data_as(C.c_void_p), out_tri.ctypes.data_as(C.c_void_p))
    hit = np.where(out_tri == particle_truth.NO_TRIANGLE, Core.PARTICLE_PROBE_UNTOUCHED, HIT_PARTICLE_MIN + (out_tri >> 1)).astype(np.uint32)
    assert 0.3 < (out_tri != particle_truth.NO_TRIANGLE).mean() < 0.999
    brute = particle_truth.brute_force(particle_truth.particle_triangles(view), pos[:40], d[:40], tmax[:40])
    return out_t, hit, brute


def _core(scene, flavour, single_level=-1, coherent=-1):
    core = Core(0)
    try:
        core.set_flavour(flavour)
        core.set_single_level(single_level)
        core.set_coherent_first_hits(coherent)
        core.upload(_scene(scene)[1])
    except Exception:
        core.close()
        raise
    return core


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _closest(core, o, d):
    """lumc_trace_closest on device buffers of the test's own, the answers pre-filled with the sentinel (the host entry point allocates its output itself)."""
    hip = C.CDLL("libamdhip64.so.7")  # the runtime the library is linked to, already loaded with it
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    n = len(o)
    out = np.full((n, 3), SENTINEL, dtype=np.uint32)
    host = [np.ascontiguousarray(o, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32), out]
    assert host[0].shape == host[1].shape == (n, 3)
    device = []
    try:
        for a in host:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), a.nbytes) == 0 and p.value
            device.append(p)
            assert hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice
        core.trace_closest_device(n, device[0].value, device[1].value, 0, device[2].value)
        core.synchronize()
        assert hip.hipMemcpy(out.ctypes.data, device[2], out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    finally:
        for p in device:
            assert hip.hipFree(p) == 0
    return out


def _held(what, got, pos, item, reference, dead_answer, unanswered):
    """got [n, words] uint32. Everything answered; the live slots equal the reference launch's answers to the same items; every other slot holds the dead answer."""
    assert not unanswered.any(), "%s: %d of %d items were never answered, the first at %d" % (what, unanswered.sum(), len(got), np.argmax(unanswered))
    live = np.zeros(len(got), dtype=bool)
    live[pos] = True
    wrong = (got[~live] != dead_answer[None, :]).any(axis=1)
    assert not wrong.any(), "%s: %d dead items without the dead answer, the first %s" % (what, wrong.sum(), got[~live][np.argmax(wrong)])
    differ = (got[pos] != reference[item]).any(axis=1)
    assert not differ.any(), "%s: %d of %d live items differ from the launch of the live items alone, the first at slot %d" % (
        what, differ.sum(), len(pos), pos[np.argmax(differ)])


# scene, single level, coherent: the two-level kernel; the single-level one; the same scene with the form switched off; the coherent form asked for by name
CLOSEST_FORMS = {"two_level": ("zoo", -1, 0), "single_level": ("hall", 1, 0), "single_level_off": ("hall", 0, 0), "coherent": ("hall", 1, 1)}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("form", list(CLOSEST_FORMS))
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_closest_hits_among_dead_rays(flavour, form, layout):
    scene, single_level, coherent = CLOSEST_FORMS[form]
    live, dead = _rays(scene)
    want, miss = _closest_truth(scene)
    core = _core(scene, flavour, single_level, coherent)
    try:
        assert core.get_single_level() == (0 if form in ("two_level", "single_level_off") else 1), "the scene is to run the form under test"
        reference = _closest(core, live[0], live[1])
        n, pos, item, (o, d) = _spread(live[:2], dead[:2], layout)
        got = _closest(core, o, d)
    finally:
        core.close()
    assert not (reference == SENTINEL).any()
    if flavour == "exact":
        differ = (reference != want).any(axis=1)
        assert not differ.any(), "%d of %d live rays differ from the oracle" % (differ.sum(), LIVE)
    _held("%s, %s, %s" % (flavour, form, layout), got, pos, item, reference, miss, (got == SENTINEL).any(axis=1))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("scene", ["zoo", "hall"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_visibility_among_dead_rays(flavour, scene, layout):
    live, dead = _rays(scene)
    want, miss = _visibility_truth(scene)
    core = _core(scene, flavour)
    try:
        assert core.get_single_level() == (1 if scene == "hall" else 0)
        reference = core.trace_visibility_host(*live)
        n, pos, item, arrays = _spread(live, dead, layout)
        got = core.trace_visibility_host(*arrays)
    finally:
        core.close()
    assert np.isfinite(reference).all()
    if flavour == "exact":
        differ = (_bits(reference) != _bits(want)).any(axis=1)
        assert not differ.any(), "%d of %d live rays differ from the oracle" % (differ.sum(), LIVE)
    _held("%s, %s, %s" % (flavour, scene, layout), _bits(got), pos, item, _bits(reference), _bits(miss), ~np.isfinite(got).all(axis=1))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_particle_hits_among_paths_that_see_no_particles(flavour, layout):
    live, dead = _particle_items()
    want_t, want_hit, brute = _particle_truth()
    core = _core("zoo", flavour)
    try:
        ref_t, ref_hit = core.trace_particles_probe(*live)
        n, pos, item, arrays = _spread(live, dead, layout)
        got_t, got_hit = core.trace_particles_probe(*arrays)
    finally:
        core.close()
    if flavour == "exact":
        differ = (ref_hit != want_hit) | (_bits(ref_t) != _bits(want_t))
        assert not differ.any(), "%d of %d live items differ from the oracle" % (differ.sum(), LIVE)
    tri = np.where(ref_hit[:40] == Core.PARTICLE_PROBE_UNTOUCHED, particle_truth.NO_TRIANGLE, ref_hit[:40] - np.uint32(HIT_PARTICLE_MIN))
    assert particle_truth.check_against_brute_force(brute, ref_t[:40], tri, per_particle=True) >= 10
    # a dead item is untouched: the sentinel and its own tmax; a live one that hit nothing is too, which the reference launch says of the same item
    live_slot = np.zeros(n, dtype=bool)
    live_slot[pos] = True
    touched = ~live_slot & ((got_hit != Core.PARTICLE_PROBE_UNTOUCHED) | (_bits(got_t) != _bits(arrays[2])))
    assert not touched.any(), "%d paths that are no delta paths were touched" % touched.sum()
    differ = (got_hit[pos] != ref_hit[item]) | (_bits(got_t[pos]) != _bits(ref_t[item]))
    assert not differ.any(), "%s, %s: %d of %d live items differ from the launch of the live items alone (%d of them untouched), the first at slot %d" % (
        flavour, layout, differ.sum(), len(pos), (differ & (got_hit[pos] == Core.PARTICLE_PROBE_UNTOUCHED)).sum(), pos[np.argmax(differ)])
