"""The coherent form of the single-level closest-hit kernel (csrc/device/dev_trace.h trace_items<Q, true, true>, visit_node_uniform;
lumc_set_coherent_first_hits): where every live lane of a wave stands on the same inner node with the same direction signs the wave fetches the node once
through the scalar unit; anywhere else the turn of the phase loop is the plain one. Per ray the same nodes and triangles in the same order, so the hits
(instance, triangle, t) and the counters (rays, node visits, triangle tests, LDS-served visits) of the two forms are EQUAL, word for word, in both flavours, with
the tree's top staged in LDS and without (LUM_LDS_NODES=0: every uniform visit goes through the constant address space).

The rays go through the closest-hit entry the single-level tests use (lumc_trace_closest_host; mode 1 of the switch gives it the coherent kernel). A wave of that
kernel takes 64 consecutive rays, and only when all its lanes are idle, so the arrays below are built wave by wave:
  identical    64 copies of one ray: the test holds at every node of the walk
  split k      32 lanes of a ray A interleaved with 32 of a ray B that visits the same k inner nodes first and another one next, for k = 1, 5 and 12: the wave makes k
               visits as one and hands over to the plain turn with the stacks the uniform visits built. k is not hoped for but computed: tests/single_level_walk.py walks
               the uploaded node array on the host by the kernel's rules (child order, culling pops, shrinking tmax) and B is taken where its walk
               shares exactly k visits with A's (k = 5, 12: the first such turn of A; k = 1: a pair from beside the scene), in A's octant, with every decision of both walks at least 1e-4 (relative) away from going the other way - far beyond what the
               device's arithmetic differs by. The device's hits of both halves must be the triangles the walks end on
  split        the same interleaving with A turned by 28 angles from 1e-7 to 0.7 rad, one wave per angle: whatever prefixes those give
  octant       63 equal rays and one mirrored in x, y or z: same root, other plane offsets - the test must fail on the signs alone
  one lane     one finite ray among 63 non-finite ones, which end where they are loaded
  non-finite   NaN and infinite origins and directions among equal finite rays
  ignore       64 equal rays, one of which ignores the triangle the others hit
  pixel        64 rays of one origin in a cone of a pixel's width, as the renderer's depth-0 waves are
  cut-out      equal and pixel-like rays through a fence of alpha-0 texels in front of the wall
and one launch of 37 rays. The hit's scene-triangle word with its flags is not an output of that entry: it reaches the frame through the fast flavour's ambient
reuse, so the renderer's frames and counters with the form on and off are compared as well, and the overlapped schedule must still be taken."""
import functools

import numpy as np
import pytest

import single_level_walk
from luminary_amd import Host, scenes
from luminary_amd.core import CNT_LIGHT_BVH, CNT_NODES, CNT_NODES_LDS, CNT_SHADOW, CNT_TRACE, CNT_TRIS, CNT_VERTICES, Core

FLAVOURS = ["fast", "exact"]
SKY = 0xFFFFFFFE
EYE = np.float32([0.3, 2.0, 9.0])


def _fence_host(width=64, height=32, bounces=3):
    """One mesh under the identity (what both flavours walk in the single-level form): a wall of 2 x 40 x 40 triangles, a floor, a box, an emissive panel and,
    in front of the wall, a fence whose texture has alpha-0 gaps between opaque slats."""
    host = Host()
    scenes.apply_benchmark_settings(host, width, height, bounces, sky=(0.5, 0.6, 0.8))
    fence = np.zeros((8, 8, 4), dtype=np.uint8)
    fence[..., :3] = (180, 140, 90)
    fence[:, ::2, 3] = 255
    tex = host.add_texture(fence)
    grey = host.add_material(scenes._material((0.6, 0.6, 0.6), 0.6))
    glow = host.add_material(scenes._material((0.8, 0.8, 0.8), 0.7, emission=(12.0, 11.0, 9.0)))
    slats = scenes._material((0.5, 0.5, 0.5), 0.6)
    slats.albedo_tex = tex
    slats = host.add_material(slats)
    wall = scenes._grid(40, 40, -6, 6, -1, 7, lambda x, z: 0.2 * np.sin(1.7 * x) * np.cos(1.1 * z))
    wall = wall.reshape(-1, 3, 3)[:, :, [0, 2, 1]].reshape(-1, 9) + np.tile(np.float32([0.0, 0.0, -5.0]), 3)  # stood up (y and z swapped), 5 behind the origin
    floor = scenes._grid(12, 12, -6, 6, -5, 8, lambda x, z: 0.1 * np.sin(1.3 * x) * np.cos(0.9 * z))
    box = scenes._box()[0] * 0.9 + np.tile(np.float32([-2.5, 0.9, 1.0]), 3)
    panel = np.float32([[-1.5, 6.5, -1.5, 1.5, 6.5, 1.5, 1.5, 6.5, -1.5], [-1.5, 6.5, -1.5, -1.5, 6.5, 1.5, 1.5, 6.5, 1.5]])
    fpos, fuv = scenes._quad_uv((0.5, 0.2, 2.0), (4.5, 0.2, 2.0), (4.5, 3.8, 2.0), (0.5, 3.8, 2.0), rep=3.0)
    plain = np.concatenate([wall, floor, box, panel]).astype(np.float32)
    pos = np.concatenate([plain, fpos]).astype(np.float32)
    uvs = np.concatenate([np.zeros((len(plain), 6), np.float32), fuv]).astype(np.float32)
    mats = np.concatenate([np.full(len(wall) + len(floor) + len(box), grey), np.full(len(panel), glow), np.full(len(fpos), slats)]).astype(np.uint16)
    host.fence_first_triangle = len(plain)  # the fence's two triangles are the mesh's last
    host.new_instance(host.add_mesh(pos, mats, uvs=uvs))
    scenes.set_camera(host, tuple(float(v) for v in EYE), (-0.05, 0.0, 0.0), fov=0.9)
    return host


@functools.lru_cache(maxsize=None)
def _scene():
    host = _fence_host()
    return host.device_scene(), host.fence_first_triangle, host


def _view():
    return _scene()[0]


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _towards(target):
    return _unit(np.float32(target) - EYE)


def _turned(d, angle, axis=(0.3, 1.0, 0.2)):
    """d turned by `angle` about `axis` (Rodrigues, float64)"""
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    d = np.asarray(d, np.float64)
    return _unit(d * np.cos(angle) + np.cross(k, d) * np.sin(angle) + k * np.dot(k, d) * (1.0 - np.cos(angle)))


def _wave(origins, dirs):
    o, d = np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(dirs, np.float32).reshape(-1, 3)
    assert o.shape == d.shape == (64, 3)
    return o, d


def _equal(direction, origin=EYE):
    return _wave(np.tile(origin, (64, 1)), np.tile(direction, (64, 1)))


def _pixel(direction, rng, width=2e-3):
    d = np.tile(direction, (64, 1)).astype(np.float64) + rng.uniform(-width, width, (64, 3))
    return _wave(np.tile(EYE, (64, 1)), _unit(d))


SPLITS = (1, 5, 12)
MARGIN = 1e-4  # relative distance of every decision of a host walk from its other outcome; the device's fma / v_rcp arithmetic differs from the walk's by ~1e-7
# (origin, A, the Bs to try) per k. k = 1: the root's children overlap around the camera, so from there every ray of an octant enters the same child first; the pair
# starts beside the scene, A down onto the floor, B along it to the wall. k = 5: from the camera to the wall (ten visits), B among turns of A. k = 12: grazing along the
# wavy wall (nineteen visits), B among turns of A about the vertical.
_ANGLES = np.concatenate([np.geomspace(1e-6, 1e-2, 120), np.linspace(1e-2, 0.3, 60)[1:]])


def _turns(a, axis):
    return [_turned(a, signed, axis) for angle in _ANGLES for signed in (angle, -angle)]


def _split_cases():
    to_wall, grazing = _towards((-3.0, 2.5, -5.0)), np.float32([0.99229467, -0.11711468, -0.04044035])
    return ((1, np.float32([5.5396085, 2.2082443, 0.044274]), np.float32([-0.4242402, -0.7353367, -0.5284885]), [np.float32([-0.0622131, -0.02664067, -0.99770725])]),
            (5, EYE, to_wall, _turns(to_wall, (0.3, 1.0, 0.2))),
            (12, np.float32([-5.400518, 5.3581214, -4.639689]), grazing, _turns(grazing, (0.0, 1.0, 0.0))))


@functools.lru_cache(maxsize=None)
def _split_waves():
    """For k in SPLITS: origin, A, B and the triangles their host walks end on - B the first candidate whose walk shares exactly k inner-node visits with A's and then
    visits another node, in A's octant, both walks robust (MARGIN) and clear of the fence's cut-outs."""
    tree = single_level_walk.scene_tree(_view())
    textures = int(_view().num_textures)
    found = []
    for k, origin, a, candidates in _split_cases():
        seq_a, margin_a, textured_a, hit_a = single_level_walk.walk(tree, origin, a, textures)
        assert margin_a >= MARGIN and not textured_a and len(seq_a) > k, (k, margin_a, textured_a, len(seq_a))
        for b in candidates:
            if (np.signbit(b) != np.signbit(a)).any() or (b == 0.0).any():
                continue
            seq_b, margin_b, textured_b, hit_b = single_level_walk.walk(tree, origin, b, textures)
            if single_level_walk.shared_visits(seq_a, seq_b) == k and margin_b >= MARGIN and not textured_b and len(seq_b) > k:
                found.append({"k": k, "origin": origin, "a": a, "b": b, "hit_a": hit_a, "hit_b": hit_b})
                break
        else:
            raise AssertionError("no ray shares exactly %d visits with A" % k)
    return found


def test_the_split_waves_share_exactly_1_5_and_12_visits():
    """No GPU: the host walk's own statement about the waves the GPU test traces (and the search's result does not depend on the order it looked in)."""
    tree = single_level_walk.scene_tree(_view())
    for s in _split_waves():
        walks = [single_level_walk.walk(tree, s["origin"], s[ray], int(_view().num_textures)) for ray in ("a", "b")]
        assert single_level_walk.shared_visits(walks[0][0], walks[1][0]) == s["k"] and min(walks[0][1], walks[1][1]) >= MARGIN
        first_apart = next(i for i, (x, y) in enumerate(zip(walks[0][0], walks[1][0])) if x != y)
        print("k = %d: %d / %d turns, apart from turn %d on (%#x | %#x), hits %s | %s" % (s["k"], len(walks[0][0]), len(walks[1][0]), first_apart,
                                                                                          walks[0][0][first_apart], walks[1][0][first_apart], s["hit_a"], s["hit_b"]))
        assert (np.signbit(s["a"]) == np.signbit(s["b"])).all(), "one octant: the uniform test fails on the node, not on the signs"


@functools.lru_cache(maxsize=None)
def _waves():
    """(origins [64 W, 3], directions, {family: range of waves})"""
    rng = np.random.RandomState(5)
    wall_targets = [(-3.0, 2.5, -5.0), (0.1, 4.0, -5.0), (2.2, 0.7, -5.0), (5.5, 6.5, -5.0), (-2.5, 0.9, 1.0), (0.0, 0.0, 3.0), (0.0, 30.0, 0.0)]  # wall, box, floor, sky
    fence_targets = [(0.5 + 4.0 * (i + 0.5) / 24.0, 0.2 + 3.6 * ((7 * i) % 24 + 0.5) / 24.0, 2.0) for i in range(24)]  # across slats and gaps
    waves, families = [], {}

    def family(name, items):
        families[name] = range(len(waves), len(waves) + len(items))
        waves.extend(items)

    family("identical", [_equal(_towards(t)) for t in wall_targets])
    a = _towards(wall_targets[1])
    split = []
    for angle in np.geomspace(1e-7, 0.7, 28):
        o, d = _equal(a)
        d[1::2] = _turned(a, angle)
        split.append((o, d))
    family("split", split)
    split_k = _split_waves()
    family("split k", [_wave(np.tile(s["origin"], (64, 1)), np.where(np.arange(64)[:, None] % 2 == 0, s["a"], s["b"])) for s in split_k])  # A on the even lanes
    octant = []
    for axis in range(3):
        o, d = _equal(_towards(wall_targets[0]))
        d[17 + axis, axis] = -d[17 + axis, axis]
        octant.append((o, d))
    family("octant", octant)
    one = []
    for lane, bad in ((0, np.nan), (41, np.inf), (63, -np.inf)):
        o, d = _equal(_towards(wall_targets[2]))
        o[:, 1] = bad
        o[lane] = EYE
        one.append((o, d))
    family("one lane", one)
    o, d = _equal(_towards(wall_targets[0]))
    o[3, 0], o[20, 2], d[33, 1], d[34, 0], d[63, 2] = np.nan, np.inf, np.nan, -np.inf, np.inf
    family("non-finite", [(o, d)])
    family("ignore", [_equal(_towards(wall_targets[1]))])
    family("pixel", [_pixel(_towards(t), rng) for t in wall_targets for _ in range(2)])
    family("cut-out", [_equal(_towards(t)) for t in fence_targets] + [_pixel(_towards(t), rng, 2e-2) for t in fence_targets[::3]])
    return np.concatenate([w[0] for w in waves]), np.concatenate([w[1] for w in waves]), families


def _trace(flavour, mode, o, d, ignore=None):
    """hits [n, 3] and the counters of one launch, from a fresh context (the staged tree top is sized at upload: LUM_LDS_NODES is read there)"""
    core = Core(0)
    try:
        core.set_flavour(flavour)
        core.upload(_view())
        assert core.get_single_level() == 1, "one instance under the identity"
        core.set_coherent_first_hits(mode)
        core.reset_counters()
        hits = core.trace_closest_host(o, d, ignore)
        return hits, core.counters()
    finally:
        core.close()


def _same_hits_and_counters(plain, coherent, what):
    assert plain[0].dtype == np.uint32 and np.array_equal(plain[0], coherent[0]), "%s: %d rays differ" % (what, int((plain[0] != coherent[0]).any(axis=1).sum()))
    for k in (CNT_TRACE, CNT_NODES, CNT_TRIS, CNT_NODES_LDS):
        assert plain[1][k] == coherent[1][k], "%s: counter %d: %d plain, %d coherent" % (what, k, plain[1][k], coherent[1][k])


@pytest.mark.gpu
@pytest.mark.parametrize("staged", [True, False], ids=["staged top", "no staged top"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_built_waves_hit_the_same_in_both_forms(flavour, staged, monkeypatch):
    if not staged:
        monkeypatch.setenv("LUM_LDS_NODES", "0")
    o, d, families = _waves()
    n = len(o)
    plain = _trace(flavour, 0, o, d)
    # the ignore family: lane 5 ignores the triangle the wave's other rays hit
    w = families["ignore"][0]
    assert plain[0][64 * w, 0] != SKY
    ignore = np.full((n, 2), 0xFFFFFFFF, np.uint32)
    ignore[64 * w + 5] = plain[0][64 * w, :2]
    plain, coherent = _trace(flavour, 0, o, d, ignore), _trace(flavour, 1, o, d, ignore)
    _same_hits_and_counters(plain, coherent, "%s, %s" % (flavour, "staged" if staged else "unstaged"))
    hits, cnt = plain
    assert cnt[CNT_TRACE] == n and cnt[CNT_NODES] > 4 * n
    assert (cnt[CNT_NODES_LDS] > 0) == staged and cnt[CNT_NODES_LDS] < cnt[CNT_NODES], "visits inside and outside the staged top"
    hit = hits[:, 0] != SKY

    def lanes(name):
        return np.concatenate([np.arange(64 * k, 64 * k + 64) for k in families[name]])
    assert hit[lanes("identical")].any() and not hit[lanes("identical")].all(), "walls and sky"
    sp = hits[lanes("split")].reshape(-1, 64, 3)
    assert (sp[0, 0, :2] == sp[0, 1, :2]).all() and (sp[-1, 0, :2] != sp[-1, 1, :2]).any(),"the halves end together at the small angles and apart at the large ones"
    for s, wave in zip(_split_waves(), families["split k"]):  # the device ends where the host walks end: the walks are the device's
        for lane, walked in ((0, s["hit_a"]), (1, s["hit_b"])):
            got = hits[64 * wave + lane]
            assert (got[0] == SKY) if walked is None else (got[0] != SKY and got[1] == walked[0] and abs(float(got[2:3].view(np.float32)[0]) - walked[1]) < 1e-3 * walked[1]), (s["k"], lane, got, walked)
    assert not hit[64 * families["one lane"][0] + 1] and hit[64 * families["one lane"][0]], "non-finite rays hit nothing"
    assert (hits[64 * w + 5, :2] != hits[64 * w, :2]).any() and (hits[64 * w + 6] == hits[64 * w]).all(), "the ignored triangle is not hit"
    cut = hits[lanes("cut-out")]
    fence_tris = (cut[:, 0] != SKY) & (cut[:, 1] >= _scene()[1])
    print("%s: %d rays, %.2f node visits and %.2f triangle tests per ray, %.2f of the visits from LDS; cut-out rays: %d end on the fence, %d behind it"
          % (flavour, n, cnt[CNT_NODES] / n, cnt[CNT_TRIS] / n, cnt[CNT_NODES_LDS] / cnt[CNT_NODES], int(fence_tris.sum()), int((~fence_tris).sum())))
    assert fence_tris.any() and (~fence_tris).any(), "slats stop rays, gaps let them through to the wall"


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_a_launch_of_fewer_than_64_rays(flavour):
    rng = np.random.RandomState(9)
    o, d = _pixel(_towards((0.1, 4.0, -5.0)), rng)
    _same_hits_and_counters(_trace(flavour, 0, o[:37], d[:37]), _trace(flavour, 1, o[:37], d[:37]), flavour)


@pytest.mark.gpu
def test_groups_of_dead_rays_do_not_end_a_wave_that_has_more_to_take():
    """A wave of the coherent form refills only when nothing is live, so a refill whose 64 rays all end where they are loaded (non-finite) leaves it with nothing
    live again - and it must go on to the rest of the chunk it reserved. 2^20 rays make the chunk 128 (n / (2 x waves) on a GPU of 256 CUs; 64 below ~0.5 M rays):
    the first 64 rays of every 128 are non-finite, the other 64 are traced, every one of them, and hit what the same rays hit in a launch of their own."""
    rng = np.random.RandomState(13)
    n, live = 1 << 20, 1 << 19
    base_o, base_d = zip(*[_pixel(_towards(t), rng) for t in ((-3.0, 2.5, -5.0), (0.1, 4.0, -5.0), (2.2, 0.7, -5.0), (0.0, 30.0, 0.0))])
    lo, ld = np.tile(np.concatenate(base_o), (live // 256, 1)), np.tile(np.concatenate(base_d), (live // 256, 1))
    o, d = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
    o.reshape(-1, 2, 64, 3)[:, 0], d.reshape(-1, 2, 64, 3)[:, 0] = np.nan, lo.reshape(-1, 64, 3)[:, :1]
    o.reshape(-1, 2, 64, 3)[:, 1], d.reshape(-1, 2, 64, 3)[:, 1] = lo.reshape(-1, 64, 3), ld.reshape(-1, 64, 3)
    alone, mixed = _trace("fast", 0, lo, ld), _trace("fast", 1, o, d)
    assert mixed[1][CNT_TRACE] == n, "%d of %d rays were loaded" % (mixed[1][CNT_TRACE], n)
    got = mixed[0].reshape(-1, 2, 64, 3)
    assert (got[:, 0, :, 0] == SKY).all() and np.array_equal(got[:, 1].reshape(-1, 3), alone[0])
    assert mixed[1][CNT_NODES] == alone[1][CNT_NODES] and mixed[1][CNT_TRIS] == alone[1][CNT_TRIS]


def _frame(flavour, coherent, pixel_major=1):
    core = Core(0)
    try:
        core.set_flavour(flavour)
        core.set_pixel_major(pixel_major)
        core.set_coherent_first_hits(coherent)
        core.upload(_view())
        core.set_pixels(None)
        core.reset_counters()
        said = (core.get_coherent_first_hits(), core.get_overlap_light_query())
        core.render(0, 128, samples_per_pass=64)  # two passes of 64 ids: a wave of the depth-0 launch holds one pixel
        fm, sm = core.accumulators()
        return fm.copy(), sm.copy(), core.counters(), said
    finally:
        core.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_the_renderer_keeps_every_bit_and_the_overlapped_schedule(flavour):
    plain, auto, forced = _frame(flavour, 0), _frame(flavour, -1), _frame(flavour, 1, pixel_major=0)
    assert plain[3] == (0, 1) and forced[3] == (1, 1), "the register guard reads the plain single-level kernel: the light queries still run beside the next depth's pass"
    assert auto[3][1] == 1
    for other, what in ((auto, "auto"), (forced, "forced, sample-major slots")):
        assert np.array_equal(plain[0], other[0]) and np.array_equal(plain[1], other[1]), what
        for k in (CNT_TRACE, CNT_SHADOW, CNT_LIGHT_BVH, CNT_VERTICES, CNT_NODES, CNT_TRIS, CNT_NODES_LDS):
            assert plain[2][k] == other[2][k], "%s: counter %d: %d | %d" % (what, k, plain[2][k], other[2][k])
    assert float(plain[0].max()) > 0.0 and plain[2][CNT_SHADOW] > 0


@pytest.mark.gpu
def test_the_switch_takes_single_level_scenes_only():
    from test_single_level import _placed_host
    core, host = Core(0), _placed_host(second=True)
    try:
        assert core.get_coherent_first_hits() == 0  # no scene
        core.set_coherent_first_hits(1)
        core.upload(host.device_scene())
        assert core.get_coherent_first_hits() == 0, "two instances: the two-level kernels have no coherent form"
    finally:
        core.close(); host.close()
    core = Core(0)
    try:
        core.set_coherent_first_hits(1)
        core.upload(_view())
        assert core.get_coherent_first_hits() == 1
        core.set_single_level(0)
        assert core.get_coherent_first_hits() == 0, "the form is a single-level form"
        core.set_single_level(-1)
        core.set_coherent_first_hits(0)
        assert core.get_coherent_first_hits() == 0
        with pytest.raises(Exception):
            core.set_coherent_first_hits(2)
    finally:
        core.close()
