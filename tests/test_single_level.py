"""The ray kernels' single-level form (dev_trace.h trace_items<Q, true>; lumc_set_single_level): on a scene of ONE hittable instance closest-hit and visibility
rays are mapped to the instance's object space where they are loaded and start at the mesh tree's root - no visit of the top-level node, no instance-entry phase,
no marker on the stack. What is tested per lane stays what it was, in the same order, so nothing that is written may change by a bit: frames and hits are held
to the two-level form with np.array_equal in both flavours, the ray and triangle counters are equal, and the node counters drop by at most one visit per ray
(exactly one for every ray that reaches the instance's box). The launchers choose per launch from the scene on the device: a scene update that adds an instance
switches back by itself. The particle pass has no single-level kernel (k_trace_particles walks the particle lattice's own two levels).

The fast flavour takes the single-level form only where the instance's transform is the identity (csrc/host/context.h single_level_allowed). Measured with the form
forced onto the placed instance below: 1047 of 10260 probe rays and the frame differed from the two-level form in the last bits, the exact flavour's not at all. The
cause is -ffp-contract=fast: the compiler decides per place which product of `(a * x + b * y) + c * z` goes into which fma - in the two-level k_trace rows 0 and 1 of
the direction round a * x first, row 2 rounds b * y first - so a second instantiation of the same expressions rounds another way. With rows of 1 and 0 and no
translation nothing is rounded in any arrangement. So for the placed instance the fast flavour is held to `get_single_level() == 0`, not 1, and its frames to
equality all the same; the hall (an identity transform) runs the form in both flavours."""
import functools

import numpy as np
import pytest

from luminary_amd import Host, scenes
from luminary_amd.core import (CNT_LIGHT_BVH, CNT_NODES, CNT_NODES_SHADOW, CNT_SHADOW, CNT_TRACE, CNT_TRIS, CNT_TRIS_SHADOW, DIRTY_INSTANCES, DIRTY_LIGHTS, Core)

pytestmark = pytest.mark.gpu
FLAVOURS = ["fast", "exact"]
PLACED = ((0.7, -0.4, 1.3), (0.35, -0.6, 0.2), (1.3, 0.8, 1.1))  # position, rotation, scale of the one instance: the object-space ray differs from the world ray


@functools.lru_cache(maxsize=None)
def _hall():
    return scenes.hall_scene(160, 90, 4, target_triangles=20_000)


def _eligible(flavour, identity):
    return 1 if (flavour == "exact" or identity) else 0


def _placed_host(second=False, particles=False, identity=False):
    """One mesh - a wavy floor, a sphere, a box and an emissive panel, 2.6 k triangles - placed once, rotated, scaled unevenly and moved; constant sky."""
    host = Host()
    scenes.apply_benchmark_settings(host, 96, 64, 4, sky=(0.5, 0.6, 0.8))
    grey = host.add_material(scenes._material((0.6, 0.6, 0.6), 0.6))
    red = host.add_material(scenes._material((0.8, 0.3, 0.2), 0.3))
    glow = host.add_material(scenes._material((0.8, 0.8, 0.8), 0.7, emission=(12.0, 11.0, 9.0)))
    floor = scenes._grid(24, 24, -5, 5, -5, 5, lambda x, z: 0.25 * np.sin(1.3 * x) * np.cos(0.9 * z))
    ball = scenes._sphere(16)[0] * 1.1 + np.tile(np.array([1.5, 1.4, -0.5], np.float32), 3)
    box = scenes._box()[0] * 0.8 + np.tile(np.array([-1.8, 0.9, 0.6], np.float32), 3)
    panel = np.array([[-1.5, 4.0, -1.5, 1.5, 4.0, 1.5, 1.5, 4.0, -1.5], [-1.5, 4.0, -1.5, -1.5, 4.0, 1.5, 1.5, 4.0, 1.5]], np.float32)
    pos = np.concatenate([floor, ball, box, panel]).astype(np.float32)
    mats = np.concatenate([np.full(len(floor), grey), np.full(len(ball), red), np.full(len(box), grey), np.full(len(panel), glow)]).astype(np.uint16)
    assert 2000 < len(pos) < 5000
    mesh = host.add_mesh(pos, mats)
    if identity:
        host.new_instance(mesh)
    else:
        host.new_instance(mesh, *PLACED)
    if second:
        _add_second(host)
    if particles:
        p = host.get_particles()
        p.active, p.count, p.size, p.scale, p.speed, p.seed, p.phase_diameter = True, 1500, 20.0, 4.0, 0.0, 3, 50.0
        host.set_particles(p)
    scenes.set_camera(host, (0.5, 3.0, 11.0), (-0.15, 0.0, 0.0), fov=0.9)
    return host


def _add_second(host):
    host.new_instance(0, (-2.5, 2.2, -3.0), (0.1, 0.9, -0.3), (0.4, 0.5, 0.45))


def _frame(view, flavour, mode, core=None):
    """first moment, second moment, counters and what lumc_get_single_level says, from a fresh context (or `core` as it stands)"""
    own = core is None
    if own:
        core = Core(0)
    try:
        if own:
            core.set_flavour(flavour)
            core.set_single_level(mode)
            core.upload(view)
        core.set_pixels(None)
        core.reset_counters()
        core.render(0, 4, samples_per_pass=4)
        fm, sm = core.accumulators()
        return fm, sm, core.counters(), core.get_single_level()
    finally:
        if own:
            core.close()


def _same_frames(a, b, what):
    assert np.array_equal(a[0], b[0]), what + ": first moment"
    assert np.array_equal(a[1], b[1]), what + ": second moment"
    assert float(a[0].max()) > 0.0, what


def _same_work_one_visit_less(two, one, what):
    for k in (CNT_TRACE, CNT_SHADOW, CNT_LIGHT_BVH, CNT_TRIS, CNT_TRIS_SHADOW):
        assert two[k] == one[k], "%s: counter %d: %d two-level, %d single-level" % (what, k, two[k], one[k])
    for rays, nodes in ((CNT_TRACE, CNT_NODES), (CNT_SHADOW, CNT_NODES_SHADOW)):
        saved = two[nodes] - one[nodes]
        print("%s: %d rays, node visits per ray %.3f two-level, %.3f single-level" % (what, two[rays], two[nodes] / max(two[rays], 1), one[nodes] / max(one[rays], 1)))
        assert two[rays] > 2_000
        assert 0 <= saved <= two[rays] and one[nodes] < two[nodes], "%s: counter %d: %d two-level, %d single-level, %d rays" % (what, nodes, two[nodes], one[nodes], two[rays])


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_the_hall_renders_the_same_frame_with_one_node_visit_less_per_ray(flavour):
    view = _hall().device_scene()
    two, one = _frame(view, flavour, 0), _frame(view, flavour, -1)
    assert (two[3], one[3]) == (0, 1)
    _same_frames(two, one, "hall, " + flavour)
    _same_work_one_visit_less(two[2], one[2], "hall, " + flavour)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_a_rotated_unevenly_scaled_and_moved_instance_renders_the_same_frame(flavour):
    host = _placed_host()
    try:
        view = host.device_scene()
        two, one = _frame(view, flavour, 0), _frame(view, flavour, -1)
        assert (two[3], one[3]) == (0, _eligible(flavour, False))
        _same_frames(two, one, "placed instance, " + flavour)
        if one[3]:
            _same_work_one_visit_less(two[2], one[2], "placed instance, " + flavour)
        else:
            assert two[2] == one[2]
    finally:
        host.close()


def test_the_switch_takes_what_it_is_documented_to_take():
    host, core = _placed_host(), Core(0)
    try:
        assert core.get_single_level() == 0  # no scene
        core.set_flavour("exact")
        core.upload(host.device_scene())
        assert core.get_single_level() == 1
        core.set_flavour("fast")
        assert core.get_single_level() == 0, "the fast flavour takes identity transforms only"
        core.set_flavour("exact")
        core.set_single_level(0)
        assert core.get_single_level() == 0
        core.set_single_level(1)
        assert core.get_single_level() == 1
        for bad in (-2, 2):
            with pytest.raises(Exception):
                core.set_single_level(bad)
        assert core.get_single_level() == 1
    finally:
        core.close(); host.close()


def test_scenes_of_many_instances_walk_both_levels():
    for host in (scenes.zoo_scene(48, 32, 3), scenes.example_scene(width=48, height=32, sphere_segments=6, ground_res=8)):
        core = Core(0)
        try:
            core.set_single_level(1)
            core.upload(host.device_scene())
            assert host.get_num_instances() > 2 and core.get_single_level() == 0
        finally:
            core.close(); host.close()


def test_particles_keep_their_two_level_pass_next_to_single_level_surfaces():
    """The particle pass is k_trace_particles over the particle lattice's own top level in either mode; the surfaces of the scene are one instance."""
    host = _placed_host(particles=True)
    try:
        view = host.device_scene()
        assert view.particles_active == 1
        two, one = _frame(view, "exact", 0), _frame(view, "exact", -1)
        assert (two[3], one[3]) == (0, 1)
        _same_frames(two, one, "placed instance with particles")
    finally:
        host.close()


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_a_second_instance_added_by_a_scene_update_switches_back(flavour):
    host, core = _placed_host(), Core(0)
    try:
        core.set_flavour(flavour)
        core.upload(host.device_scene())
        assert core.get_single_level() == _eligible(flavour, False)
        before = _frame(None, flavour, -1, core=core)
        _add_second(host)
        core.update(host.device_scene(), DIRTY_INSTANCES | DIRTY_LIGHTS)
        assert core.get_single_level() == 0
        core.clear()
        updated = _frame(None, flavour, -1, core=core)
        fresh_host = _placed_host(second=True)
        try:
            fresh = _frame(fresh_host.device_scene(), flavour, -1)
        finally:
            fresh_host.close()
        assert fresh[3] == 0
        _same_frames(updated, fresh, "two instances after an update, " + flavour)
        assert updated[2][:3] == fresh[2][:3]
        assert not np.array_equal(before[0], updated[0]), "the second instance is in view"
    finally:
        core.close(); host.close()


def _hostile_rays():
    rng = np.random.RandomState(41)

    def unit(v):
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    centre = np.array(PLACED[0], np.float32) + np.array([0.0, 1.5, 0.0], np.float32)
    o_far = rng.uniform(-40.0, 40.0, (3000, 3)).astype(np.float32)                 # most of these miss the instance's box
    d_far = unit(rng.normal(size=(3000, 3)))
    o_aim = rng.uniform(-25.0, 25.0, (3000, 3)).astype(np.float32)                 # aimed at it from outside
    d_aim = unit(centre + rng.uniform(-4.0, 4.0, (3000, 3)) - o_aim)
    o_in = (centre + rng.uniform(-3.0, 3.0, (3000, 3))).astype(np.float32)         # starting inside it
    d_in = unit(rng.normal(size=(3000, 3)))
    o_ax = (centre + rng.uniform(-8.0, 8.0, (1200, 3))).astype(np.float32)         # axis-parallel, zero components of either sign
    d_ax = np.zeros((1200, 3), np.float32)
    axis = rng.randint(0, 3, 1200)
    d_ax[np.arange(1200), axis] = rng.choice([-1.0, 1.0], 1200)
    d_ax = np.where(d_ax == 0.0, np.copysign(np.float32(0.0), rng.choice([-1.0, 1.0], (1200, 3))), d_ax).astype(np.float32)
    o_bad = (centre + rng.uniform(-5.0, 5.0, (60, 3))).astype(np.float32)          # non-finite origins and directions
    d_bad = unit(rng.normal(size=(60, 3)))
    for k, value in enumerate((np.nan, np.inf, -np.inf)):
        for c in range(3):
            o_bad[6 * k + c, c] = value
            d_bad[6 * k + 3 + c, c] = value
    o, d = np.concatenate([o_far, o_aim, o_in, o_ax, o_bad]), np.concatenate([d_far, d_aim, d_in, d_ax, d_bad])
    assert np.signbit(d_ax[d_ax == 0.0]).any() and not np.signbit(d_ax[d_ax == 0.0]).all()
    return o, d


@pytest.mark.parametrize("identity", [False, True], ids=["placed", "identity"])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_hostile_rays_through_the_probes_hit_the_same_in_both_forms(flavour, identity):
    host, core = _placed_host(identity=identity), Core(0)
    try:
        core.set_flavour(flavour)
        core.upload(host.device_scene())
        o, d = _hostile_rays()
        n = len(o)
        hits, cnts = {}, {}
        for mode in (0, -1):
            core.set_single_level(mode)
            assert core.get_single_level() == (0 if mode == 0 else _eligible(flavour, identity))
            core.reset_counters()
            hits[mode] = core.trace_closest_host(o, d)
            cnts[mode] = core.counters()
        assert hits[0].dtype == np.uint32 and np.array_equal(hits[0], hits[-1]), "%d of %d rays differ" % (int((hits[0] != hits[-1]).any(axis=1).sum()), n)
        hit = hits[0][:, 0] != 0xFFFFFFFE
        print("%s: %d rays, %d hit; node visits %d two-level, %d single-level" % (flavour, n, int(hit.sum()), cnts[0][CNT_NODES], cnts[-1][CNT_NODES]))
        print("hit shares: far %.3f, aimed %.3f, from inside %.3f, axis-parallel %.3f" % (hit[:3000].mean(), hit[3000:6000].mean(), hit[6000:9000].mean(), hit[9000:10200].mean()))
        assert hit[:3000].mean() < 0.5 and hit[3000:6000].mean() > 0.2 and hit[6000:9000].mean() > 0.2 and hit[9000:10200].any() and not hit[-60:-42].any()
        assert cnts[0][CNT_TRACE] == cnts[-1][CNT_TRACE] == n and cnts[0][CNT_TRIS] == cnts[-1][CNT_TRIS]
        assert 0 <= cnts[0][CNT_NODES] - cnts[-1][CNT_NODES] <= n and (cnts[-1][CNT_NODES] < cnts[0][CNT_NODES]) == bool(_eligible(flavour, identity))
        # the same rays as visibility rays, open-ended and as segments that end short of or beyond the closest hit
        t = hits[0][:, 2].copy().view(np.float32)
        dist = np.where(hit, t * np.where(np.arange(n) % 2 == 0, np.float32(0.5), np.float32(1.5)), np.float32(3.0e38)).astype(np.float32)
        ids = np.full((n, 4), 0xFFFFFFFF, np.uint32)
        vis = {}
        for mode in (0, -1):
            core.set_single_level(mode)
            vis[mode] = core.trace_visibility_host(o, d, dist, ids)
        assert np.array_equal(vis[0].view(np.uint32), vis[-1].view(np.uint32))
        assert (vis[0] == 0.0).all(axis=1).any() and (vis[0] == 1.0).all(axis=1).any(), "blocked and open rays are both among them"
    finally:
        core.close(); host.close()
