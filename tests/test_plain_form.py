"""The shading kernel's plain form (kernels.h k_shade<.., kPlain>; lumc_set_plain_form): a scene with no translucent material, a light tree whose root holds only
lights - all of them staged in LDS, none textured - no ocean and a constant-colour or HDRI sky is shaded by an instantiation that holds no refraction code, no
light-tree descent, no textured light colour and no read of a light from memory. What it leaves out never runs on such a scene, so in the exact flavour nothing
that is written may change by a bit: frames are held to the general form with np.array_equal, the ray, light-query and vertex counters are equal. The three
facts about the content are computed on the host (scene_device.hip scene_traits) by every upload and update; the launcher asks at every launch, so a material
edited to translucent switches back by itself.

The fast flavour compiles with -ffp-contract=fast, and two instantiations of the same expressions may be contracted differently (tests/test_single_level.py met
this in the ray kernels): its plain form is held to the exact flavour no further off than its general form is, by the rule below.

`python tests/test_plain_form.py` writes the fast flavour's figures to profiles/plain_form.json."""
import functools
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # (under pytest tests/conftest.py has done this)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from luminary_amd import SUBSTRATE_OPAQUE, SUBSTRATE_TRANSLUCENT, Host, scenes
from luminary_amd.core import CNT_LIGHT_BVH, CNT_SHADOW, CNT_TRACE, CNT_VERTICES, DIRTY_MATERIALS, Core

pytestmark = pytest.mark.gpu
W = H = 64
BOUNCES = 4
IDS = 8          # sample ids of the exact comparisons
FAST_IDS = 64    # ... and of the fast flavour's
GLASS = 1        # the room's red material: the one the tests turn translucent


def _quads(quads):
    return np.concatenate([scenes._quad_uv(*q)[0] for q in quads]).astype(np.float32).reshape(-1, 9)


def _room(translucent=False, textured_emitter=False, many_lights=False, ocean=False):
    """One mesh placed once - a wavy floor, a back wall, a sphere, a box and four emissive quads (eight lights), 0.5 k triangles - under a constant sky; all
    materials opaque. The keywords break one condition of the plain form each."""
    host = Host()
    scenes.apply_benchmark_settings(host, W, H, BOUNCES, sky=(0.3, 0.35, 0.45))
    grey = host.add_material(scenes._material((0.6, 0.6, 0.6), 0.6))
    red = scenes._material((0.8, 0.3, 0.2), 0.15)
    if translucent:
        red.base_substrate = SUBSTRATE_TRANSLUCENT
    red = host.add_material(red)
    assert red == GLASS
    glow = host.add_material(scenes._material((0.8, 0.8, 0.8), 0.7, emission=(14.0, 12.0, 9.0)))
    floor = scenes._grid(9, 7, -5, 5, -5, 5, lambda x, z: 0.2 * np.sin(1.3 * x) * np.cos(0.9 * z)).reshape(-1, 9)
    wall = _quads([((-5, 0, -5), (5, 0, -5), (5, 6, -5), (-5, 6, -5))])
    ball = (scenes._sphere(9)[0] * 1.1 + np.tile(np.array([1.5, 1.4, -0.5], np.float32), 3)).reshape(-1, 9)
    box = (scenes._box()[0] * 0.8 + np.tile(np.array([-1.8, 0.9, 0.6], np.float32), 3)).reshape(-1, 9)
    if many_lights:  # 300 emissive triangles: more than the root's 128 children, so the root holds nodes (and more than LDS stages)
        panels = scenes._grid(15, 10, -3, 3, -2, 2, lambda x, z: 4.5 + 0.0 * x).reshape(-1, 9)
        assert len(panels) == 300
    else:
        panels = _quads([((x - 0.7, 4.5, z - 0.7), (x - 0.7, 4.5, z + 0.7), (x + 0.7, 4.5, z + 0.7), (x + 0.7, 4.5, z - 0.7)) for x in (-2.0, 2.0) for z in (-2.0, 1.5)])
        assert len(panels) == 8
    pos = np.concatenate([floor, wall, ball, box, panels]).astype(np.float32)
    mats = np.concatenate([np.full(len(floor) + len(wall), grey), np.full(len(ball), red), np.full(len(box), grey), np.full(len(panels), glow)]).astype(np.uint16)
    assert len(pos) < 1000
    host.new_instance(host.add_mesh(pos, mats))
    if textured_emitter:  # one more emitter, with an emission texture (a second mesh: it brings texture coordinates)
        tex = np.zeros((4, 4, 4), dtype=np.uint8)
        tex[..., 3] = 255
        tex[:, 0::2, :3] = (250, 200, 40)
        tex[:, 1::2, :3] = (40, 90, 250)
        screen = scenes._material((0.8, 0.8, 0.8), 0.7, emission=(0.0, 0.0, 0.0))
        screen.luminance_tex, screen.emission_scale = host.add_texture(tex), 20.0
        p, uv = scenes._quad_uv((-1, 0.5, -4.9), (1, 0.5, -4.9), (1, 2.5, -4.9), (-1, 2.5, -4.9))
        host.new_instance(host.add_mesh(p, np.full(len(p), host.add_material(screen), dtype=np.uint16), uvs=uv))
    if ocean:
        o = host.get_ocean()
        o.active, o.height, o.amplitude, o.frequency = True, 0.6, 0.2, 0.5
        host.set_ocean(o)
    scenes.set_camera(host, (0.5, 3.0, 11.0), (-0.15, 0.0, 0.0), fov=0.9)
    return host


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(host, view) of the two plain scenes, made once"""
    host = scenes.cornell_host("/tmp/lum_plain_form_cornell", W, H, BOUNCES) if name == "cornell" else _room()
    return host, host.device_scene()


def _frame(view, flavour, mode, first=0, ids=IDS):
    """first moment, second moment, counters and what lumc_get_plain_form says, from a fresh context"""
    core = Core(0)
    try:
        core.set_flavour(flavour)
        core.set_plain_form(mode)
        core.upload(view)
        core.set_pixels(None)
        core.reset_counters()
        core.render(first, ids, samples_per_pass=ids)
        fm, sm = core.accumulators()
        return fm.copy(), sm.copy(), core.counters(), core.get_plain_form()
    finally:
        core.close()


def _same_bits(a, b, what):
    assert np.array_equal(a[0], b[0]), what + ": first moment"
    assert np.array_equal(a[1], b[1]), what + ": second moment"
    assert float(a[0].max()) > 0.0, what


@pytest.mark.parametrize("name", ["cornell", "room"])
def test_the_exact_flavour_keeps_every_bit(name):
    view = _scene(name)[1]
    general, plain = _frame(view, "exact", 0), _frame(view, "exact", -1)
    assert (general[3], plain[3]) == (0, 1)
    _same_bits(general, plain, name)
    for k in (CNT_TRACE, CNT_SHADOW, CNT_LIGHT_BVH, CNT_VERTICES):
        assert general[2][k] == plain[2][k] and plain[2][k] > 0, "%s: counter %d: %d general, %d plain" % (name, k, general[2][k], plain[2][k])


def _rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b.astype(np.float64)))


@functools.lru_cache(maxsize=None)
def _fast_figures(name):
    """e_plain and e_general on sample ids [0, 64), e_general on the disjoint ids [64, 128): relative L2 distance of the fast flavour's first moment from the
    exact flavour's over the same ids."""
    view = _scene(name)[1]
    exact_a, exact_b = _frame(view, "exact", -1, 0, FAST_IDS)[0], _frame(view, "exact", -1, FAST_IDS, FAST_IDS)[0]
    plain = _frame(view, "fast", -1, 0, FAST_IDS)
    general_a, general_b = _frame(view, "fast", 0, 0, FAST_IDS), _frame(view, "fast", 0, FAST_IDS, FAST_IDS)
    assert (plain[3], general_a[3], general_b[3]) == (1, 0, 0)
    return {"e_plain": _rel_l2(plain[0], exact_a), "e_general": _rel_l2(general_a[0], exact_a), "e_general_other_ids": _rel_l2(general_b[0], exact_b)}


@pytest.mark.parametrize("name", ["cornell", "room"])
def test_the_fast_flavours_plain_form_is_no_further_from_exact_than_its_general_form(name):
    """Contraction may round the two instantiations differently. The yardstick is the general form's own distance from the exact flavour and how much that
    distance moves between two disjoint ranges of sample ids: e_plain may exceed the larger e_general by no more than the two e_general differ."""
    f = _fast_figures(name)
    print("%s: e_plain %.6g, e_general %.6g, e_general on other ids %.6g" % (name, f["e_plain"], f["e_general"], f["e_general_other_ids"]))
    assert f["e_general"] > 0.0 and f["e_general_other_ids"] > 0.0
    assert f["e_plain"] - max(f["e_general"], f["e_general_other_ids"]) <= abs(f["e_general"] - f["e_general_other_ids"]), f


@pytest.mark.parametrize("broken", ["translucent", "textured_emitter", "many_lights", "ocean"])
def test_the_form_is_refused_where_it_must_be(broken):
    host = _room(**{broken: True})
    try:
        view = host.device_scene()
        assert view.ocean_active == (1 if broken == "ocean" else 0)
        off, forced = _frame(view, "exact", 0), _frame(view, "exact", 1)
        assert (off[3], forced[3]) == (0, 0), broken
        _same_bits(off, forced, broken)
        assert off[2] == forced[2]
    finally:
        host.close()


def test_a_material_edit_switches_the_form_off_and_back_on():
    def edited(substrate, host=None):
        host = host or _room()
        m = host.get_material(GLASS)
        m.base_substrate = substrate
        host.set_material(GLASS, m)
        return host

    def render(core):
        core.clear()
        core.render(0, IDS, samples_per_pass=IDS)
        fm, sm = core.accumulators()
        return fm.copy(), sm.copy()

    host, core = _room(), Core(0)
    fresh = []
    try:
        core.set_flavour("exact")
        core.upload(host.device_scene())
        core.set_pixels(None)
        assert core.get_plain_form() == 1
        opaque = render(core)
        for substrate, want_form in ((SUBSTRATE_TRANSLUCENT, 0), (SUBSTRATE_OPAQUE, 1)):
            edited(substrate, host)
            core.update(host.device_scene(), DIRTY_MATERIALS)
            assert core.get_plain_form() == want_form
            got = render(core)
            fresh.append(edited(substrate))
            want = _frame(fresh[-1].device_scene(), "exact", -1)
            assert want[3] == want_form
            _same_bits(got, want, "after the edit to substrate %d" % substrate)
            assert np.array_equal(got[0], opaque[0]) == (substrate == SUBSTRATE_OPAQUE), "glass must change the image, and going back must restore it"
    finally:
        core.close()
        host.close()
        for h in fresh:
            h.close()


if __name__ == "__main__":
    out = {"what": "relative L2 distance of the fast flavour's first moment from the exact flavour's, %d x %d, %d bounces, %d sample ids: plain form and general "
                   "form on ids [0, %d), general form on ids [%d, %d) (tests/test_plain_form.py)" % (W, H, BOUNCES, FAST_IDS, FAST_IDS, FAST_IDS, 2 * FAST_IDS),
           "rule": "e_plain - max(e_general, e_general_other_ids) <= |e_general - e_general_other_ids|"}
    for scene in ("cornell", "room"):
        out[scene] = _fast_figures(scene)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "plain_form.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
