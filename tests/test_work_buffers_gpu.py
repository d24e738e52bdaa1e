"""The work arena laid out again in a living context (csrc/host/core.hip ensure_work, csrc/host/work_layout.h).

One Core renders a plain scene with one sample id per pass, then with four (the capacity grows), then the same scene in fog (19 visibility-ray kinds instead
of 4 at an unchanged capacity), then a procedural sky with clouds (the cloud arrays appear), then the plain scene with one sample id again (the larger block is
kept). After every step its moments equal, bit for bit, those of a fresh Core that only ever saw that step: an array the new layout forgot, misplaced or sized
for the old capacity would be written past or shared with its neighbour. Exact flavour, 48 x 32 pixels, 3 bounces, no particles."""
import numpy as np
import pytest

from luminary_amd import SKY_MODE_CONSTANT_COLOR, scenes
from test_clouds import _cloud_view, _sky_scene, _with_clouds
from test_fog import _fogged, _view

W, H, BOUNCES = 48, 32, 3


def _step(core, view, samples):
    core.upload(view)
    core.set_pixels(None)
    core.render(0, samples, samples_per_pass=samples)
    return core.accumulators()


@pytest.mark.gpu
def test_the_work_arena_is_laid_out_again_for_more_paths_more_kinds_and_clouds():
    from luminary_amd.core import Core
    views = {"plain": _view(scenes.zoo_scene(W, H, BOUNCES, sky_mode=SKY_MODE_CONSTANT_COLOR)),
             "fog": _view(_fogged(scenes.zoo_scene(W, H, BOUNCES, sky_mode=SKY_MODE_CONSTANT_COLOR))),  # the zoo's emissive triangles: bridges
             "clouds": _cloud_view(_with_clouds(_sky_scene(W, H, BOUNCES)))}
    steps = [("plain", 1), ("plain", 4), ("fog", 4), ("clouds", 4), ("plain", 1)]
    fresh = {}
    for step in sorted(set(steps)):
        core = Core(0)
        try:
            core.set_flavour("exact")
            fresh[step] = _step(core, views[step[0]], step[1])
        finally:
            core.close()
    assert not np.array_equal(fresh[("plain", 4)][0], fresh[("fog", 4)][0]) and np.isfinite(fresh[("clouds", 4)][0]).all()
    core = Core(0)
    try:
        core.set_flavour("exact")
        for i, step in enumerate(steps):
            fm, sm = _step(core, views[step[0]], step[1])
            assert np.array_equal(fm, fresh[step][0]), "step %d %s: first moment, %d of %d differ" % (i + 1, step, (fm != fresh[step][0]).sum(), fm.size)
            assert np.array_equal(sm, fresh[step][1]), "step %d %s: second moment" % (i + 1, step)
    finally:
        core.close()
