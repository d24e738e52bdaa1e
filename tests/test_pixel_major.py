"""The order of a pass's path slots (csrc/device/kernels.h pass_slot_split, kernels_shared.h accumulate_pixel_major; lumc_set_pixel_major): pixel-major slots put the sample ids
of one pixel side by side, sample-major slots one sample id of neighbouring pixels. A path's arithmetic does not depend on its slot, every result slot has one
writer and a pixel's samples are added in sample order either way. So every case renders with the switch on and off and asks for EQUAL first and second moments
and equal counters, in both flavours, and the exact flavour's frame is the oracle's as well.

The sizes are the ones at which the mapping or the accumulate kernel's tiles can go wrong: 50 x 31 = 1550 pixels (no multiple of 64: the last wave of the
accumulate kernel is part empty, the last workgroup too); batches of 1, 3, 64 and 65 (a wave of paths straddles pixels, a pixel straddles waves, the accumulate
kernel's tile of eight samples is part empty at 1, 3 and 65); a strided pixel list; a pass split over two calls; a second pass into the same accumulators; the
physical camera, whose invalid rays are not appended."""
import functools

import numpy as np
import pytest

import oracle_lib
from luminary_amd import scenes
from luminary_amd.core import CNT_LIGHT_BVH, CNT_SHADOW, CNT_TRACE, CNT_VERTICES, Core
from test_physical_camera import _host as _physical_host, _physical_camera
from test_single_level import _placed_host

FLAVOURS = ["fast", "exact"]
W, H = 50, 31
ORACLE_IDS = 3
COUNTERS = (CNT_TRACE, CNT_SHADOW, CNT_LIGHT_BVH, CNT_VERTICES)


def _resized(host, bounces):
    s = host.get_settings()
    s.width, s.height, s.max_ray_depth = W, H, bounces
    host.set_settings(s)
    return host


@functools.lru_cache(maxsize=None)
def _view(name):
    if name == "zoo":  # a dozen instances, translucent and cut materials, a light tree with inner nodes: the two-level ray kernels, the general shading kernel
        return oracle_lib.with_luts(scenes.zoo_scene(W, H, bounces=4).device_scene())  # (with_luts: the tables the oracle reads)
    if name == "single":  # one mesh placed once under the identity: the single-level ray kernels, the overlapped schedule
        return oracle_lib.with_luts(_resized(_placed_host(identity=True), 4).device_scene())
    if name == "two":  # the same mesh placed twice
        return oracle_lib.with_luts(_resized(_placed_host(second=True), 4).device_scene())
    assert name == "physical"  # a wall behind the default lens: rays that do not leave the lens get no path
    host = _physical_host(W, H, depth=2, plane_z=-10.0)
    return oracle_lib.with_luts(host.device_scene()), _physical_camera(None, False, host.get_camera())


def _render(name, flavour, mode, batch, calls, pixels=None):
    """first moment, second moment and the counters after `calls` = [(first sample id, ids), ...], each in passes of `batch`, from a fresh context"""
    core = Core(0)
    try:
        core.set_flavour(flavour)
        core.set_pixel_major(mode)
        assert core.get_pixel_major() == mode
        view = _view(name)
        if name == "physical":
            core.upload(view[0])
            core.set_physical_camera(view[1])
        else:
            core.upload(view)
        core.set_pixels(None if pixels is None else np.asarray(pixels, dtype=np.uint32))
        core.reset_counters()
        for first, ids in calls:
            core.render(first, ids, samples_per_pass=batch)
        fm, sm = core.accumulators()
        return fm.copy(), sm.copy(), core.counters()
    finally:
        core.close()


@functools.lru_cache(maxsize=None)
def _sample_major(name, flavour, batch, calls, pixels=None):
    return _render(name, flavour, 0, batch, calls, pixels)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return oracle_lib.render(_view(name), 0, ORACLE_IDS)


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), what + ": first moment"
    assert np.array_equal(a[1], b[1]), what + ": second moment"
    for k in COUNTERS:
        assert a[2][k] == b[2][k], "%s: counter %d: %d | %d" % (what, k, a[2][k], b[2][k])
    assert float(a[0].max()) > 0.0 and a[2][CNT_TRACE] > 0, what


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("batch", [1, 3, 64, 65])
@pytest.mark.parametrize("name", ["zoo", "single", "two"])
def test_pixel_major_slots_keep_every_bit_and_every_counter(name, batch, flavour):
    calls = ((0, ORACLE_IDS if batch <= ORACLE_IDS else batch),)  # batch 1: three passes of one id; 3, 64, 65: one pass
    off, on = _sample_major(name, flavour, batch, calls), _render(name, flavour, 1, batch, calls)
    _same(off, on, "%s, %s, batch %d" % (name, flavour, batch))
    assert on[2][CNT_SHADOW] > 0
    if flavour == "exact" and batch <= ORACLE_IDS:
        ofm, osm, _ = _oracle(name)
        assert np.array_equal(on[0], ofm) and np.array_equal(on[1], osm), "the exact flavour's frame is the oracle's"


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("batch", [3, 64])
def test_a_strided_pixel_list(batch, flavour):
    """A pixel list as the tile deal sets it: every seventh pixel from the fourth, 221 of them - the slot's pixel is an index into the list."""
    pixels = tuple(range(3, W * H, 7))
    calls = ((0, batch),)
    off, on = _sample_major("zoo", flavour, batch, calls, pixels), _render("zoo", flavour, 1, batch, calls, pixels)
    assert on[0].shape[-1] == len(pixels)
    _same(off, on, "strided list, %s, batch %d" % (flavour, batch))
    if flavour == "exact" and batch == ORACLE_IDS:
        ofm, osm, _ = oracle_lib.render(_view("zoo"), 0, ORACLE_IDS, pixels=np.asarray(pixels, dtype=np.uint32))
        assert np.array_equal(on[0], ofm) and np.array_equal(on[1], osm)


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("name", ["zoo", "single"])
def test_two_calls_are_one_call_and_a_second_pass_adds_to_the_first(name, flavour):
    """Ids [0, 10) in passes of 5 - the second pass adds into the accumulators the first left - in one call, and as two calls of one pass each."""
    one_call, two_calls = ((0, 10),), ((0, 5), (5, 5))
    off = _sample_major(name, flavour, 5, one_call)
    _same(off, _render(name, flavour, 1, 5, one_call), "%s, %s, one call" % (name, flavour))
    _same(off, _render(name, flavour, 1, 5, two_calls), "%s, %s, two calls" % (name, flavour))


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("batch", [3, 64])
def test_the_physical_camera_appends_only_valid_rays(batch, flavour):
    calls = ((0, batch),)
    off, on = _sample_major("physical", flavour, batch, calls), _render("physical", flavour, 1, batch, calls)
    assert 0 < on[2][CNT_TRACE], "some rays leave the lens"
    _same(off, on, "physical camera, %s, batch %d" % (flavour, batch))


@pytest.mark.gpu
def test_the_switch():
    core = Core(0)
    try:
        for mode in (0, 1):
            core.set_pixel_major(mode)
            assert core.get_pixel_major() == mode
        core.set_pixel_major(-1)
        assert core.get_pixel_major() in (0, 1)
        with pytest.raises(Exception):
            core.set_pixel_major(2)
    finally:
        core.close()
