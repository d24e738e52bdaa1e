"""The overlapped schedule (csrc/host/core.hip wavefront_depths, overlap_allowed; lumc_set_overlap_light_query): a depth's light queries run on the context's side
stream beside the next depth's closest-hit pass. Nothing a frame is made of depends on the order: a visibility word depends only on its own ray, the NEE records
are complete before anything reads them, the resolve's sums keep their order. So every case renders with the switch on and off and asks for EQUAL first and second
moments and equal counters, all of them, in both flavours; where the schedule must refuse (two-level ray kernels: the registers; fog; ray sorting) the getter
says 0 as well. The register guard's arithmetic is a plain function and is checked without a device."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib
from luminary_amd import scenes
from luminary_amd.core import CNT_LIGHT_BVH, CNT_SHADOW, CNT_TRACE, Core
from test_plain_form import _room
from test_single_level import _placed_host

FLAVOURS = ["fast", "exact"]
IDS, PER_PASS = 8, 4  # 8 sample ids in passes of 4: the second pass meets the events of the first


def _with_depth(host, max_depth):
    s = host.get_settings()
    s.max_ray_depth = max_depth
    host.set_settings(s)
    return host


def _fogged(host):
    f = host.get_fog()
    f.active, f.density, f.height, f.dist, f.droplet_diameter = True, 40.0, 500.0, 500.0, 10.0
    host.set_fog(f)
    return host


@functools.lru_cache(maxsize=None)
def _view(name):
    if name == "cornell":  # 36 triangles, one instance: the single-level ray kernels; fast: the fused resolve, exact: the plain one
        return scenes.cornell_host("/tmp/lum_overlap_cornell", 64, 48, 8).device_scene()
    if name == "room":  # one mesh placed once, 0.5 k triangles, 64 x 64, 4 bounces
        return _room().device_scene()
    if name == "room_depth0":  # the only depth is the last: nothing to overlap
        return _with_depth(_room(), 0).device_scene()
    if name == "room_depth1":  # depth 0 overlaps, depth 1 is the last
        return _with_depth(_room(), 1).device_scene()
    if name == "room_fog":
        return oracle_lib.with_luts(_fogged(_room()).device_scene())
    assert name == "two_instances"  # the two-level ray kernels: no room in the registers
    return _placed_host(second=True).device_scene()


def _render(name, flavour, mode, sorting=0, own_stream=False):
    """first moment, second moment, all counters and what lumc_get_overlap_light_query said before the render, from a fresh context"""
    core = Core(0)
    try:
        core.set_flavour(flavour)
        core.set_overlap_light_query(mode)
        if sorting:
            core.set_ray_sorting(sorting)
        core.upload(_view(name))
        core.set_pixels(None)
        core.reset_counters()
        said = core.get_overlap_light_query()
        if not own_stream:
            core.render(0, IDS, samples_per_pass=PER_PASS)
        else:  # two calls back to back on a stream of the caller's, nothing in between
            hip = C.CDLL("libamdhip64.so.7")  # the runtime the library is linked to, already loaded with it
            stream = C.c_void_p()
            assert hip.hipStreamCreateWithFlags(C.byref(stream), C.c_uint(1)) == 0 and stream.value  # hipStreamNonBlocking
            try:
                core.render(0, PER_PASS, samples_per_pass=PER_PASS, stream=stream.value)
                core.render(PER_PASS, IDS - PER_PASS, samples_per_pass=PER_PASS, stream=stream.value)
                core.synchronize()
            finally:
                assert hip.hipStreamDestroy(stream) == 0
        fm, sm = core.accumulators()
        return fm.copy(), sm.copy(), core.counters(), said
    finally:
        core.close()


@functools.lru_cache(maxsize=None)
def _serial(name, flavour, sorting=0):
    return _render(name, flavour, 0, sorting)


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), what + ": first moment"
    assert np.array_equal(a[1], b[1]), what + ": second moment"
    assert a[2] == b[2], what + ": counters %s | %s" % (a[2], b[2])
    assert float(a[0].max()) > 0.0 and a[2][CNT_TRACE] > 0 and a[2][CNT_SHADOW] > 0, what


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("name", ["cornell", "room"])
def test_the_overlapped_schedule_keeps_every_bit_and_every_counter(name, flavour):
    serial, overlapped = _serial(name, flavour), _render(name, flavour, 1)
    assert (serial[3], overlapped[3]) == (0, 1), "one instance under the identity: the single-level ray kernels leave room for the light queries"
    assert serial[2][CNT_LIGHT_BVH] > 0, "no light query to overlap"
    _same(serial, overlapped, "%s, %s" % (name, flavour))


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("name, said", [("room_depth0", 0), ("room_depth1", 1)])
def test_every_depth_but_the_last(name, said, flavour):
    """Depth limit 0: the only depth is the last, the pass has nothing to overlap and says so. Depth limit 1: depth 0's light queries beside depth 1's closest hits,
    depth 1's on the caller's stream."""
    serial, overlapped = _serial(name, flavour), _render(name, flavour, 1)
    assert (serial[3], overlapped[3]) == (0, said)
    _same(serial, overlapped, "%s, %s" % (name, flavour))


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_the_two_level_ray_kernels_keep_the_serial_order(flavour):
    serial, asked = _serial("two_instances", flavour), _render("two_instances", flavour, 1)
    assert (serial[3], asked[3]) == (0, 0), "4 x 120 + 112 registers do not fit a SIMD"
    _same(serial, asked, "two instances, " + flavour)


@pytest.mark.gpu
def test_fog_and_ray_sorting_keep_the_serial_order():
    serial, asked = _serial("room_fog", "fast"), _render("room_fog", "fast", 1)
    assert (serial[3], asked[3]) == (0, 0), "fog puts its passes between the closest hits and the shading"
    _same(serial, asked, "fog")
    serial, asked = _serial("room", "fast", 1), _render("room", "fast", 1, sorting=1)
    assert (serial[3], asked[3]) == (0, 0), "the sort's keys and the trace through them are ordered on one stream"
    _same(serial, asked, "ray sorting")


@pytest.mark.gpu
def test_two_renders_back_to_back_on_a_callers_stream():
    """The side stream is joined into the stream the caller gave, not into another: the second call's passes and the accumulate kernels find the first call's work
    done. The stream is a non-blocking one made in the HIP runtime the library is linked to (torch brings a HIP runtime of its own, whose streams that one does not know)."""
    overlapped = _render("room", "fast", 1, own_stream=True)
    assert overlapped[3] == 1
    _same(_serial("room", "fast"), overlapped, "two calls on a non-default stream")


def test_the_register_guard_is_plain_arithmetic():
    """(closest-hit kernel, visibility kernel, k_light_query) registers per lane. The visibility kernel never runs beside the light queries - it waits for them -,
    so the guard asks for the other two: both rounded up to the allocation unit of 8, four ray-kernel waves and one of the light queries within a SIMD's 512."""
    for trace, shadow, light_query, fits in [(96, 96, 111, True), (114, 111, 111, False), (128, 128, 64, False)]:
        assert Core.overlap_registers_fit(trace, light_query) is fits, (trace, shadow, light_query)
    assert Core.overlap_registers_fit(100, 112) is False, "100 is allocated as 104: 4 x 104 + 112 = 528"
    assert Core.overlap_registers_fit(96, 128) is True and Core.overlap_registers_fit(96, 129) is False
    assert Core.overlap_registers_fit(0, 0) is False, "counts that could not be read"
