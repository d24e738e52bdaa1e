"""One context through every resize of its device buffers, against contexts that have only ever seen one configuration.

The host layer owns device memory through DeviceBuffer members (luminary_amd/csrc/host/device_buffer.h) and reads a buffer's size from the buffer; the queues,
the scene's table pointers and the sort's planes are views into them. What that can get wrong is history: a size that is stale after a smaller frame, a view
that still points into a freed block, planes that changed owners (ray-sorting mode 3). So one context is driven 16x8 -> 40x24 -> 16x8 - the second frame no
multiple of the denoiser's 32x8 tile or of the 4x4 adaptive blocks, the first still with a bloom chain of 3 - and through every mode that re-cuts or swaps a
buffer, and after each step everything it can download must equal, bit for bit, the same calls on a fresh context. Exact flavour, as conftest.py sets it."""
import numpy as np
import pytest

from luminary_amd import SKY_MODE_HDRI, scenes
from luminary_amd.core import DIRTY_CONSTANTS, Core, default_output_params

SMALL, BIG = (16, 8), (40, 24)
SPP = 2


def _host(directory, size, fog=False):
    host = scenes.cornell_host(str(directory), size[0], size[1], 3)
    sky = host.get_sky()  # a baked sky: the context keeps the panorama across uploads, and lumc_sky_hdri_build needs an atmosphere
    sky.mode, sky.hdri_dim, sky.hdri_samples = SKY_MODE_HDRI, 16, 2
    host.set_sky(sky)
    if fog:
        f = host.get_fog()
        f.active, f.density, f.height, f.dist, f.droplet_diameter = True, 40.0, 500.0, 500.0, 10.0
        host.set_fog(f)
    return host


def _render(core, first=0, count=SPP):
    core.render(first, count, samples_per_pass=count)
    fm, sm = core.accumulators()
    return {"first_moment": fm, "second_moment": sm}


def _plain(core, size):
    core.set_pixels(None)
    return _render(core)


def _frame(core, size):
    """The full-frame chain: accumulate, result image, bloom, guides and denoiser (on a host image, then in place on the context's), output."""
    w, h = size
    core.set_pixels(None)
    out = _render(core)
    out["result"] = core.generate_result(uniform_samples=SPP)
    out["bloom"] = core.post_bloom(out["result"], w, h, 0.5)
    out["albedo"], out["normal"], out["depth"] = core.render_guides(2)
    out["denoised"] = core.denoise(out["result"], uniform_samples=SPP)
    out["denoised_in_place"] = core.denoise(None, uniform_samples=SPP)
    out["argb8"], out["planes"] = core.generate_output(default_output_params(w, h, SPP), want_float=True)
    return out


def _pixel_list(core, size):
    w, h = size
    out = {}
    core.set_pixels(np.array([0, 1, w - 1, w, 5 * w + 7, w * h - 2, w * h - 1], dtype=np.uint32))
    out.update(("listed_" + k, v) for k, v in _render(core).items())
    core.set_pixels(None)
    out.update(_render(core))
    return out


def _undersampled(core, size):
    core.set_pixels(None)
    core.render_undersampled(1, 0)
    out = dict(zip(("first_moment", "second_moment"), core.accumulators()))
    out["preview"] = core.generate_result_undersampled(1, 0)
    return out


def _adaptive(core, size):
    core.set_pixels(None)
    core.adaptive_begin(4, 2, 1)
    core.adaptive_render(2)  # the uniform execution, the stage build, one execution of the built stage
    out = dict(zip(("first_moment", "second_moment"), core.accumulators()))
    out["stage_counts"], out["block_variance"] = core.adaptive_download()
    out["result"] = core.generate_result()
    core.adaptive_end()
    return out


def _sorted_then_plain(core, size):
    core.set_pixels(None)
    core.set_ray_sorting(3)  # the queue's planes trade places with the sort's
    core.render(0, 1)
    core.set_ray_sorting(0)
    return _render(core, 1, 1)


def _baked_sky(core, dim):
    cam = (0.0, 1.0, 3.0)
    out = {"panorama": core.sky_hdri_build(cam, dim, 2)}
    core.set_pixels(None)  # the scene's sky now points at this panorama
    out.update(_render(core))
    return out


def _assert_equal(step, got, want):
    assert sorted(got) == sorted(want)
    for name in sorted(got):
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.shape == b.shape and a.dtype == b.dtype, (step, name, a.shape, b.shape)
        assert np.isfinite(a.astype(np.float64)).all(), (step, name)
        assert np.array_equal(a, b), "%s: %s differs in %d of %d values" % (step, name, int((a != b).sum()), a.size)


def _fresh(view, calls, size):
    """`calls` on a context that has seen nothing but `view`."""
    core = Core(0)
    try:
        core.upload(view)
        return calls(core, size)
    finally:
        core.close()


@pytest.mark.gpu
def test_one_context_through_every_resize_equals_fresh_contexts(tmp_path):
    hosts = {"small": _host(tmp_path / "small", SMALL), "big": _host(tmp_path / "big", BIG), "fog": _host(tmp_path / "fog", BIG, fog=True)}
    views = {k: h.device_scene() for k, h in hosts.items()}
    want_small = _fresh(views["small"], _frame, SMALL)
    want_big = _fresh(views["big"], _frame, BIG)
    assert want_small["first_moment"].any() and want_big["depth"].max() > 0.0
    core = Core(0)
    try:
        assert core.flavour == "exact"
        core.upload(views["small"])
        _assert_equal("16x8", _frame(core, SMALL), want_small)
        core.upload(views["big"])
        _assert_equal("40x24 after 16x8", _frame(core, BIG), want_big)

        _assert_equal("7 listed pixels, then the full frame", _pixel_list(core, BIG), _fresh(views["big"], _pixel_list, BIG))
        _assert_equal("undersampled, stage 1", _undersampled(core, BIG), _fresh(views["big"], _undersampled, BIG))
        want_adaptive = _fresh(views["big"], _adaptive, BIG)
        for round_ in (1, 2):
            _assert_equal("adaptive round %d" % round_, _adaptive(core, BIG), want_adaptive)
        _assert_equal("ray-sorting mode 3 on and off", _sorted_then_plain(core, BIG), _fresh(views["big"], _sorted_then_plain, BIG))

        core.update(views["fog"], DIRTY_CONSTANTS)  # the work block is cut again for 17 visibility kinds (and the sort's planes go with it)
        fogged = _plain(core, BIG)
        _assert_equal("fog on", fogged, _fresh(views["fog"], _plain, BIG))
        assert not np.array_equal(fogged["first_moment"], want_big["first_moment"]), "the fog changed nothing"
        core.update(views["big"], DIRTY_CONSTANTS)
        _assert_equal("fog off", _plain(core, BIG), {k: want_big[k] for k in ("first_moment", "second_moment")})

        want_sky = {dim: _fresh(views["big"], lambda c, size, dim=dim: _baked_sky(c, dim), BIG) for dim in (8, 16)}
        assert want_sky[8]["panorama"].shape == (8, 8, 4) and want_sky[16]["panorama"].any()
        for dim in (8, 16, 8):
            _assert_equal("sky baked at %d" % dim, _baked_sky(core, dim), want_sky[dim])

        core.upload(views["small"])
        _assert_equal("16x8 after 40x24", _frame(core, SMALL), want_small)
    finally:
        core.close()
