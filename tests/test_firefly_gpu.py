"""Firefly rejection on the device (csrc/host/firefly.hip k_bucket_accumulate, k_bucket_accumulate_scatter, k_firefly_resolve; include/lum_core.h
lumc_set_firefly_buckets / lumc_firefly_resolve; include/luminary_amd.h luminary_ext_set_firefly_rejection). Exact flavour (one case in the fast one), frame 48 x 32,
at most 24 sample ids per test.

  buckets   bucket b holds, bit for bit, the first_moment of a fresh context that rendered the ids b, b + K, ... with one lumc_render call per id - for passes of
            1, 3 and all ids, both slot orders, the full frame and a strided pixel list - and the accumulators keep the bits they have with the buckets off.
  resolve   k_firefly_resolve equals the twin (tests/test_firefly.py holds the twin to the definition) on the downloaded buckets, image and counters, also after
            chosen bucket words were overwritten with 1e6, NaN and Inf.
  host      the public switch: off changes nothing, on delivers the chain run on the twin's image.

Sizes: 48 x 32 = 1536 pixels is six workgroups of 256 and twelve of the pixel-major form's 128; the strided list range(3, 1536, 7) has 219 pixels - a part-empty
last wave and workgroup in either form. 2 K + 3 ids leave the tile of eight slots part empty (11, 13, 19 ids), give the buckets unequal counts (3 and 2) and, in
passes of 1 and 3, start passes at every phase of id mod K."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import luminary_amd
import oracle_lib
from luminary_amd import scenes
from luminary_amd.core import Core, CoreError, default_output_params, firefly_resolve_host, undersampling_schedule
from test_mesh_positions_api import bend

pytestmark = pytest.mark.gpu
F, U = np.float32, np.uint32
W, H = 48, 32
P = W * H
STRIDED = tuple(range(3, P, 7))
INVALID_API_ARGUMENT = 3


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(U)


@functools.lru_cache(maxsize=None)
def _zoo_view():
    return oracle_lib.with_luts(scenes.zoo_scene(W, H, bounces=4).device_scene())


def _core(flavour="exact", pixel_major=0, pixels=None, buckets=0):
    core = Core(0)
    core.set_flavour(flavour)
    core.set_pixel_major(pixel_major)
    core.upload(_zoo_view())
    core.set_pixels(None if pixels is None else np.asarray(pixels, dtype=U))
    if buckets:
        core.set_firefly_buckets(buckets)
    return core


@functools.lru_cache(maxsize=None)
def _bucket_reference(K, ids, pixels, flavour="exact"):
    """[K, 3, pixels]: per bucket the first_moment of a fresh context that rendered the ids b, b + K, ... below `ids` with one lumc_render call per id; counts [K]."""
    sums, counts = [], []
    for b in range(K):
        core = _core(flavour, 0, pixels)
        try:
            for s in range(b, ids, K):
                core.render(s, 1, samples_per_pass=1)
            sums.append(core.accumulators()[0].copy())
            counts.append(len(range(b, ids, K)))
        finally:
            core.close()
    sums, counts = np.stack(sums), np.asarray(counts, U)
    sums.setflags(write=False)
    return sums, counts


@functools.lru_cache(maxsize=None)
def _plain(ids, per_pass, pixel_major, pixels, flavour="exact"):
    """the accumulators of a context that never had buckets"""
    core = _core(flavour, pixel_major, pixels)
    try:
        core.render(0, ids, samples_per_pass=per_pass)
        fm, sm = core.accumulators()
        return fm.copy(), sm.copy()
    finally:
        core.close()


def _check_buckets(core, K, ids, per_pass, pixel_major, pixels, flavour="exact"):
    core.render(0, ids, samples_per_pass=per_pass)
    sums, counts = core.buckets()
    want, want_counts = _bucket_reference(K, ids, pixels, flavour)
    where = "K = %d, passes of %d, %s slots, %s" % (K, per_pass, "pixel-major" if pixel_major else "sample-major", "full frame" if pixels is None else "strided list")
    assert np.array_equal(counts, want_counts), (where, counts, want_counts)
    for b in range(K):
        assert np.array_equal(_bits(sums[b]), _bits(want[b])), "%s: bucket %d: %d of %d words differ" % (where, b, int((_bits(sums[b]) != _bits(want[b])).sum()), want[b].size)
    fm, sm = core.accumulators()
    pfm, psm = _plain(ids, per_pass, pixel_major, pixels, flavour)
    assert np.array_equal(_bits(fm), _bits(pfm)) and np.array_equal(_bits(sm), _bits(psm)), where + ": the accumulators changed"
    assert float(sums.max()) > 0.0


@pytest.mark.parametrize("pixels", [None, STRIDED], ids=["frame", "strided"])
@pytest.mark.parametrize("pixel_major", [0, 1])
@pytest.mark.parametrize("K", [4, 5, 8])
def test_buckets_are_what_they_are_defined_to_be(K, pixel_major, pixels):
    ids = 2 * K + 3
    core = _core("exact", pixel_major, pixels, K)
    try:
        assert core.get_pixel_major() == pixel_major
        for per_pass in (1, 3, ids):
            core.clear()
            _check_buckets(core, K, ids, per_pass, pixel_major, pixels)
        st = core.firefly_stats()
        assert (st.buckets, st.bytes, st.samples, st.resolves) == (K, 12 * K * (P if pixels is None else len(pixels)), ids, 0)
    finally:
        core.close()


def test_buckets_in_the_fast_flavour():
    """One case in the fast flavour, in passes of one id: what a fast path computes may depend on the pass it shares with others (the reuse of ambient samples),
    so only a render in the reference's own passes can be asked for the reference's bits. Larger passes must still leave the accumulators as without buckets."""
    K, ids = 5, 13
    core = _core("fast", 1, None, K)
    try:
        _check_buckets(core, K, ids, 1, 1, None, "fast")
        core.clear()
        core.render(0, ids, samples_per_pass=ids)
        fm, sm = core.accumulators()
        pfm, psm = _plain(ids, ids, 1, None, "fast")
        assert np.array_equal(_bits(fm), _bits(pfm)) and np.array_equal(_bits(sm), _bits(psm))
        sums, counts = core.buckets()
        assert counts.tolist() == [3, 3, 3, 2, 2] and np.allclose(sums.sum(axis=0), fm, rtol=1e-4, atol=1e-5), "the buckets part the frame's sum"
    finally:
        core.close()


@pytest.mark.parametrize("pixel_major", [0, 1])
def test_two_calls_are_one_call_and_a_clear_zeroes_sums_and_counts(pixel_major):
    K = 5
    core = _core("exact", pixel_major, None, K)
    try:
        core.render(0, 11, samples_per_pass=3)
        one, one_counts = core.buckets()
        core.clear()
        zero, zero_counts = core.buckets()
        assert not _bits(zero).any() and not zero_counts.any(), "lumc_clear_accumulators zeroes the sums and the counts"
        assert not _bits(core.accumulators()[0]).any()
        core.render(0, 5, samples_per_pass=3)
        core.render(5, 6, samples_per_pass=3)
        two, two_counts = core.buckets()
        assert np.array_equal(_bits(one), _bits(two)) and np.array_equal(one_counts, two_counts) and one_counts.tolist() == [3, 2, 2, 2, 2]
        want, _ = _bucket_reference(K, 11, None)
        assert np.array_equal(_bits(two), _bits(want))
        core.set_pixels(None)  # a new pixel set: the planes are allocated again and zeroed
        zero, zero_counts = core.buckets()
        assert not _bits(zero).any() and not zero_counts.any()
    finally:
        core.close()


def test_the_bucket_count_is_refused_outside_4_to_16_and_changes_nothing():
    core = _core("exact", 0, None, 4)
    try:
        core.render(0, 4, samples_per_pass=4)
        before, counts = core.buckets()
        fm = core.accumulators()[0].copy()
        for K in (1, 3, 17, 1 << 30):
            with pytest.raises(CoreError) as e:
                core._call("lumc_set_firefly_buckets", C.c_uint32(K))
            assert "buckets" in str(e.value) and str(K) in str(e.value), str(e.value)
        after, after_counts = core.buckets()
        assert np.array_equal(_bits(before), _bits(after)) and np.array_equal(counts, after_counts) and np.array_equal(_bits(fm), _bits(core.accumulators()[0]))
        assert core.firefly_stats().buckets == 4
        core.set_firefly_buckets(16)
        assert core.firefly_stats().bytes == 16 * 12 * P and not _bits(core.accumulators()[0]).any(), "a new count clears the accumulators"
        core.set_firefly_buckets(0)
        assert core.firefly_stats().bytes == 0
        with pytest.raises(CoreError):
            core.buckets()
        with pytest.raises(CoreError) as e:
            core.firefly_resolve()
        assert "no buckets" in str(e.value)
    finally:
        core.close()


def _resolve_and_compare(core, image, what):
    sums, counts = core.buckets()
    got = core.firefly_resolve()
    st = core.firefly_stats()
    want, want_stats = firefly_resolve_host(sums, counts, image)
    assert np.array_equal(_bits(got), _bits(want)), "%s: %d of %d words differ from the twin" % (what, int((_bits(got) != _bits(want)).sum()), want.size)
    assert (st.last_rewritten, st.last_trimmed, st.last_nonfinite) == want_stats, (what, want_stats)
    untouched = (_bits(want) == _bits(image)).all(axis=0).reshape(-1)
    assert np.array_equal(_bits(got).reshape(3, -1)[:, untouched], _bits(image).reshape(3, -1)[:, untouched]), what + ": a pixel the twin leaves alone lost lumc_generate_result's bits"
    return want_stats, untouched


@pytest.mark.parametrize("K", [4, 8])
def test_the_resolve_kernel_is_the_twin(K):
    ids = 2 * K + 3
    core = _core("exact", 1, None, K)
    try:
        core.render(0, ids, samples_per_pass=ids)
        for lem in (False, True):
            image = core.generate_result(uniform_samples=ids, local_error_minimization=lem)
            stats, untouched = _resolve_and_compare(core, image, "K = %d, rendered buckets, lem %d" % (K, lem))
            assert stats[2] == 0 and 0 < untouched.sum(), "the rendered buckets are finite, and some pixels need no trimming"
        # chosen bucket words overwritten: pixel 0 gets a bucket of 1e6, pixel 63 a NaN channel, pixel 64 an Inf bucket, the last pixel no finite bucket at all
        sums, counts = core.buckets()
        sums = sums.copy()
        sums[1, :, 0] = 1.0e6
        sums[2, 1, 63] = np.nan
        sums[K - 1, :, 64] = np.inf
        sums[:, 0, P - 1] = np.nan
        sums[:, :, 65] = sums[0, :, 65][None, :] / F(counts[0]) * counts[:, None].astype(F)  # equal bucket means: left alone
        core.upload_buckets(sums)
        for lem in (False, True):
            image = core.generate_result(uniform_samples=ids, local_error_minimization=lem)
            stats, untouched = _resolve_and_compare(core, image, "K = %d, overwritten words, lem %d" % (K, lem))
            assert stats[0] > 0 and stats[1] > 0 and stats[2] == 3, stats
            out = core.firefly_resolve()  # (the image is resolved a second time: a resolved pixel is written again with the same value)
            assert not _bits(out)[:, (P - 1) // W, (P - 1) % W].any(), "no finite bucket: 0"
            assert np.isfinite(out).all()
        assert core.firefly_stats().resolves == 6
    finally:
        core.close()


def test_the_resolve_is_refused_where_it_cannot_run():
    core = _core("exact", 0, STRIDED, 4)
    try:
        core.render(0, 4, samples_per_pass=4)
        with pytest.raises(CoreError) as e:
            core.firefly_resolve()
        assert "pixel set" in str(e.value), str(e.value)
        core.set_pixels(None)
        core.render(0, 4, samples_per_pass=4)
        core.generate_result(uniform_samples=4)
        core.clear()
        with pytest.raises(CoreError) as e:
            core.firefly_resolve()
        assert "no bucket has samples" in str(e.value), str(e.value)
        core.adaptive_begin(4, 2, 1)
        with pytest.raises(CoreError) as e:
            core.firefly_resolve()
        assert "adaptive" in str(e.value), str(e.value)
    finally:
        core.close()


def test_the_preview_s_first_sample_lands_in_bucket_zero():
    """The undersampling schedule of stage 2 is every pixel's id 0; with the ids [1, 9) after it the buckets are those of a plain render of [0, 9)."""
    K = 4
    core = _core("exact", 0, None, K)
    try:
        schedule = undersampling_schedule(2)
        for n, (stage, it) in enumerate(schedule):
            core.render_undersampled(stage, it)
            assert core.buckets()[1].tolist() == [1 if n == len(schedule) - 1 else 0, 0, 0, 0], "id 0 counts when the schedule's last step has run"
        core.render(1, 8, samples_per_pass=3)
        got, counts = core.buckets()
        want, want_counts = _bucket_reference(K, 9, None)
        assert np.array_equal(counts, want_counts) and counts.tolist() == [3, 2, 2, 2]
        assert np.array_equal(_bits(got), _bits(want))
    finally:
        core.close()


# ---- the public switch ----
@contextlib.contextmanager
def _main_core(host, buckets=0):
    """The host's main context as a Core that does not own it."""
    core = Core.__new__(Core)
    core._lib, core._ctx = luminary_amd._lib(), C.c_void_p(host.core_context())
    core.width, core.height, core.num_pixels, core._firefly_buckets = W, H, P, buckets
    try:
        yield core
    finally:
        core._ctx = C.c_void_p()


def _host_image(host, spp):
    host.set_output_properties(W, H)
    host.render(spp)
    img, count, _ = host.get_image(host.acquire_output())
    assert count == spp
    return img


def _interleaved(planes):
    return np.ascontiguousarray(np.asarray(planes).reshape(3, H, W).transpose(1, 2, 0))


def test_the_host_switch(tmp_path):
    spp, K = 12, 4
    never = scenes.cornell_host(str(tmp_path / "never"), W, H, 3)
    host = scenes.cornell_host(str(tmp_path / "ff"), W, H, 3)
    try:
        img_never = _host_image(never, spp)
        fm_never, sm_never = never.accumulators()
        # off: a host that never heard of it
        host.set_firefly_rejection(enabled=True, buckets=K)
        host.set_firefly_rejection(enabled=False)
        assert np.array_equal(_host_image(host, spp), img_never), "disabled: nothing changes"
        fm, sm = host.accumulators()
        assert np.array_equal(_bits(fm), _bits(fm_never)) and np.array_equal(_bits(sm), _bits(sm_never))
        assert host.firefly_stats()["frames_resolved"] == 0 and host.firefly_stats()["bytes"] == 0
        # on: the setter restarts the integration
        host.set_firefly_rejection(enabled=True, buckets=K)
        assert host.is_rendering()[1] == 0, "the setter restarts the integration"
        img_on = _host_image(host, spp)  # (count == spp: the accumulation started over)
        st = host.firefly_stats()
        assert st["frames_resolved"] >= 1 and st["frames_skipped"] == 0 and st["buckets"] == K and st["bytes"] == 12 * K * P
        fm, sm = host.accumulators()
        assert np.array_equal(_bits(fm), _bits(fm_never)) and np.array_equal(_bits(sm), _bits(sm_never)), "the accumulators keep the plain sums"
        radiance, n = np.zeros((H, W, 3), F), C.c_uint32()
        get = luminary_amd._lib().luminary_ext_get_radiance
        get.restype = C.c_uint64
        assert get(host._h, radiance.ctypes.data_as(C.c_void_p), C.byref(n), C.c_uint32(W), C.c_uint32(H)) == 0 and n.value == spp
        # by hand: render, result image, the twin on the downloaded buckets
        core = Core(0)
        try:
            core.upload(oracle_lib.with_luts(host.device_scene()))
            core.set_pixels(None)
            core.set_firefly_buckets(K)
            core.render(0, spp, samples_per_pass=spp)
            image = core.generate_result(uniform_samples=spp)
            sums, counts = core.buckets()
        finally:
            core.close()
        robust, stats = firefly_resolve_host(sums, counts, image)
        assert stats[0] > 0, "some pixel of the box is rewritten at three ids per bucket"
        got = host.robust_radiance(W, H)
        assert np.array_equal(_bits(got), _bits(_interleaved(robust))), "luminary_ext_get_robust_radiance is the twin on lumc_generate_result's image"
        st = host.firefly_stats()
        assert (st["last_rewritten"], st["last_trimmed"], st["last_nonfinite"]) == stats
        want = oracle_lib.api_output(default_output_params(W, H, spp), robust)  # bloom with the camera's blend, then the display chain
        assert np.array_equal(img_on, want), "the delivered output is the chain run on the resolved image"
        assert not np.array_equal(img_on, img_never)
        # luminary_ext_get_denoised follows the outputs: it denoises the resolved image
        core = Core(0)
        try:
            core.upload(oracle_lib.with_luts(host.device_scene()))
            core.set_pixels(None)
            core.set_firefly_buckets(K)
            core.render(0, spp, samples_per_pass=spp)
            core.generate_result(uniform_samples=spp)
            assert np.array_equal(_bits(core.firefly_resolve()), _bits(robust))
            core.render_guides(host.get_denoiser().guide_samples)
            by_hand = core.denoise(None, uniform_samples=spp)
        finally:
            core.close()
        assert np.array_equal(_bits(host.denoised(W, H)), _bits(_interleaved(by_hand)))
        assert np.array_equal(_bits(radiance), _bits(_interleaved(fm_never.reshape(3, -1) * F(1.0 / spp)))), "luminary_ext_get_radiance keeps the plain mean"
        # a change of the bucket count restarts as well; the same count does not
        host.set_firefly_rejection(enabled=True, buckets=K)
        assert host.is_rendering()[1] == spp
        host.set_firefly_rejection(enabled=True, buckets=K + 1)
        assert host.is_rendering()[1] == 0
    finally:
        never.close()
        host.close()


def test_a_shutter_render_fills_the_buckets():
    """luminary_ext_render_shutter(host, 4, 2, 2) renders through lumc_render: eight ids in the buckets, which the twin resolves to the host's bits."""
    K = 4
    host = scenes.zoo_scene(W, H, 3)
    try:
        host.set_firefly_rejection(enabled=True, buckets=K)
        plain = [m for m in range(host.get_num_meshes()) if len(host.get_mesh(m)[3]) >= 8 and not any(host.get_material(int(i)).emission_active for i in set(host.get_mesh(m)[3]))]
        mesh = plain[0]
        host.shutter_open()
        host.set_mesh_positions(mesh, bend(host.get_mesh(mesh)[0], 0.3, 0.5))
        fn = luminary_amd._lib().luminary_ext_render_shutter
        fn.restype = C.c_uint64
        assert fn(host._h, C.c_uint32(4), C.c_uint32(2), C.c_uint32(2)) == 0
        assert host.is_rendering()[1] == 8
        with _main_core(host, K) as core:
            sums, counts = core.buckets()
            assert counts.tolist() == [2, 2, 2, 2]
            fm = host.accumulators()[0]
            assert np.allclose(sums.sum(axis=0), fm, rtol=1e-4, atol=1e-5) and float(sums.max()) > 0.0
            image = core.generate_result(uniform_samples=8)
        robust, stats = firefly_resolve_host(sums, counts, image)
        assert np.array_equal(_bits(host.robust_radiance(W, H)), _bits(_interleaved(robust)))
    finally:
        host.close()


def test_adaptive_sampling_is_skipped_and_counted(tmp_path):
    images = []
    for enabled in (False, True):
        host = scenes.cornell_host(str(tmp_path / ("a%d" % enabled)), W, H, 2)
        try:
            s = host.get_settings()
            s.enable_adaptive_sampling = True
            s.adaptive_sampling_update_interval = 2
            host.set_settings(s)
            host.set_firefly_rejection(enabled=enabled, buckets=4)
            host.set_output_properties(W, H)
            host.render(4)
            images.append(host.get_image(host.acquire_output())[0])
            st = host.firefly_stats()
            assert st["frames_resolved"] == 0 and (st["frames_skipped"] >= 1) == enabled, st
        finally:
            host.close()
    assert np.array_equal(images[0], images[1]), "adaptive sampling: the image is left alone"


def test_a_second_device_slot_makes_the_setter_fail(tmp_path, monkeypatch):
    monkeypatch.setenv("LUM_FAKE_DEVICES", "2")
    monkeypatch.setenv("LUM_MAX_DEVICES", "2")
    host = scenes.cornell_host(str(tmp_path / "two"), W, H, 2)
    try:
        assert host.get_device_count() == 2
        fn = luminary_amd._lib().luminary_ext_set_firefly_rejection
        fn.restype = C.c_uint64
        on = luminary_amd.FireflySettings(True, 8)
        assert fn(host._h, C.byref(on)) == INVALID_API_ARGUMENT
        assert not host.get_firefly_rejection().enabled
        off = luminary_amd.FireflySettings(False, 8)
        assert fn(host._h, C.byref(off)) == 0, "switching it off is always possible"
        host.set_device_enable(1, False)
        assert fn(host._h, C.byref(on)) == 0, "one slot left: accepted"
    finally:
        host.close()
