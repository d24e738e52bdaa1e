"""Denoiser: first-hit guides and the variance-guided a-trous filter (luminary_amd/csrc/device/dev_denoise.h; include/lum_core.h lumc_render_guides / lumc_denoise;
include/luminary_amd.h luminary_ext_set_denoiser).

The checker is tests/support/denoise_check.c, a plain-C restatement of prepare, a-trous and finish that takes log2 / exp2 from the test oracle. The CPU tests pin
the filter's properties on the restatement; the GPU tests hold the exact flavour to it bit for bit, the guides to the oracle's first-hit data, the fast flavour
to the exact one, and the host API to the chain done by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
from luminary_amd import scenes
from luminary_amd.core import Core, default_output_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CHECK = {}
LUM = np.array([0.212655, 0.715158, 0.072187], np.float32)


def _check_lib(tmp_path_factory):
    """tests/support/denoise_check.c, built like the other C checkers (no contraction), linked against the oracle library."""
    if "lib" not in _CHECK:
        oracle_lib.lib()  # builds oracle/_build/liboracle.so if needed
        d = tmp_path_factory.mktemp("dn_check")
        so = str(d / "denoise_check.so")
        build = os.path.join(ROOT, "oracle", "_build")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tests", "support", "denoise_check.c"),
                               "-o", so, "-L", build, "-loracle", "-Wl,-rpath," + build, "-lm"])
        _CHECK["lib"] = C.CDLL(so)
    return _CHECK["lib"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _restated(lib, image, fm, sm, samples, guides, iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_z=1.0):
    """image, fm [3, H, W]; sm, samples [H, W]; guides [7, H, W] (albedo, normal, depth). Returns (filtered image, filtered variance)."""
    _, h, w = image.shape
    img = np.ascontiguousarray(image, np.float32).copy()
    var = np.zeros((h, w), np.float32)
    fm, sm, guides = (np.ascontiguousarray(x, np.float32) for x in (fm, sm, guides))
    samples = np.ascontiguousarray(np.broadcast_to(samples, (h, w)), np.uint32)
    rc = lib.dn_denoise(C.c_uint32(w), C.c_uint32(h), C.c_uint32(iterations), C.c_float(sigma_l), C.c_float(sigma_n), C.c_float(sigma_z), _p(fm), _p(sm), _p(samples),
                        _p(guides), _p(img), _p(var))
    assert rc == 0
    return img, var


def _moments(mean, variance_of_mean, n):
    """Accumulators of n samples whose mean is `mean` [3, H, W] and whose luminance has the given variance of the mean [H, W] (float64 in, float32 out)."""
    mean = np.asarray(mean, np.float64)
    lum_sq = np.tensordot(LUM.astype(np.float64), mean * mean, axes=1)
    return (mean * n).astype(np.float32), (n * (lum_sq + n * np.asarray(variance_of_mean, np.float64))).astype(np.float32)


def _guides(h, w, albedo=1.0, normal=(0.0, 0.0, 1.0), depth=2.0):
    g = np.zeros((7, h, w), np.float32)
    g[0:3] = albedo
    g[3:6] = np.asarray(normal, np.float32).reshape(3, 1, 1)
    g[6] = depth
    return g


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU: the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------------

def test_normal_packing_round_trip(tmp_path_factory):
    """2 x snorm16 octahedral: the axes are exact (orthogonal faces get a dot product of exactly 0), anything else within 2^-14."""
    lib = _check_lib(tmp_path_factory)
    rng = np.random.RandomState(3)
    v = rng.normal(size=(2000, 3)).astype(np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v = np.concatenate([np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], np.float32), v.astype(np.float32)])
    out = np.zeros_like(v)
    for i in range(v.shape[0]):
        lib.dn_normal_roundtrip(_p(v[i:i + 1]), _p(out[i:i + 1]))
    assert np.array_equal(out[:6], v[:6])
    assert np.abs(out - v).max() < 2.0 ** -13


def test_a_constant_image_stays_constant(tmp_path_factory):
    """A weighted mean of equal values: each of the 25 products and sums rounds once (2^-24 relative), five iterations: within 5 * 26 * 2^-24 < 1e-5."""
    lib = _check_lib(tmp_path_factory)
    h, w = 40, 50
    rng = np.random.RandomState(1)
    image = np.empty((3, h, w), np.float32)
    image[0], image[1], image[2] = 0.7, 0.3, 1.9
    variance = rng.uniform(0.0, 0.5, (h, w))
    fm, sm = _moments(image, variance, 16)
    out, _ = _restated(lib, image, fm, sm, 16, _guides(h, w, albedo=0.5))
    assert np.allclose(out, image, rtol=1e-5, atol=0.0)


def test_a_converged_image_passes_through_bit_for_bit(tmp_path_factory):
    lib = _check_lib(tmp_path_factory)
    h, w = 33, 47
    rng = np.random.RandomState(2)
    image = rng.uniform(0.0, 3.0, (3, h, w)).astype(np.float32)
    g = _guides(h, w)
    g[0:3] = rng.uniform(0.0, 1.0, (3, h, w))  # x / a * a is not x: the filter must not go that way
    g[6, :5] = -1.0
    fm = image * np.float32(8)
    sm = (np.tensordot(LUM, (fm / np.float32(8)) ** 2, axes=1) * np.float32(8)).astype(np.float32)
    sm *= np.float32(1.0 - 2.0 ** -20)  # a second moment at or just below the squared mean: variance max(0, .) = 0
    out, var = _restated(lib, image, fm, sm, 8, g)
    assert (var == 0).all()
    assert np.array_equal(out.view(np.uint32), image.view(np.uint32))


def _b3_factors(iterations):
    """Variance left by the B3 a-trous filter with all edge weights 1 at an interior pixel of independent noise: the product of sum(h^2) over the iterations
    (every level as if its input were independent), and sum(H^2) of the composite kernel H (what the levels' shared taps really leave)."""
    k = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
    per_level = (k ** 2).sum() ** 2
    comp = np.array([1.0])
    for i in range(iterations):
        d = np.zeros(4 * (1 << i) + 1)
        d[::1 << i] = k
        comp = np.convolve(comp, d)
    return per_level ** iterations, (comp ** 2).sum() ** 2


def test_edges_stop_the_filter_and_the_noise_falls_by_the_b3_factor(tmp_path_factory):
    """Two half-planes with orthogonal normals and different colours, noise of known variance. No output pixel depends on the other side (one side's colour is
    changed, the other side's output compared bit for bit), and the noise variance inside each side falls by the B3 kernel's factor.
    The factor: sum(h^2) = (2/256 + 2/16 + 9/64)^2 = 0.074768 per level. One iteration leaves exactly that of independent noise; the estimate over the N = 40 x 30
    interior pixels, whose filtered noise is correlated over 5 x 5, has a relative deviation of about sqrt(2 * 25 / N) = 0.2: margin 1.6 (3 sigma). Five iterations:
    the product 0.074768^5 = 2.3e-6 would need independent levels and a support of 125 pixels; the levels share taps, so what an unbounded plane keeps is sum(H^2)
    of the composite kernel (printed: 2.3e-4). What is measured is the variance inside a 40 x 30 window about its own mean, which does not see the residue's slow
    part and so comes out below sum(H^2) (2e-5 to 3e-5). Asserted for five iterations: the variance falls again by more than 10 from the first iteration's (the
    composite kernel's factor against one level's is 300), and never below the product."""
    lib = _check_lib(tmp_path_factory)
    h, w, n, sigma = 64, 96, 16, 0.05
    rng = np.random.RandomState(5)
    noise = rng.normal(0.0, sigma, (h, w))
    left = np.arange(w) < w // 2

    def scene(left_colour):
        clean = np.empty((3, h, w))
        clean[:, :, left] = np.asarray(left_colour).reshape(3, 1, 1)
        clean[:, :, ~left] = np.asarray((0.2, 0.5, 0.9)).reshape(3, 1, 1)
        image = (clean + noise).astype(np.float32)  # grey noise: its luminance variance is sigma^2
        fm, sm = _moments(image, np.full((h, w), sigma ** 2), n)
        g = _guides(h, w)
        g[3:6, :, left] = np.array([1.0, 0.0, 0.0], np.float32).reshape(3, 1, 1)
        return clean, image, fm, sm, g

    # sigma_luminance so wide that the luminance weight is 1: the taps inside a side carry the plain B3 weights
    results = {}
    for iterations in (1, 5):
        clean, image, fm, sm, g = scene((0.9, 0.4, 0.1))
        out, _ = _restated(lib, image, fm, sm, n, g, iterations=iterations, sigma_l=1e6)
        _, image2, fm2, sm2, g2 = scene((0.1, 0.2, 3.0))
        out2, _ = _restated(lib, image2, fm2, sm2, n, g2, iterations=iterations, sigma_l=1e6)
        assert np.array_equal(out[:, :, ~left].view(np.uint32), out2[:, :, ~left].view(np.uint32)), "the right side does not see the left side's colour"
        assert not np.array_equal(out[:, :, left], out2[:, :, left])
        ratios = []
        for side in (slice(4, 44), slice(52, 92)):
            res = (out.astype(np.float64) - clean)[1, 17:47, side]
            ratios.append(res.var() / sigma ** 2)
        results[iterations] = ratios
    product1, _ = _b3_factors(1)
    product5, composite5 = _b3_factors(5)
    print("variance kept: 1 iteration %s (sum h^2 = %.6f), 5 iterations %s (product %.3g, composite kernel %.3g)" % (results[1], product1, results[5], product5, composite5))
    assert abs(product1 - 0.074768) < 1e-6
    for r in results[1]:
        assert product1 / 1.6 < r < product1 * 1.6
    for r1, r5 in zip(results[1], results[5]):
        assert product5 <= r5 < r1 / 10.0
    # with the default sigma_luminance the filter is gentler, and still removes most of the noise without crossing the edge
    clean, image, fm, sm, g = scene((0.9, 0.4, 0.1))
    out, var = _restated(lib, image, fm, sm, n, g)
    assert ((out.astype(np.float64) - clean)[:, 17:47, 4:44]).var() < 0.1 * sigma ** 2
    assert np.abs(out[:, :, left].astype(np.float64).mean(axis=(1, 2)) - (0.9, 0.4, 0.1)).max() < 0.01, "nothing of the other side's colour leaks in"
    assert var[17:47, 4:44].mean() < 0.1 * (sigma ** 2)


def test_demodulation_keeps_texture_detail(tmp_path_factory):
    """A checkerboard albedo times a smooth irradiance, plus noise: the filter works on the irradiance, so the checkerboard keeps its contrast and the error
    against the noise-free image falls."""
    lib = _check_lib(tmp_path_factory)
    h, w, n = 64, 64, 8
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    checker = np.where(((xs // 2) + (ys // 2)) % 2 == 0, 0.9, 0.2)
    irradiance = 1.0 + 0.5 * np.sin(xs / 20.0) * np.cos(ys / 25.0)
    clean = np.stack([checker * irradiance] * 3)
    rng = np.random.RandomState(9)
    sigma_irr = 0.15
    noise = rng.normal(0.0, sigma_irr, (h, w)) * checker  # noise of the incoming light, seen through the albedo
    image = (clean + noise).astype(np.float32)
    fm, sm = _moments(image, (sigma_irr * checker) ** 2, n)
    g = _guides(h, w)
    g[0:3] = checker
    out, _ = _restated(lib, image, fm, sm, n, g)
    err_in = ((image.astype(np.float64) - clean) ** 2).mean()
    err_out = ((out.astype(np.float64) - clean) ** 2).mean()
    bright, dark = checker > 0.5, checker < 0.5
    contrast_clean = clean[0][bright].mean() / clean[0][dark].mean()
    contrast_out = out[0][bright].mean() / out[0][dark].mean()
    print("demodulation: mse in %.3g out %.3g, contrast clean %.4f out %.4f" % (err_in, err_out, contrast_clean, contrast_out))
    assert err_out < 0.2 * err_in
    assert abs(contrast_out / contrast_clean - 1.0) < 0.02
    flat = _guides(h, w)  # the same filter without the albedo guide blurs the checkerboard or leaves the noise: either way a larger error
    out_flat, _ = _restated(lib, image, fm, sm, n, flat)
    assert ((out_flat.astype(np.float64) - clean) ** 2).mean() > 2.0 * err_out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------------------

def _oracle_debug(view_host, mode, w, h):
    st = view_host.get_settings()
    st.shading_mode = mode
    view_host.set_settings(st)
    view = oracle_lib.with_luts(view_host.device_scene())
    fm, _, _ = oracle_lib.render(view, 0, 1)
    return fm.reshape(3, h, w)


def _oracle_first_hits(view, w, h):
    l = oracle_lib.lib()
    o, d = np.zeros((w * h, 3), np.float32), np.zeros((w * h, 3), np.float32)
    ray = (C.c_float * 6)()
    for p in range(w * h):
        l.oracle_camera_ray(C.byref(view), C.c_uint32(p % w), C.c_uint32(p // w), C.c_uint32(0), ray)
        o[p], d[p] = list(ray)[:3], list(ray)[3:]
    return oracle_lib.trace_closest(view, o, d, np.full((w * h, 2), 0xFFFFFFFF, dtype=np.uint32))


@pytest.mark.gpu
def test_guides_equal_the_oracles_first_hit_data():
    """Material zoo, sample id 0: albedo against the oracle's ALBEDO image (albedo + emission; emitters, which the LIGHTS image names, have guide albedo 1), the
    signed normal against the oracle's NORMAL image (saturated: it pins the positive components, the others must be <= 0, the length 1), the distance against
    the oracle's closest hit of the oracle's camera ray; all bit for bit, misses flagged by depth -1."""
    w, h = 96, 64
    host = scenes.zoo_scene(w, h, 8)
    view = oracle_lib.with_luts(host.device_scene())
    core = Core(0)
    try:
        core.upload(view)
        albedo, normal, depth = core.render_guides(1)
    finally:
        core.close()
    hits = _oracle_first_hits(view, w, h)
    hit = (hits[:, 0] <= 0x7FFFFFFF).reshape(h, w)
    want_t = hits[:, 2].copy().view(np.float32).reshape(h, w)
    assert 0.2 < hit.mean() < 1.0, "an open sky: some rays miss"
    assert np.array_equal(depth[hit].view(np.uint32), want_t[hit].view(np.uint32))
    assert (depth[~hit] == -1.0).all() and (normal[:, ~hit] == 0.0).all() and (albedo[:, ~hit] == 1.0).all()
    o_albedo, o_normal, o_lights = (_oracle_debug(host, m, w, h) for m in (1, 3, 5))
    emitter = hit & (o_lights > np.float32(0.025)).any(axis=0)  # albedo * 0.025 + emission with albedo <= 1
    assert emitter.any() and (albedo[:, emitter] == 1.0).all()
    plain = hit & ~emitter
    assert np.array_equal(albedo[:, plain].view(np.uint32), o_albedo[:, plain].view(np.uint32))
    assert (albedo[:, plain] != 1.0).any()
    pos = (o_normal > 0) & hit
    assert np.array_equal(normal[pos].view(np.uint32), o_normal[pos].view(np.uint32))
    assert (normal[(o_normal == 0) & hit] <= 0.0).all() and (normal[:, hit] < 0.0).any(), "signed: the debug image's zeros are the negative components"
    # a direction, not a scaled one: instance rotations are 16-bit quaternions (unit within a few 2^-15), vertex normals are packed
    assert np.abs(np.linalg.norm(normal[:, hit].astype(np.float64), axis=0) - 1.0).max() < 2.0 ** -12


@pytest.mark.gpu
def test_guides_follow_a_physical_cameras_rays():
    """With a physical camera the guide's distance is the closest hit of the lens's outgoing ray; pixels whose ray does not leave the lens are misses."""
    import test_physical_camera as tpc
    w, h = 96, 64
    host = tpc._host(w, h, plane_z=-3.0, rot=(0.0, 0.5, 0.0))  # a wall seen at an angle: the distance varies over the frame
    core, view = tpc._core_for(host)
    try:
        _, normal, depth = core.render_guides(1)
        o, d, weight = core.camera_rays(np.arange(w * h, dtype=np.uint32), 0, 1)
        hits = core.trace_closest_host(o, d, np.full((w * h, 2), 0xFFFFFFFF, dtype=np.uint32))
        thin = Core(0)
        try:
            thin.upload(view)
            _, _, depth_thin = thin.render_guides(1)
        finally:
            thin.close()
    finally:
        core.close()
        host.close()
    valid = (weight > 0).reshape(h, w)
    hit = valid & (hits[:, 0] <= 0x7FFFFFFF).reshape(h, w)
    t = hits[:, 2].copy().view(np.float32).reshape(h, w)
    assert hit.sum() > 100 and (~valid).any()
    assert np.array_equal(depth[hit].view(np.uint32), t[hit].view(np.uint32))
    assert (depth[~hit] == -1.0).all()
    assert not np.array_equal(depth, depth_thin)


def _pixel_samples(core, w, h):
    info = core.adaptive_info()
    counts, _ = core.adaptive_download()
    out = np.zeros(w * h, dtype=np.uint32)
    ex = np.asarray(info["executions"], dtype=np.uint32)
    oracle_lib.lib().oracle_pixel_samples(C.c_uint32(w), C.c_uint32(h), _p(ex), _p(counts), _p(out))
    return out.reshape(h, w)


@pytest.mark.gpu
def test_the_exact_flavour_equals_the_restatement_bit_for_bit(tmp_path_factory):
    """lumc_denoise against tests/support/denoise_check.c fed with the downloaded guides and accumulators: a frame that is no multiple of the 32 x 8 tile,
    iterations 1 to 6, the LDS and the direct form of the iterations with taps 1 and 2 apart (which also agree with each other), and an adaptive accumulation
    with per-pixel sample counts."""
    lib = _check_lib(tmp_path_factory)
    w, h, spp = 75, 45, 6
    host = scenes.cornell_host(str(tmp_path_factory.mktemp("dn_cornell")), w, h, 3)
    view = oracle_lib.with_luts(host.device_scene())
    core = Core(0)
    try:
        assert core.flavour == "exact"
        core.upload(view)
        core.set_pixels(None)
        core.render(0, spp, samples_per_pass=spp)
        fm, sm = core.accumulators()
        image = core.generate_result(uniform_samples=spp)
        guides = np.concatenate([x.reshape(-1, h, w) for x in core.render_guides(4)])
        changed = 0
        for iterations in range(1, 7):
            want, _ = _restated(lib, image, fm.reshape(3, h, w), sm.reshape(h, w), spp, guides, iterations=iterations)
            got = {}
            for lds in (True, False):
                core.set_denoise_form(lds)
                got[lds] = core.denoise(image, uniform_samples=spp, iterations=iterations)
                bad = int((got[lds].view(np.uint32) != want.view(np.uint32)).sum())
                assert bad == 0, "iterations %d, lds %s: %d of %d values differ, max %g" % (iterations, lds, bad, want.size, np.abs(got[lds] - want).max())
            assert np.array_equal(got[True].view(np.uint32), got[False].view(np.uint32))
            changed += int((want != image).sum())
        assert changed > 6 * w * h, "the filter did something"
        # in place on the context's result image, and a different set of widths
        core.set_denoise_form(True)
        in_place = core.denoise(None, uniform_samples=spp, sigma_luminance=2.0, sigma_normal=32.0, sigma_depth=3.0)
        want, _ = _restated(lib, image, fm.reshape(3, h, w), sm.reshape(h, w), spp, guides, sigma_l=2.0, sigma_n=32.0, sigma_z=3.0)
        assert np.array_equal(in_place.view(np.uint32), want.view(np.uint32))
        # adaptive accumulation: every pixel normalises by its own sample count
        core.adaptive_begin(8, 3, 2)
        core.adaptive_render(7)
        core.synchronize()
        samples = _pixel_samples(core, w, h)
        assert len(np.unique(samples)) > 1
        fm, sm = core.accumulators()
        image = core.generate_result()
        guides = np.concatenate([x.reshape(-1, h, w) for x in core.render_guides(4)])
        want, _ = _restated(lib, image, fm.reshape(3, h, w), sm.reshape(h, w), samples, guides)
        for lds in (True, False):
            core.set_denoise_form(lds)
            got = core.denoise(image)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "adaptive, lds %s" % lds
        assert (want != image).any()
    finally:
        core.close()


# measured on the MI355X (Cornell box 75 x 45, 6 spp, 5 iterations): see the docstring of the test below
FAST_FLAVOUR_MEASURED = 1.12e-6


@pytest.mark.gpu
def test_the_fast_flavour_stays_close_to_the_exact_one(tmp_path_factory):
    """The same accumulators, guides and image through both flavours of the filter. Measured on the MI355X: the largest relative difference of a value is 1.12e-6
    (mean 1.5e-7; relative to the value, or to a thousandth of the image's mean where the value is smaller). The assertion is four times that figure."""
    w, h, spp = 75, 45, 6
    host = scenes.cornell_host(str(tmp_path_factory.mktemp("dn_cornell")), w, h, 3)
    view = oracle_lib.with_luts(host.device_scene())
    core = Core(0)
    try:
        core.upload(view)
        core.set_pixels(None)
        core.render(0, spp, samples_per_pass=spp)
        image = core.generate_result(uniform_samples=spp)
        core.render_guides(4)
        exact = core.denoise(image, uniform_samples=spp)
        core.set_flavour("fast")
        fast = core.denoise(image, uniform_samples=spp)
    finally:
        core.close()
    rel = np.abs(fast.astype(np.float64) - exact) / np.maximum(np.abs(exact.astype(np.float64)), 1e-3 * float(exact.mean()))
    print("fast flavour: max relative difference %.3g, mean %.3g" % (rel.max(), rel.mean()))
    assert FAST_FLAVOUR_MEASURED is not None, "not yet measured on the GPU"
    assert rel.max() < 4.0 * FAST_FLAVOUR_MEASURED


def _rel_mse(img, ref):
    img, ref = img.astype(np.float64), ref.astype(np.float64)
    return float((((img - ref) ** 2) / (ref ** 2 + 1e-2)).mean())


@pytest.mark.gpu
def test_denoised_cornell_box_beats_the_raw_image_at_16_spp(tmp_path_factory):
    """Cornell box, 256 x 256, exact flavour. Yardstick: the undenoised render of 4096 spp from this same test. At 16 spp the denoised image's relative MSE must be
    below the raw image's. The ratios at 4, 16, 64, 256 and 1024 spp are printed (DESIGN section 7 records them). Measured on the MI355X: 0.024, 0.047, 0.133, 0.40 and
    1.12 - at 1024 spp the filter's bias is larger than the noise it removes; the denoised 16-spp image has the error of a raw image of about 270 spp."""
    w = h = 256
    host = scenes.cornell_host(str(tmp_path_factory.mktemp("dn_cornell")), w, h, 4)
    view = oracle_lib.with_luts(host.device_scene())
    core = Core(0)
    stops = (4, 16, 64, 256, 1024, 4096)
    raw, den = {}, {}
    try:
        core.upload(view)
        core.set_pixels(None)
        core.render_guides(4)
        done = 0
        for spp in stops:
            core.render(done, spp - done, samples_per_pass=min(spp - done, 64))
            done = spp
            raw[spp] = core.generate_result(uniform_samples=spp)
            if spp <= 1024:
                den[spp] = core.denoise(raw[spp], uniform_samples=spp)
    finally:
        core.close()
    ref = raw[4096]
    figures = {spp: (_rel_mse(raw[spp], ref), _rel_mse(den[spp], ref)) for spp in den}
    for spp, (r, d) in figures.items():
        print("cornell %4d spp: relMSE raw %.4g denoised %.4g ratio %.3f" % (spp, r, d, d / r))
    print("raw relMSE by spp: " + ", ".join("%d: %.4g" % (s, _rel_mse(raw[s], ref)) for s in stops[:-1]))
    assert figures[16][1] < figures[16][0]


def _host_image(host, w, h, spp):
    host.set_output_properties(w, h)
    host.render(spp)
    img, count, _ = host.get_image(host.acquire_output())
    assert count == spp
    return img


@pytest.mark.gpu
def test_the_host_api_applies_the_denoiser_between_result_and_bloom(tmp_path, monkeypatch):
    """Enabled: the ARGB8 image equals core result -> lumc_denoise -> bloom -> output done by hand. Disabled: today's bytes (a host that never heard of the
    denoiser). Debug shading modes, non-beauty output modes and the undersampling preview are not filtered. Eight device slots give the one-device image."""
    w, h, spp = 100, 70, 5
    never = scenes.cornell_host(str(tmp_path / "never"), w, h, 3)
    img_never = _host_image(never, w, h, spp)

    host = scenes.cornell_host(str(tmp_path / "dn"), w, h, 3)
    d = host.get_denoiser()
    assert (d.enabled, d.guide_samples, d.iterations, d.sigma_luminance, d.sigma_normal, d.sigma_depth) == (False, 4, 5, 4.0, 128.0, 1.0)
    host.set_denoiser(enabled=True)
    host.set_denoiser(enabled=False)
    assert np.array_equal(_host_image(host, w, h, spp), img_never), "disabled: nothing changes"
    host.set_denoiser(enabled=True, guide_samples=2)
    assert host.get_denoiser().enabled and host.get_denoiser().guide_samples == 2
    host.render(1)  # setting it does not restart: one more sample
    img_on, count, _ = host.get_image(host.acquire_output())
    assert count == spp + 1 and not np.array_equal(img_on, img_never)

    view = oracle_lib.with_luts(host.device_scene())
    core = Core(0)
    try:
        core.upload(view)
        core.set_pixels(None)
        core.render(0, spp + 1, samples_per_pass=spp + 1)
        core.generate_result(uniform_samples=spp + 1)
        core.render_guides(2)
        by_hand = core.denoise(None, uniform_samples=spp + 1)
    finally:
        core.close()
    want = oracle_lib.api_output(default_output_params(w, h, spp + 1), by_hand)  # bloom with the camera's blend, then the display chain
    assert np.array_equal(img_on, want)
    # the float image, and the undenoised one next to it
    den = host.denoised(w, h)
    assert np.array_equal(den.transpose(2, 0, 1).reshape(3, h, w).view(np.uint32), by_hand.view(np.uint32))

    # what is not filtered: an enabled denoiser changes nothing there
    for case in ("debug", "variance", "preview"):
        images = []
        for enabled in (False, True):
            hst = scenes.cornell_host(str(tmp_path / ("%s%d" % (case, enabled))), w, h, 3)
            st = hst.get_settings()
            if case == "debug":
                st.shading_mode = 1
            elif case == "variance":
                st.adaptive_sampling_output_mode = 1
            else:
                st.undersampling = 2
            hst.set_settings(st)
            hst.set_denoiser(enabled=enabled)
            hst.set_output_properties(w, h)
            if case == "preview":
                hst.render(1)  # with a recurring output and undersampling the first allocation is a coarse preview stage
                images.append(hst.get_image(hst.acquire_output())[0])
            else:
                images.append(_host_image(hst, w, h, 3))
            hst.close()
        assert np.array_equal(images[0], images[1]), case

    monkeypatch.setenv("LUM_FAKE_DEVICES", "8")
    monkeypatch.setenv("LUM_MAX_DEVICES", "8")
    multi = scenes.cornell_host(str(tmp_path / "eight"), w, h, 3)
    assert multi.get_device_count() == 8
    multi.set_denoiser(enabled=True, guide_samples=2)
    assert np.array_equal(_host_image(multi, w, h, spp + 1), img_on), "eight device slots: the one-device image"
