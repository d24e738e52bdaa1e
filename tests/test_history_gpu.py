"""Image history on the device (csrc/host/history.hip k_history_reproject, k_history_blend; include/lum_core.h lumc_history_carry / lumc_history_blend;
include/luminary_amd.h luminary_ext_set_history). Exact flavour (one case in the fast one); tests/test_history.py holds the twins to the definition.

  kernels   both kernels equal the twins byte for byte, counters included, on the synthetic planes of the CPU test at 7 x 5 (less than a wave), 50 x 31 (a
            part-empty last wave and workgroup) and 64 x 64 (exact 32 x 8 tiles), for every camera key, with the clamp off and on (one form of the blend is built).
  host      on zoo_scene(50, 31): the image shown after a camera move is the twins fed with what the public getters return; the drops; off is off.
  effect    on the Cornell box at 48 x 32 the shown image of 1 id + history is closer to a converged render than the plain 1-id image.

The move of the end-to-end cases - 0.3 along x, 0.1 along y, a yaw of 0.03 - was chosen by running the twin on the guides of a few candidates: the twin carries 1086 of
the 1550 pixels, rejects 455 (the objects' silhouettes and the glass, whose averaged guides fail the depth and normal tests) and finds 9 off the old frame; larger
moves carry less than half, a pure translation of 0.1 rejects almost nothing. The conditions are on the twin's counters: at least half carried, at least one rejected."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import history_cases as H
import luminary_amd
from luminary_amd import core as lumcore
from luminary_amd import scenes
from luminary_amd.core import Core

pytestmark = pytest.mark.gpu
F, U = np.float32, np.uint32
W, HT = 50, 31
P = W * HT
KEYS = ("identical", "translated", "rotated", "fov", "turned", "half_off")
MOVE = ((0.3, 0.1, 0.0), 0.03)  # translation, yaw


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(U)


def _planar(img):
    """[H, W, 3] -> [3, P]"""
    return np.ascontiguousarray(np.asarray(img, F).transpose(2, 0, 1)).reshape(3, -1)


@contextlib.contextmanager
def _main_core(host, w=W, h=HT):
    """The host's main context as a Core that does not own it."""
    core = Core.__new__(Core)
    core._lib, core._ctx = luminary_amd._lib(), C.c_void_p(host.core_context())
    core.width, core.height, core.num_pixels = w, h, w * h
    try:
        yield core
    finally:
        core._ctx = C.c_void_p()


def _move(host, translation=MOVE[0], yaw=MOVE[1]):
    c = host.get_camera()
    c.pos.x += translation[0]
    c.pos.y += translation[1]
    c.pos.z += translation[2]
    c.rotation.y += yaw
    host.set_camera(c)


def _params(host):
    s = host.get_history()
    return lumcore.history_params(True, s.max_history, s.depth_tolerance, s.normal_threshold, s.clamp_sigma)


def _frame_state(host, w=W, h=HT):
    """what the public getters say about the frame as it was last shown: shown [3, P], weight [P], normal [3, P], depth [P], the denoised image [3, P], the camera key"""
    shown, weight = host.history_image(w, h)
    _, normal, depth = host.first_hit_guides(w, h)
    with _main_core(host, w, h) as core:
        state_key, current = core.history_keys()
    assert bytes(state_key) == bytes(current), "the state was shown from the camera as it stands"
    return {"shown": _planar(shown), "weight": weight.reshape(-1), "normal": normal.reshape(3, -1), "depth": depth.reshape(-1), "cur": _planar(host.denoised(w, h)), "key": current}


# ---- 1. the kernels equal the twins ----
@pytest.fixture(scope="module")
def device():
    core = Core(0)
    yield core
    core.close()


@pytest.mark.parametrize("name", KEYS)
@pytest.mark.parametrize("frame", H.FRAMES)
def test_the_kernels_equal_the_twins(device, frame, name):
    old, now = H.keys(*frame)[name]
    for random_guides in (False, True):
        pl = H.planes(old, now, seed=frame[0] + 100 * KEYS.index(name), random_guides=random_guides)
        for clamp in (0.0, 1.5):
            st = lumcore.history_params(clamp_sigma=clamp)
            c, w, stats = lumcore.history_reproject_host(now, old, st, pl["normal"], pl["depth"], pl["old_shown"], pl["old_weight"], pl["old_normal"], pl["old_depth"])
            image, shown, weight = lumcore.history_blend_host(st, now.width, now.height, 3, pl["image"], c, w)
            got = device.history_kernels(now, old, st, 3, pl["image"], pl["normal"], pl["depth"], pl["old_shown"], pl["old_weight"], pl["old_normal"], pl["old_depth"])
            what = (random_guides, clamp)
            assert got["stats"] == stats, what
            for k, want in (("carried", c), ("carried_weight", w), ("image", image), ("shown", shown), ("weight", weight), ("state_normal", pl["normal"]), ("state_depth", pl["depth"])):
                assert H.same_bits(got[k], want), (k, what)
    if name == "identical":
        assert stats[0] > 0
    if name == "turned":
        assert stats == (0, 0, frame[0] * frame[1])


# ---- 2. / 6. end to end ----
def _end_to_end(host):
    host.set_denoiser(enabled=True)
    host.set_history(enabled=True)
    host.set_output_properties(W, HT)
    host.render(32)
    assert host.get_image(host.acquire_output())[1] == 32
    before = _frame_state(host)
    assert np.array_equal(_bits(before["shown"]), _bits(before["cur"])) and (before["weight"] == F(32)).all(), "nothing carried yet: the shown image is the chain's, the weight its samples"
    assert host.history_stats()["frames_carried"] == 0 and host.history_stats()["valid"] == 1
    _move(host)
    assert host.is_rendering()[1] == 0, "the move restarts the integration"
    host.render(1)
    assert host.get_image(host.acquire_output())[1] == 1
    after = _frame_state(host)
    st = _params(host)
    carried, cw, stats = lumcore.history_reproject_host(after["key"], before["key"], st, after["normal"], after["depth"], before["shown"], before["weight"], before["normal"], before["depth"])
    print("end to end: carried, rejected, off =", stats, "of", P)
    assert stats[0] >= P // 2 and stats[1] >= 1, "the twin carries at least half of the frame and rejects something"
    image, shown, weight = lumcore.history_blend_host(st, W, HT, 1, after["cur"], carried, cw)
    assert np.array_equal(_bits(after["shown"]), _bits(shown)), "the shown image is the twins' on the getters' planes"
    assert np.array_equal(_bits(after["weight"]), _bits(weight))
    assert not np.array_equal(_bits(shown), _bits(after["cur"])), "the history changed the image"
    hs = host.history_stats()
    assert (hs["last_carried"], hs["last_rejected"], hs["last_off"]) == stats and hs["frames_carried"] == 1 and hs["frames_dropped"] == 0 and hs["bytes"] == 48 * P
    with _main_core(host) as core:
        _, _, c_dev, cw_dev = core.download_history()
    assert np.array_equal(_bits(c_dev), _bits(carried)) and np.array_equal(_bits(cw_dev), _bits(cw))
    # a second output of the same accumulation sees the same C and W
    host.render(1)
    cur2 = _planar(host.denoised(W, HT))
    _, shown2, weight2 = lumcore.history_blend_host(st, W, HT, 2, cur2, carried, cw)
    again = host.history_image(W, HT)
    assert np.array_equal(_bits(_planar(again[0])), _bits(shown2)) and np.array_equal(_bits(again[1].reshape(-1)), _bits(weight2))
    assert host.history_stats()["frames_carried"] == 1


def test_end_to_end_the_shown_image_is_the_twins():
    host = scenes.zoo_scene(W, HT, 3)
    try:
        _end_to_end(host)
    finally:
        host.close()


def test_end_to_end_in_the_fast_flavour(monkeypatch):
    """the unit is shared between the flavours: the fast flavour's planes through the same kernels equal the twins fed by those planes"""
    monkeypatch.setenv("LUM_FLAVOUR", "fast")
    host = scenes.zoo_scene(W, HT, 3)
    try:
        _end_to_end(host)
    finally:
        host.close()


# ---- 3. the effect ----
def test_history_brings_the_first_sample_closer_to_the_converged_image(tmp_path):
    """Cornell box, 48 x 32: 64 ids, a move of 0.1 along x with a yaw of 0.02, 1 id. Mean squared error against 1024 ids of the moved camera: shown (1 id + history)
    strictly below the plain 1-id image. Measured on one MI355X, exact flavour: the ratio shown / plain is printed below and recorded in DESIGN.md section 17."""
    w, h = 48, 32
    host = scenes.cornell_host(str(tmp_path / "a"), w, h, 3)
    ref = scenes.cornell_host(str(tmp_path / "b"), w, h, 3)
    try:
        host.set_history(enabled=True)
        host.set_output_properties(w, h)
        host.render(64)
        _move(host, (0.1, 0.0, 0.0), 0.02)
        host.render(1)
        shown = host.history_image(w, h)[0].astype(np.float64)
        fm, _ = host.accumulators()
        plain = fm.reshape(3, h, w).transpose(1, 2, 0).astype(np.float64)  # one id: the sums are the image
        assert host.history_stats()["frames_carried"] == 1
        _move(ref, (0.1, 0.0, 0.0), 0.02)
        ref.render(1024)
        fm, _ = ref.accumulators()
        truth = fm.reshape(3, h, w).transpose(1, 2, 0).astype(np.float64) / 1024.0
        mse_shown, mse_plain = float(((shown - truth) ** 2).mean()), float(((plain - truth) ** 2).mean())
        print("effect: mse shown %.6g, plain %.6g, ratio %.4f" % (mse_shown, mse_plain, mse_shown / mse_plain))
        assert mse_shown < mse_plain
    finally:
        host.close()
        ref.close()


# ---- 4. drops ----
def _shown_is_the_chain_without_history(host, samples, w=W, h=HT):
    shown, weight = host.history_image(w, h)
    assert np.array_equal(_bits(shown), _bits(host.denoised(w, h))), "the shown image has the bytes of the chain without history"
    assert (weight == F(samples)).all()


def test_every_other_restart_drops_and_names_its_cause():
    host = scenes.zoo_scene(W, HT, 3)
    try:
        host.set_denoiser(enabled=True)
        host.set_history(enabled=True)
        host.set_output_properties(W, HT)
        host.render(8)
        drops = 0

        def dropped(cause, w=W, h=HT):
            nonlocal drops
            drops += 1
            host.render(2)
            _shown_is_the_chain_without_history(host, 2, w, h)
            st = host.history_stats()
            assert st["frames_dropped"] == drops and cause in st["last_drop"] and st["frames_carried"] == 0, st
        m = host.get_material(0)
        m.roughness = 0.5
        host.set_material(0, m)
        with pytest.raises(luminary_amd.LuminaryError):
            host.history_image(W, HT)  # dropped at the edit, not at the next output
        dropped("material")
        inst = host.get_instance(2)
        inst.position.x += 0.2
        host.set_instance(inst)
        dropped("instance")
        c = host.get_camera()
        c.use_physical_camera = True
        host.set_camera(c)
        dropped("physical camera")
        c.pos.x += 0.1  # a move of the physical camera is no carry either
        host.set_camera(c)
        dropped("physical camera")
        c.use_physical_camera = False
        host.set_camera(c)
        dropped("physical camera")
        s = host.get_settings()
        s.width, s.height = 48, 32
        host.set_settings(s)
        host.set_output_properties(48, 32)
        dropped("frame size", 48, 32)
    finally:
        host.close()


def test_two_moves_without_an_output_carry_from_the_older_key():
    host = scenes.zoo_scene(W, HT, 3)
    try:
        host.set_denoiser(enabled=True)
        host.set_history(enabled=True)
        host.set_output_properties(W, HT)
        host.render(16)
        before = _frame_state(host)
        _move(host, (0.2, 0.0, 0.0), 0.0)
        host.set_output_properties(W, HT, enabled=False)
        host.render(2)  # nobody looks: no output, the state stays
        host.set_output_properties(W, HT)
        _move(host, (0.1, 0.1, 0.0), 0.03)
        host.render(1)
        after = _frame_state(host)
        st = _params(host)
        carried, cw, stats = lumcore.history_reproject_host(after["key"], before["key"], st, after["normal"], after["depth"], before["shown"], before["weight"], before["normal"], before["depth"])
        assert stats[0] >= P // 2
        _, shown, weight = lumcore.history_blend_host(st, W, HT, 1, after["cur"], carried, cw)
        assert np.array_equal(_bits(after["shown"]), _bits(shown)) and np.array_equal(_bits(after["weight"]), _bits(weight))
        assert host.history_stats()["frames_carried"] == 1 and host.history_stats()["frames_dropped"] == 0
    finally:
        host.close()


# ---- 5. off is off ----
def _everything(host):
    """every output the switch must not touch while it is off, after 8 ids, a move and 2 ids"""
    host.set_denoiser(enabled=True)
    host.set_output_properties(W, HT)
    host.render(8)
    first = host.get_image(host.acquire_output())[0]
    _move(host)
    host.render(2)
    second = host.get_image(host.acquire_output())[0]
    fm, sm = host.accumulators()
    host.render_mattes(4)
    ids, cov = host.matte(luminary_amd.MATTE_LAYER_INSTANCE, 4, W, HT)
    return {"first": first, "second": second, "fm": _bits(fm), "sm": _bits(sm), "denoised": _bits(host.denoised(W, HT)), "ids": ids, "cov": _bits(cov)}


def test_off_is_off_and_on_leaves_the_other_getters_alone():
    never, toggled, on = scenes.zoo_scene(W, HT, 3), scenes.zoo_scene(W, HT, 3), scenes.zoo_scene(W, HT, 3)
    try:
        toggled.set_history(enabled=True, clamp_sigma=1.0)
        toggled.set_history(enabled=False)
        on.set_history(enabled=True)
        a, b, c = _everything(never), _everything(toggled), _everything(on)
        for k in a:
            assert np.array_equal(a[k], b[k]), ("enabled and disabled before rendering: every byte stays", k)
        for k in ("fm", "sm", "denoised", "ids", "cov"):
            assert np.array_equal(a[k], c[k]), ("history on: the accumulators, the denoised image and the mattes are what they were", k)
        assert np.array_equal(a["first"], c["first"]), "before any move nothing is carried: the first output is the plain chain's"
        assert not np.array_equal(a["second"], c["second"]), "after the move the output shows the history"
        assert never.history_stats()["bytes"] == 0 and toggled.history_stats()["bytes"] == 0 and on.history_stats()["frames_carried"] == 1
        # switched off while a frame is held: dropped, and the next output is the plain chain's again
        on.set_history(enabled=False)
        assert "switched off" in on.history_stats()["last_drop"]
        on.render(2)
        never.render(2)
        assert np.array_equal(on.get_image(on.acquire_output())[0], never.get_image(never.acquire_output())[0])
    finally:
        for h in (never, toggled, on):
            h.close()


def test_setting_history_does_not_restart_and_adaptive_sampling_is_skipped(tmp_path):
    host = scenes.zoo_scene(W, HT, 3)
    try:
        host.set_output_properties(W, HT)
        host.render(4)
        host.set_history(enabled=True)
        assert host.is_rendering()[1] == 4, "the setter does not restart the integration"
        host.render(4)
        assert host.history_image(W, HT)[1].max() == F(8)
    finally:
        host.close()
    images = []
    for enabled in (False, True):
        host = scenes.cornell_host(str(tmp_path / ("a%d" % enabled)), 48, 32, 2)
        try:
            s = host.get_settings()
            s.enable_adaptive_sampling = True
            s.adaptive_sampling_update_interval = 2
            host.set_settings(s)
            host.set_history(enabled=enabled)
            host.set_output_properties(48, 32)
            host.render(4)
            images.append(host.get_image(host.acquire_output())[0])
            st = host.history_stats()
            assert st["frames_carried"] == 0 and (st["frames_skipped"] >= 1) == enabled and st["valid"] == 0, st
        finally:
            host.close()
    assert np.array_equal(images[0], images[1]), "adaptive sampling: the image is left alone"
