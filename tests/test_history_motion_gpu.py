"""Image history across rigid instance moves, on the device (csrc/host/history.hip k_history_owner, k_history_motion, k_history_reproject_motion; include/lum_core.h
lumc_set_history_motion; include/luminary_amd.h luminary_ext_set_history_motion). tests/test_history_motion.py holds the twins to the definition.

  kernels   the three kernels equal the twins byte for byte, counters included, on every family, frame and instance count of the CPU test; with no instance moved
            k_history_reproject_motion gives k_history_reproject's bytes.
  host      on zoo_scene(50, 31), both flavours: 32 ids, one non-emissive instance moved by three pixels, 1 id - the shown image is the twins fed with what the public
            getters return. The instance is the one that owns most pixels of the frame among the scene's nine objects, read from the owner plane, and the move is
            three pixels at its mean depth: that there are carried pixels of the mover and rejected ones is asserted, not assumed.
  drops     a moved emitter, a changed instance count, a mesh edit, motion off (today's string); moves without an output; off is off; the effect."""
import ctypes as C

import numpy as np
import pytest

import history_cases as H
import history_motion_cases as M
import luminary_amd
from luminary_amd import core as lumcore
from luminary_amd import scenes
from luminary_amd.core import Core
from test_history_gpu import _bits, _frame_state, _main_core, _move, _params, _planar, _shown_is_the_chain_without_history

pytestmark = pytest.mark.gpu
F, U = np.float32, np.uint32
W, HT = 50, 31
P = W * HT
INSTANCES, OBJECTS, EMITTER = 13, range(1, 10), 11  # zoo_scene: the ground, nine objects, the sheet, two emitters


@pytest.fixture(scope="module")
def device():
    core = Core(0)
    yield core
    core.close()


def _hits_of(owner, width, rng):
    """a closest-hit pass's hit_id records [paths, 4] that give this owner plane: one path per pixel that has one, in a shuffled order, the hit word in x, the pixel in z"""
    owner = np.asarray(owner, U)
    pixels = np.flatnonzero(owner != U(M.EMPTY))
    rng.shuffle(pixels)
    hit = owner[pixels].copy()
    hit[owner[pixels] == U(M.MISS)] = U(0xFFFFFFFF)    # nothing was hit
    hit[owner[pixels] == U(M.PARTICLE)] = U(0x80000007)  # some particle
    hits = np.zeros((len(pixels), 4), U)
    hits[:, 0], hits[:, 1] = hit, rng.integers(0, 1000, len(pixels))
    hits[:, 2] = (pixels % width).astype(U) | ((pixels // width).astype(U) << U(16))
    return hits


@pytest.mark.parametrize("name", M.FAMILIES)
@pytest.mark.parametrize("frame", H.FRAMES)
def test_the_kernels_equal_the_twins(device, frame, name):
    st = lumcore.history_params()
    for count in M.COUNTS:
        c = M.family(name, frame[0], frame[1], count)
        rec, rstats = lumcore.history_motion_records_host(c["old8"], c["new8"])
        want = lumcore.history_reproject_motion_host(c["now"], c["old"], st, M.CAP, c["normal"], c["depth"], c["old_shown"], c["old_weight"], c["old_normal"], c["old_depth"], c["owner"],
                                                     c["old_owner"], rec)
        hits = _hits_of(c["owner"], frame[0], np.random.default_rng(count))
        got = device.history_motion_kernels(c["now"], c["old"], st, M.CAP, c["normal"], c["depth"], c["old_shown"], c["old_weight"], c["old_normal"], c["old_depth"], None, c["old_owner"],
                                            c["old8"], c["new8"], hit_ids=hits)
        assert np.array_equal(got["owner"], np.asarray(c["owner"], U)), (count, "k_history_owner")
        assert got["records"].tobytes() == rec.tobytes() and got["motion_stats"] == rstats, (count, "k_history_motion")
        assert got["stats"] == want[2], count
        assert H.same_bits(got["carried"], want[0]) and H.same_bits(got["carried_weight"], want[1]), (count, "k_history_reproject_motion")
        assert sum(want[2][:3]) == frame[0] * frame[1]


@pytest.mark.parametrize("frame", H.FRAMES)
def test_with_no_instance_moved_the_motion_kernel_gives_the_camera_kernels_bytes(device, frame):
    rng = np.random.default_rng(frame[0])
    Pf = frame[0] * frame[1]
    for name, (old, now) in H.keys(*frame).items():
        pl = H.planes(old, now, seed=frame[0] + 7, random_guides=(name == "rotated"))
        st = lumcore.history_params()
        plain = device.history_kernels(now, old, st, 3, pl["image"], pl["normal"], pl["depth"], pl["old_shown"], pl["old_weight"], pl["old_normal"], pl["old_depth"])
        for count in (0, 65):
            ids = np.concatenate([np.arange(count, dtype=U), np.array([M.MISS, M.OCEAN, M.PARTICLE, M.EMPTY], U)])
            owner, old_owner = rng.choice(ids, Pf), rng.choice(ids, Pf)
            t8 = np.stack([M.words(rng.uniform(-5, 5, 3), rng.uniform(0.5, 2, 3), M.quat(rng.normal(size=3), 1.0)) for _ in range(count)]) if count else np.zeros((0, 8), F)
            got = device.history_motion_kernels(now, old, st, M.CAP, pl["normal"], pl["depth"], pl["old_shown"], pl["old_weight"], pl["old_normal"], pl["old_depth"], owner, old_owner, t8, t8)
            assert got["motion_stats"] == (0, count, 0)
            assert got["stats"] == plain["stats"] + (0, 0), (name, count)
            assert H.same_bits(got["carried"], plain["carried"]) and H.same_bits(got["carried_weight"], plain["carried_weight"]), (name, count)


# ---- the core's refusals ----
def test_the_core_entry_points_refuse_and_name_the_cause():
    from luminary_amd.core import CoreError, FIRST_HIT_GUIDES, FIRST_HIT_OWNER, HistoryMotionParams
    host = scenes.zoo_scene(W, HT, 3)
    core = Core(0)
    try:
        core.upload(host.device_scene())
        core.set_pixels(None)
        core.render(0, 2, samples_per_pass=2)
        core.generate_result(uniform_samples=2)
        for bad, what in ((HistoryMotionParams(2, 8.0), "enabled is 0 or 1"), (HistoryMotionParams(1, 0.0), "positive and finite"), (HistoryMotionParams(1, -1.0), "positive and finite"),
                          (HistoryMotionParams(1, float("nan")), "positive and finite"), (HistoryMotionParams(1, float("inf")), "positive and finite")):
            with pytest.raises(CoreError, match=what):
                core._call("lumc_set_history_motion", C.byref(bad))
        with pytest.raises(CoreError, match="null argument"):
            core._call("lumc_set_history_motion", C.c_void_p(None))
        # the owner bit: with the guides only, and with the motion on only; nothing is allocated by a refusal
        with pytest.raises(CoreError, match="goes with LUMC_FIRST_HIT_GUIDES"):
            core.render_first_hits(4, FIRST_HIT_OWNER, 0)
        with pytest.raises(CoreError, match="needs the history's motion switched on"):
            core.render_first_hits(4, FIRST_HIT_GUIDES | FIRST_HIT_OWNER, 0)
        with pytest.raises(CoreError, match="what is LUMC_FIRST_HIT_GUIDES"):
            core.render_first_hits(4, 8, 0)
        assert core.history_motion_stats().bytes == 0 and not core.has_history_snapshot()
        with pytest.raises(CoreError, match="the state holds no owner plane"):
            core.download_history_owner(state=True, current=False)
        with pytest.raises(CoreError, match="no owner plane for this frame"):
            core.download_history_owner(state=False, current=True)
        snap = np.zeros((INSTANCES, 8), F)
        with pytest.raises(CoreError, match="the state holds no snapshot"):
            core._call("lumc_download_history_transforms", C.c_void_p(snap.ctypes.data), C.c_void_p(None), C.c_void_p(None))
        assert core.download_history_transforms(INSTANCES)[0] is None
        # a state shown with its owner plane; then the carry's two refusals
        core.set_history(lumcore.history_params())
        core.set_history_motion(True, 8.0)
        core.render_first_hits(4, FIRST_HIT_GUIDES | FIRST_HIT_OWNER, 0)
        core.history_blend(2)
        assert core.has_history_snapshot() and core.history_motion_stats().snapshot_instances == INSTANCES
        core.render_guides(4)  # guides without their owner plane: the plane of the earlier render is not this one's
        with pytest.raises(CoreError, match="no owner plane for this frame"):
            core.history_carry()
        inst = host.get_instance(2)
        host.new_instance(inst.mesh_id, (0.0, 3.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        core.upload(host.device_scene())
        core.set_pixels(None)
        core.render_first_hits(4, FIRST_HIT_GUIDES | FIRST_HIT_OWNER, 0)
        with pytest.raises(CoreError, match="the instance count differs from the snapshot's"):
            core.history_carry()
        # switched off: the camera form, which needs neither
        core.set_history_motion(False, 8.0)
        core.history_carry()
        assert core.history_motion_stats().motion_carries == 0 and core.history_stats().carries == 1
        # the kernels' entry point for the tests
        key = lumcore.history_key((0, 0, 0), (0, 0, 0, 1), H.FOV, 4, 4)
        a, b, o, t8 = np.ones((3, 16), F), np.ones(16, F), np.zeros(16, U), np.ones((1, 8), F)
        st = lumcore.history_params()
        ok = dict(now_key=key, old_key=key, params=st, motion_max_history=8.0, normal=a, depth=b, old_shown=a, old_weight=b, old_normal=a, old_depth=b, owner=o, old_owner=o, old8=t8, new8=t8)
        assert core.history_motion_kernels(**ok)["stats"][:3] == (16, 0, 0)
        for cap in (0.0, float("nan"), float("inf")):
            with pytest.raises(CoreError, match="motion_max_history must be positive and finite"):
                core.history_motion_kernels(**dict(ok, motion_max_history=cap))
        with pytest.raises(CoreError, match="max_history must be positive"):
            core.history_motion_kernels(**dict(ok, params=lumcore.history_params(max_history=0.0)))
        with pytest.raises(CoreError, match="null argument"):
            core.history_motion_kernels(**dict(ok, owner=None))
        with pytest.raises(CoreError, match="more paths than pixels"):
            core.history_motion_kernels(**dict(ok, owner=None, hit_ids=np.zeros((17, 4), U)))
    finally:
        core.close()
        host.close()


# ---- end to end ----
def _start(host, ids=32, motion=True):
    host.set_denoiser(enabled=True)
    host.set_history(enabled=True)
    if motion:
        host.set_history_motion(enabled=True)
    host.set_output_properties(W, HT)
    host.render(ids)
    assert host.get_image(host.acquire_output())[1] == ids


def _motion_state(host):
    s = _frame_state(host)
    shown_owner, current = host.history_owner(W, HT)
    assert np.array_equal(shown_owner, current), "the state was shown with the guides as they stand"
    s["owner"] = current.reshape(-1)
    s["t8"] = host.history_transforms(INSTANCES)[1]
    return s


def _nudge(host, state, instance=None, pixels=3.0):
    """`instance` (default: the object that owns most of the frame) moved by `pixels` pixels at its mean depth along x, a fifth of that along y; returns its id"""
    if instance is None:
        owned = [(int((state["owner"] == U(i)).sum()), i) for i in OBJECTS]
        assert max(owned)[0] > 0, "no object of the zoo owns a pixel of this frame"
        instance = max(owned)[1]
    mine = state["owner"] == U(instance)
    depth = float(state["depth"][mine & (state["depth"] > 0)].mean()) if (mine & (state["depth"] > 0)).any() else 10.0
    shift = pixels * 2.0 * float(state["key"].fov) / W * depth
    inst = host.get_instance(instance)
    inst.position.x += shift
    inst.position.y += 0.2 * shift
    assert host.instance_change_carries_history([inst]) == (instance != EMITTER)
    host.set_instance_transforms([inst])
    assert host.is_rendering()[1] == 0, "the move restarts the integration"
    return instance


def _twins(before, after, st, cap, samples=1):
    rec, rstats = lumcore.history_motion_records_host(before["t8"], after["t8"])
    carried, cw, stats = lumcore.history_reproject_motion_host(after["key"], before["key"], st, cap, after["normal"], after["depth"], before["shown"], before["weight"], before["normal"],
                                                               before["depth"], after["owner"], before["owner"], rec)
    _, shown, weight = lumcore.history_blend_host(st, W, HT, samples, after["cur"], carried, cw)
    return rstats, stats, shown, weight, carried, cw


def _end_to_end(host):
    _start(host)
    before = _motion_state(host)
    assert host.history_motion_stats()["valid"] == 1 and host.history_motion_stats()["frames_carried"] == 0
    mover = _nudge(host, before)
    host.render(1)
    assert host.get_image(host.acquire_output())[1] == 1
    after = _motion_state(host)
    assert bytes(before["key"]) == bytes(after["key"]) and not np.array_equal(before["t8"][mover], after["t8"][mover])
    st, cap = _params(host), host.get_history_motion().motion_max_history
    rstats, stats, shown, weight, carried, cw = _twins(before, after, st, cap)
    print("end to end: instance", mover, "records moved, same, void =", rstats, "pixels carried, rejected, off, owner moved, owner moved and carried =", stats, "of", P)
    assert rstats == (1, INSTANCES - 1, 0)
    assert stats[4] > 0 and stats[1] > 0, "mover-owned pixels carried, and some pixels rejected"
    assert np.array_equal(_bits(after["shown"]), _bits(shown)), "the shown image is the twins' on the getters' planes"
    assert np.array_equal(_bits(after["weight"]), _bits(weight))
    assert not np.array_equal(_bits(shown), _bits(after["cur"])), "the history changed the image"
    hs, ms = host.history_stats(), host.history_motion_stats()
    assert (hs["last_carried"], hs["last_rejected"], hs["last_off"]) == stats[:3] and hs["frames_carried"] == 1 and hs["frames_dropped"] == 0
    assert (ms["instances_moved"], ms["instances_same"], ms["instances_void"]) == rstats and (ms["last_moved_pixels"], ms["last_moved_carried"]) == stats[3:]
    assert ms["frames_carried"] == 1 and ms["bytes"] >= 8 * P + 32 * INSTANCES + 128 * INSTANCES
    with _main_core(host) as core:
        _, _, c_dev, cw_dev = core.download_history()
    assert np.array_equal(_bits(c_dev), _bits(carried)) and np.array_equal(_bits(cw_dev), _bits(cw))


def test_end_to_end_the_shown_image_is_the_twins():
    host = scenes.zoo_scene(W, HT, 3)
    try:
        _end_to_end(host)
    finally:
        host.close()


def test_end_to_end_in_the_fast_flavour(monkeypatch):
    monkeypatch.setenv("LUM_FLAVOUR", "fast")
    host = scenes.zoo_scene(W, HT, 3)
    try:
        _end_to_end(host)
    finally:
        host.close()


# ---- drops ----
def test_what_still_drops_names_its_cause():
    host = scenes.zoo_scene(W, HT, 3)
    try:
        _start(host, 8)
        drops = 0

        def dropped(cause):
            nonlocal drops
            drops += 1
            with pytest.raises(luminary_amd.LuminaryError):
                host.history_image(W, HT)  # dropped at the edit
            host.render(2)
            _shown_is_the_chain_without_history(host, 2)
            st = host.history_stats()
            assert st["frames_dropped"] == drops and cause in st["last_drop"] and st["frames_carried"] == 0, st
        _nudge(host, _motion_state(host), instance=EMITTER)
        dropped("a moved instance emits")
        inst = host.get_instance(2)  # luminary_host_set_instance: more than the transforms may have changed
        inst.position.x += 0.2
        host.set_instance(inst)
        dropped("an instance changed")
        m = host.get_material(0)
        m.roughness = 0.5
        host.set_material(0, m)
        dropped("material")
        # under the physical camera nothing is reprojected: an instance move drops as it always did, and the output comes
        c = host.get_camera()
        c.use_physical_camera = True
        host.set_camera(c)
        dropped("physical camera")
        inst = host.get_instance(2)
        inst.position.x += 0.1
        assert not host.instance_change_carries_history([inst])
        host.set_instance_transforms([inst])
        dropped("an instance changed")
        c.use_physical_camera = False
        host.set_camera(c)
        dropped("physical camera")
        # a carry granted for an instance move needs the motion form: switching the motion off while it is due drops
        _nudge(host, _motion_state(host), instance=2)
        host.set_history_motion(enabled=False)
        dropped("motion was switched off")
        _nudge_plain(host, 2)
        dropped("an instance changed")
    finally:
        host.close()


def _nudge_plain(host, instance):
    inst = host.get_instance(instance)
    inst.position.x += 0.1
    host.set_instance_transforms([inst])


def test_a_new_instance_drops_with_the_count():
    host = scenes.zoo_scene(W, HT, 3)
    try:
        _start(host, 8)
        inst = host.get_instance(2)
        host.new_instance(inst.mesh_id, (0.0, 3.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        with pytest.raises(luminary_amd.LuminaryError):
            host.history_image(W, HT)
        host.render(2)
        _shown_is_the_chain_without_history(host, 2)
        st = host.history_stats()
        assert st["frames_carried"] == 0 and st["frames_dropped"] == 1 and "an instance changed" in st["last_drop"], st
    finally:
        host.close()


def test_a_mesh_edit_drops():
    host = scenes.zoo_scene(W, HT, 3)
    try:
        _start(host, 8)
        inst = host.get_instance(2)
        host.set_mesh_positions(inst.mesh_id, host.get_mesh(inst.mesh_id)[0] * F(1.05))
        with pytest.raises(luminary_amd.LuminaryError):
            host.history_image(W, HT)
        host.render(2)
        _shown_is_the_chain_without_history(host, 2)
        assert "mesh" in host.history_stats()["last_drop"] and host.history_stats()["frames_carried"] == 0
    finally:
        host.close()


# ---- moves without an output ----
@pytest.mark.parametrize("second", ("instance", "camera"))
def test_two_moves_without_an_output_carry_from_the_older_snapshot_and_key(second):
    host = scenes.zoo_scene(W, HT, 3)
    try:
        _start(host, 16)
        before = _motion_state(host)
        mover = _nudge(host, before, pixels=2.0)
        host.set_output_properties(W, HT, enabled=False)
        host.render(2)  # nobody looks: no output, the state stays
        host.set_output_properties(W, HT)
        if second == "instance":
            _nudge(host, before, instance=mover, pixels=1.0)
        else:
            _move(host, (0.1, 0.05, 0.0), 0.01)
        host.render(1)
        after = _motion_state(host)
        rstats, stats, shown, weight, _, _ = _twins(before, after, _params(host), host.get_history_motion().motion_max_history)
        assert rstats[0] == 1 and stats[0] >= P // 2
        assert np.array_equal(_bits(after["shown"]), _bits(shown)) and np.array_equal(_bits(after["weight"]), _bits(weight))
        assert host.history_stats()["frames_carried"] == 1 and host.history_stats()["frames_dropped"] == 0
    finally:
        host.close()


# ---- off is off ----
def _everything(host):
    host.set_denoiser(enabled=True)
    host.set_output_properties(W, HT)
    host.render(8)
    first = host.get_image(host.acquire_output())[0]
    _nudge_plain(host, 2)
    host.render(2)
    second = host.get_image(host.acquire_output())[0]
    fm, sm = host.accumulators()
    host.render_mattes(4)
    ids, cov = host.matte(luminary_amd.MATTE_LAYER_INSTANCE, 4, W, HT)
    _, gn, gd = host.first_hit_guides(W, HT)
    out = {"first": first, "second": second, "fm": _bits(fm), "sm": _bits(sm), "denoised": _bits(host.denoised(W, HT)), "ids": ids, "cov": _bits(cov), "gn": _bits(gn), "gd": _bits(gd)}
    if host.get_history().enabled:
        shown, weight = host.history_image(W, HT)
        out["shown"], out["weight"] = _bits(shown), _bits(weight)
    return out


def test_off_is_off():
    never, history, toggled, on = (scenes.zoo_scene(W, HT, 3) for _ in range(4))
    try:
        history.set_history(enabled=True)
        toggled.set_history(enabled=True)
        toggled.set_history_motion(enabled=True, motion_max_history=4.0)
        toggled.set_history_motion(enabled=False)
        on.set_history_motion(enabled=True)  # the motion without the history is nothing
        a, b, c, d = _everything(never), _everything(history), _everything(toggled), _everything(on)
        for k in a:
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], d[k]), ("history on, or motion on without history: an instance move drops, every byte stays", k)
        for k in b:
            assert np.array_equal(b[k], c[k]), ("motion switched on and off before rendering: a host that never heard of it", k)
        assert history.history_motion_stats()["bytes"] == 0 and toggled.history_motion_stats()["bytes"] == 0 and on.history_motion_stats()["bytes"] == 0
        assert "an instance changed" in history.history_stats()["last_drop"] and "an instance changed" in toggled.history_stats()["last_drop"]
    finally:
        for h in (never, history, toggled, on):
            h.close()


# ---- the effect ----
def test_history_brings_the_first_sample_of_a_moved_instance_closer_to_the_converged_image():
    """zoo at 50 x 31: 64 ids, the largest object moved by three pixels, 1 id. Mean squared error against 1024 ids of the moved scene: shown (1 id + history) below the
    plain 1-id image, which is what a drop shows. The ratio is printed and recorded in DESIGN.md section 17, not asserted."""
    host, ref = scenes.zoo_scene(W, HT, 3), scenes.zoo_scene(W, HT, 3)
    try:
        host.set_history(enabled=True)
        host.set_history_motion(enabled=True)
        host.set_output_properties(W, HT)
        host.render(64)
        host.get_image(host.acquire_output())
        before = _motion_state(host)
        mover = _nudge(host, before)
        host.render(1)
        host.get_image(host.acquire_output())
        shown = host.history_image(W, HT)[0].astype(np.float64)
        fm, _ = host.accumulators()
        plain = fm.reshape(3, HT, W).transpose(1, 2, 0).astype(np.float64)
        assert host.history_stats()["frames_carried"] == 1
        ref.set_instance_transforms([host.get_instance(mover)])
        ref.render(1024)
        fm, _ = ref.accumulators()
        truth = fm.reshape(3, HT, W).transpose(1, 2, 0).astype(np.float64) / 1024.0
        mse_shown, mse_plain = float(((shown - truth) ** 2).mean()), float(((plain - truth) ** 2).mean())
        print("effect: mse shown %.6g, plain %.6g, ratio %.4f" % (mse_shown, mse_plain, mse_shown / mse_plain))
        assert mse_shown < mse_plain
    finally:
        host.close()
        ref.close()
