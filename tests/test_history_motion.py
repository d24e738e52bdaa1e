"""Image history across rigid instance moves, on the host side (include/lum_core.h lumc_history_motion_records_host, lumc_history_reproject_motion_host;
include/luminary_amd.h luminary_ext_set_history_motion; csrc/host/history.h "Motion", history.cpp, api.cpp), no GPU.

The record of an instance and the motion form of a pixel are one definition compiled twice; this file holds the host's compilation - the twins - to a numpy
restatement written from the header's text (tests/history_motion_cases.py: binary64 for the record, binary32 for the pixel, one operation at a time in the header's
order), bit for bit - no operation had to be compared within an ulp -; tests/test_history_motion_gpu.py holds the device's compilation to the twins.

The worlds are a wall and the sky with a box instance lying on the wall as a thin plate (history_motion_cases.family), so that depth and normal agree between the
plate and the wall around it and only the owners tell them apart. What a family claims to exercise - carried pixels of the mover, taps refused by their owner,
rejected pixels - is asserted from the restatement alone at 50 x 31 and 64 x 64; at 7 x 5 the plate covers four pixels and a family need not show everything, there
the comparison of the bytes stands alone."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import history_cases as H
import history_motion_cases as M
import luminary_amd
from luminary_amd import core, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U, D = np.float32, np.uint32, np.float64
INVALID_API_ARGUMENT, API_EXCEPTION = 3, 7
# The accuracy of the record (test_a_point_of_the_mover_lands_where_float64_puts_it): the worst distance, in pixels, between where a point of the moved instance
# lands through the record and the old key in binary32 and where a float64 evaluation puts it, over the families at 50 x 31 - measured on the CPU, where this
# arithmetic is the device's - and the bound: four times that, for scenes further from the origin than the families'. Both are in DESIGN.md section 17.
WORST_MEASURED, BOUND = 1.0e-5, 4.0e-5


def _run(case, st=None, cap=M.CAP, records=None):
    st = st or core.history_params()
    rec = core.history_motion_records_host(case["old8"], case["new8"])[0] if records is None else records
    return core.history_reproject_motion_host(case["now"], case["old"], st, cap, case["normal"], case["depth"], case["old_shown"], case["old_weight"], case["old_normal"], case["old_depth"],
                                              case["owner"], case["old_owner"], rec)


def _restate(case, st=None, cap=M.CAP, records=None):
    st = st or core.history_params()
    rec = M.motion_records(case["old8"], case["new8"])[0] if records is None else records
    return M.reproject_motion(case["now"], case["old"], st, cap, case["normal"], case["depth"], case["old_shown"], case["old_weight"], case["old_normal"], case["old_depth"], case["owner"],
                              case["old_owner"], rec)


# ---- the twins equal the restatement ----
@pytest.mark.parametrize("name", M.FAMILIES)
@pytest.mark.parametrize("frame", H.FRAMES)
def test_the_twins_equal_the_restatement(frame, name):
    for count in M.COUNTS:
        case = M.family(name, frame[0], frame[1], count)
        rec, rstats = core.history_motion_records_host(case["old8"], case["new8"])
        want_rec, want_rstats = M.motion_records(case["old8"], case["new8"])
        assert rstats == want_rstats and sum(rstats) == count
        assert rec.tobytes() == want_rec.tobytes(), (count, "the records, all 128 bytes of each")
        got, want = _run(case, records=rec), _restate(case, records=want_rec)
        assert got[2] == want[2], count
        assert H.same_bits(got[0], want[0]) and H.same_bits(got[1], want[1]), count
        assert sum(got[2][:3]) == frame[0] * frame[1] and got[2][4] <= got[2][3]
        if frame[0] >= 50:
            M.check_claims(name, case, want[2], want[3])


def test_the_records_classes():
    base = M.words((1.0, 2.0, -3.0), (1.2, 0.9, 0.6), M.quat((0, 1, 0), 0.3))
    moved = M.words((1.5, 2.0, -3.0), (1.2, 0.9, 0.6), M.quat((0, 1, 0), 0.3))

    def cls(old, new):
        rec, stats = core.history_motion_records_host(old, new)
        want, wstats = M.motion_records(old, new)
        assert rec.tobytes() == want.tobytes() and stats == wstats
        return int(rec["cls"][0]), rec[0]
    c, r = cls(base, base)
    assert c == M.SAME and not np.frombuffer(r.tobytes(), U)[1:].any(), "SAME: every other field is zero"
    c, r = cls(base, moved)
    assert c == M.MOVED and np.array_equal(r["t_new"], moved[:3]) and np.array_equal(r["t_old"], base[:3])
    assert np.allclose(r["L"].reshape(3, 3), np.eye(3), atol=1e-6) and np.allclose(r["NL"].reshape(3, 3), np.eye(3), atol=1e-6), "a translation: both maps are the identity"
    for k in range(6):
        for bad in (np.nan, np.inf, -np.inf) + ((0.0, -0.0) if k >= 3 else ()):
            for side in (0, 1):
                w = moved.copy()
                w[k] = bad
                c, r = cls(w, base) if side == 0 else cls(base, w)
                assert c == M.VOID and not np.frombuffer(r.tobytes(), U)[1:].any(), (k, bad, side)
    tiny = moved.copy()
    tiny[3:6] = 1e-30  # 1 / scale stays finite, the determinant of the world->object matrix overflows binary32's range but not binary64's: no VOID by accident
    assert cls(base, tiny)[0] == M.MOVED
    huge = moved.copy()
    huge[3] = 3e38  # 1 / scale is a denormal: still a matrix with a determinant
    assert cls(base, huge)[0] in (M.MOVED, M.VOID)
    # a quaternion of zeros (words 0x7FFF7FFF 0x7FFF7FFF decode to u = 0, s = 0): the matrix is zero, its determinant too
    zero = moved.copy()
    zero[6:8] = np.array([0x7FFF7FFF, 0x7FFF7FFF], U).view(F)
    assert cls(base, zero)[0] == M.VOID
    # L of a rotation with a non-uniform scale is no rotation, and NL is its inverse transposed
    a, b = M.words((0, 0, 0), (2.0, 0.5, 1.0), M.quat((0, 0, 1), 0.2)), M.words((0, 0, 0), (2.0, 0.5, 1.0), M.quat((0, 0, 1), 0.9))
    c, r = cls(a, b)
    L, NL = r["L"].reshape(3, 3).astype(D), r["NL"].reshape(3, 3).astype(D)
    assert c == M.MOVED and np.abs(L @ L.T - np.eye(3)).max() > 0.1 and np.abs(NL.T @ L - np.eye(3)).max() < 1e-6


# ---- hand cases ----
def _sticker(w=12, h=6, shift=3, cap=M.CAP, weight=1000.0):
    """A wall that fills the frame at depth 5 from a camera without rotation and a sticker of 4 x 4 pixels on it, instance 1, moved by `shift` pixels along +x: depth
    and normal agree everywhere, old and new; only the owners tell the sticker from the wall."""
    key = core.history_key((0, 0, 0), (0, 0, 0, 1), H.FOV, w, h)
    P = w * h
    py, px = np.divmod(np.arange(P), w)
    d = np.stack(H.centre_ray(key, px.astype(F), py.astype(F)))
    normal = np.zeros((3, P), F)
    normal[2] = 1.0
    depth = (F(-5.0) / d[2]).astype(F)
    pixel = 2.0 * H.FOV / w * 5.0
    ident = M.words((0, 0, 0), (1, 1, 1), (0, 0, 0, 1))
    old8 = np.stack([ident, ident])
    new8 = old8.copy()
    new8[1][0] = shift * pixel
    old_owner, owner = np.zeros((h, w), U), np.zeros((h, w), U)
    old_owner[1:5, 3:7] = 1
    owner[1:5, 3 + shift:7 + shift] = 1
    shown = np.where(old_owner.reshape(-1) == 1, F(1.0), F(100.0))
    case = {"now": key, "old": key, "old8": old8, "new8": new8, "normal": normal, "depth": depth, "owner": owner.reshape(-1), "old_normal": normal, "old_depth": depth,
            "old_owner": old_owner.reshape(-1), "old_shown": np.stack([shown] * 3), "old_weight": np.full(P, weight, F)}
    return case, owner, old_owner


def test_disoccluded_background_is_rejected_although_depth_and_normal_agree():
    case, owner, old_owner = _sticker()
    got, want = _run(case), _restate(case)
    assert got[2] == want[2] and H.same_bits(got[0], want[0]) and H.same_bits(got[1], want[1])
    plain = core.history_reproject_host(case["now"], case["old"], core.history_params(), case["normal"], case["depth"], case["old_shown"], case["old_weight"], case["old_normal"], case["old_depth"])
    assert plain[2] == (72, 0, 0), "depth and normal agree everywhere: the camera form carries every pixel, the sticker's old colour into the wall it uncovered"
    carried, cw = got[0][0].reshape(6, 12), got[1].reshape(6, 12)
    # a pixel centre lands on a pixel centre up to rounding, so a neighbouring tap may enter with a weight of a few ulp: exact conditions where every neighbour has the same old owner
    assert (cw[2:4, 4] == 0).all() and (carried[2:4, 4] == 0).all(), "the wall the sticker uncovered, with the old sticker all around: rejected"
    uncovered = (old_owner == 1) & (owner == 0)
    assert uncovered.sum() == 12 and not np.isclose(carried[uncovered & (cw > 0)], 1.0).any(), "nothing of the sticker's colour stays behind"
    assert (cw[uncovered] < 1e-3).all()
    assert got[2][1] >= 2 and want[3]["refused_by_owner"].sum() > 0


def test_the_movers_pixels_take_no_background_tap_and_the_cap_is_the_movers_alone():
    case, owner, old_owner = _sticker()
    got = _run(case)
    carried, cw = got[0][0].reshape(6, 12), got[1].reshape(6, 12)
    mine = owner == 1
    assert got[2][3] == 16 and got[2][4] == 16, "every pixel of the sticker carries"
    assert (carried[mine] == F(1.0)).all(), "only the sticker's own colour, although wall taps with agreeing depth and normal lie inside the footprint of its border pixels"
    assert (cw[mine] <= F(M.CAP)).all() and (cw[mine] > F(M.CAP) * F(0.999)).all(), "W = min(motion_max_history, mean weight) ws"
    wall = (owner == 0) & (old_owner == 0)
    assert np.allclose(carried[wall], 100.0, rtol=1e-6) and (cw[wall] <= F(32.0)).all() and (cw[wall] > F(31.9)).all(), "the wall keeps max_history"
    # a larger cap for the mover than for the rest is taken as given; a small weight is under both caps
    case2, _, _ = _sticker(weight=2.0)
    cw2 = _run(case2, cap=64.0)[1].reshape(6, 12)
    assert np.allclose(cw2[mine], 2.0, rtol=1e-5) and np.allclose(cw2[wall], 2.0, rtol=1e-5)
    cw3 = _run(case, cap=64.0)[1].reshape(6, 12)
    assert (cw3[mine] > F(63.9)).all() and (cw3[wall] <= F(32.0)).all()


def test_void_foreign_and_reserved_owners():
    case, owner, old_owner = _sticker()
    P = 72
    # the owner's record is VOID, or its id is no record's: rejected, nothing read; the wall around takes nothing from where it was
    for variant in ("void", "foreign"):
        c = dict(case)
        if variant == "void":
            c["old8"] = case["old8"].copy()
            c["old8"][1][3] = 0.0
        else:
            c["owner"] = np.where(case["owner"] == 1, U(9), case["owner"]).astype(U)
        got, want = _run(c), _restate(c)
        assert got[2] == want[2] and H.same_bits(got[0], want[0]) and H.same_bits(got[1], want[1])
        mine = (owner == 1).reshape(-1)
        assert not got[1][mine].any() and not got[0][:, mine].any() and got[2][1] >= 16 and got[2][3] == 0, variant
    # reserved ids are SAME: a sky, an ocean, particles and pixels without a path carry among themselves as the camera form does
    for rid in (M.MISS, M.OCEAN, M.PARTICLE, M.EMPTY):
        c = dict(case)
        c["owner"], c["old_owner"] = np.full(P, rid, U), np.full(P, rid, U)
        got = _run(c)
        plain = core.history_reproject_host(c["now"], c["old"], core.history_params(), c["normal"], c["depth"], c["old_shown"], c["old_weight"], c["old_normal"], c["old_depth"])
        assert got[2] == plain[2] + (0, 0) and H.same_bits(got[0], plain[0]) and H.same_bits(got[1], plain[1]), rid
    # SAME owners of different ids share their taps (two still instances side by side), a MOVED neighbour's are refused
    c = dict(case)
    c["old8"], c["new8"] = np.concatenate([case["old8"], case["old8"][:1]]), np.concatenate([case["new8"], case["new8"][:1]])
    c["owner"], c["old_owner"] = np.where(case["owner"] == 0, U(2), case["owner"]).astype(U), case["old_owner"]
    got = _run(c)
    wall = ((owner == 0) & (old_owner == 0)).reshape(-1)
    assert (got[1][wall] > F(31.9)).all(), "instance 2 now, instance 0 then, both SAME: carried"


# ---- every record SAME: the camera form, bit for bit ----
@pytest.mark.parametrize("frame", H.FRAMES)
def test_all_records_same_is_the_camera_form_bit_for_bit(frame):
    rng = np.random.default_rng(frame[1])
    P = frame[0] * frame[1]
    for name, (old, now) in H.keys(*frame).items():
        for random_guides in (False, True):
            pl = H.planes(old, now, seed=frame[0] + 100 * len(name), random_guides=random_guides)
            st = core.history_params()
            plain = core.history_reproject_host(now, old, st, pl["normal"], pl["depth"], pl["old_shown"], pl["old_weight"], pl["old_normal"], pl["old_depth"])
            for count in (0, 1, 65, 300):
                ids = np.concatenate([np.arange(count, dtype=U), np.array([M.MISS, M.OCEAN, M.PARTICLE, M.EMPTY], U)])
                owner, old_owner = rng.choice(ids, P), rng.choice(ids, P)
                t8 = np.stack([M.words(rng.uniform(-5, 5, 3), rng.uniform(0.5, 2, 3), M.quat(rng.normal(size=3), 1.0)) for _ in range(count)]) if count else np.zeros((0, 8), F)
                rec, rstats = core.history_motion_records_host(t8, t8)
                assert rstats == (0, count, 0)
                got = core.history_reproject_motion_host(now, old, st, 0.5, pl["normal"], pl["depth"], pl["old_shown"], pl["old_weight"], pl["old_normal"], pl["old_depth"], owner, old_owner, rec)
                assert got[2] == plain[2] + (0, 0), (name, count)
                assert H.same_bits(got[0], plain[0]) and H.same_bits(got[1], plain[1]), (name, random_guides, count)


# ---- accuracy ----
def _worst_landing_error(width, height):
    worst = 0.0
    rng = np.random.default_rng(11)
    for name in ("t0.3", "t3", "t40", "rotated", "sheared", "rescaled", "both", "leaving"):
        case = M.family(name, width, height, 3)
        mover = case["mover"]
        rec = core.history_motion_records_host(case["old8"], case["new8"])[0][mover]
        assert rec["cls"] == M.MOVED
        Mo, Mn = M.matrix64(case["old8"][mover]), M.matrix64(case["new8"][mover])
        to, tn = case["old8"][mover][:3].astype(D), case["new8"][mover][:3].astype(D)
        old = case["old"]
        q = np.array(list(old.rotation), D)
        step = 2.0 * float(old.fov) / width
        vfov = step * height * 0.5
        for _ in range(200):
            p_obj = rng.uniform(-0.5, 0.5, 3)
            p_obj[rng.integers(0, 3)] = rng.choice([-0.5, 0.5])  # on the box's surface
            X_new, X_old = tn + np.linalg.solve(Mn, p_obj), to + np.linalg.solve(Mo, p_obj)
            # float64: a pinhole at the old key
            v = X_old - np.array(list(old.pos), D)
            u, s = -q[:3], q[3]
            dc = 2.0 * np.dot(u, v) * u + (s * s - np.dot(u, u)) * v + 2.0 * s * np.cross(u, v)
            if not dc[2] < 0:
                continue
            fx64, fy64 = (float(old.fov) - dc[0] / dc[2]) / step - 0.5, (dc[1] / dc[2] + vfov) / step - 0.5
            if not (-1 <= fx64 < width and -1 <= fy64 < height):
                continue
            # binary32: the header's step 1 on the point as the new frame holds it, then the twin's projection
            X = X_new.astype(F)
            dd = tuple(X[i] - rec["t_new"][i] for i in range(3))
            Xo = tuple(rec["t_old"][i] + M.row_apply(rec["L"][3 * i], rec["L"][3 * i + 1], rec["L"][3 * i + 2], dd) for i in range(3))
            got = core.history_project_host(old, np.array([Xo[i] - F(old.pos[i]) for i in range(3)], F))
            assert got is not None
            worst = max(worst, float(np.hypot(float(got[0]) - fx64, float(got[1]) - fy64)))
    return worst


def test_a_point_of_the_mover_lands_where_float64_puts_it():
    worst = _worst_landing_error(50, 31)
    print("worst landing error over the families at 50 x 31: %.3g pixels (recorded %.3g, bound %.3g)" % (worst, WORST_MEASURED, BOUND))
    assert worst <= BOUND, worst


# ---- which instance changes carry, what the setters refuse ----
def test_which_instance_changes_carry():
    host = scenes.zoo_scene(32, 32, 2)
    try:
        plain, emitter = host.get_instance(2), host.get_instance(11)
        plain.position.x += 0.2
        emitter.position.x += 0.2
        assert not host.instance_change_carries_history([plain]), "history and motion are off"
        host.set_history(enabled=True)
        assert not host.instance_change_carries_history([plain]), "motion is off"
        host.set_history_motion(enabled=True)
        assert host.instance_change_carries_history([plain])
        assert not host.instance_change_carries_history([emitter]) and not host.instance_change_carries_history([plain, emitter]), "a moved instance emits"
        assert host.instance_change_carries_history([plain, host.get_instance(11)]), "an emitter that stays where it is moves no light"
        assert not host.instance_change_carries_history([]), "nothing changes"
        host.set_history(enabled=False)
        assert not host.instance_change_carries_history([plain]), "the motion without the history is nothing"
        fn = luminary_amd._lib().luminary_ext_instance_change_carries_history
        fn.restype = C.c_uint64
        out = C.c_bool(True)
        arr = (luminary_amd.Instance * 1)(plain)
        assert fn(None, arr, 1, C.byref(out)) != 0 and fn(host._h, arr, 1, None) != 0 and fn(host._h, None, 1, C.byref(out)) == INVALID_API_ARGUMENT
        bad = host.get_instance(2)
        bad.id = 1000
        assert fn(host._h, (luminary_amd.Instance * 1)(bad), 1, C.byref(out)) == INVALID_API_ARGUMENT and out.value is False
    finally:
        host.close()


def test_the_setter_refuses_and_the_getters_refuse_before_any_output():
    host = scenes.zoo_scene(32, 32, 2)
    try:
        d = host.get_history_motion()
        assert (d.enabled, d.motion_max_history) == (False, 8.0), "off by default"
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(luminary_amd.LuminaryError) as e:
                host.set_history_motion(enabled=True, motion_max_history=bad)
            assert e.value.code == INVALID_API_ARGUMENT
            d = host.get_history_motion()
            assert (d.enabled, d.motion_max_history) == (False, 8.0), ("a refusal changes nothing", bad)
        host.set_history_motion(enabled=True, motion_max_history=2.5)
        d = host.get_history_motion()
        assert (d.enabled, d.motion_max_history) == (True, 2.5)
        lib = luminary_amd._lib()
        for fn in (lib.luminary_ext_set_history_motion, lib.luminary_ext_get_history_motion, lib.luminary_ext_get_history_motion_stats, lib.luminary_ext_get_history_owner,
                   lib.luminary_ext_get_history_transforms):
            fn.restype = C.c_uint64
        assert lib.luminary_ext_set_history_motion(None, C.byref(d)) != 0 and lib.luminary_ext_set_history_motion(host._h, None) != 0
        assert lib.luminary_ext_get_history_motion(host._h, None) != 0 and lib.luminary_ext_get_history_motion_stats(host._h, None) != 0
        for getter in (lambda: host.history_owner(32, 32), lambda: host.history_transforms(13)):
            with pytest.raises(luminary_amd.LuminaryError) as e:
                getter()
            assert e.value.code == API_EXCEPTION, "nothing was shown yet"
        st = host.history_motion_stats()
        assert all(v == 0 for v in st.values()), st
    finally:
        host.close()


def test_the_twins_refuse_null_arrays_bad_frames_and_bad_caps():
    key = core.history_key((0, 0, 0), (0, 0, 0, 1), H.FOV, 4, 4)
    st = core.history_params()
    a, b, o = np.ones((3, 16), F), np.ones(16, F), np.zeros(16, U)
    rec = core.history_motion_records_host(np.ones((1, 8), F), np.ones((1, 8), F))[0]
    args = (key, key, st, 8.0, a, b, a, b, a, b, o, o, rec)
    assert core.history_reproject_motion_host(*args)[2][:3] == (16, 0, 0)
    for cap in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            core.history_reproject_motion_host(*args[:3], cap, *args[4:])
    with pytest.raises(ValueError):
        core.history_reproject_motion_host(core.history_key((0, 0, 0), (0, 0, 0, 1), H.FOV, 0, 0), key, st, 8.0, np.zeros((3, 0), F), np.zeros(0, F), a, b, a, b, np.zeros(0, U), o, rec)
    with pytest.raises(ValueError):
        core.history_reproject_motion_host(*args[:10], np.zeros(15, U), o, rec)
    fn = luminary_amd._lib().lumc_history_reproject_motion_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 3 + [C.c_float] + [C.c_void_p] * 9 + [C.c_uint32] + [C.c_void_p] * 3
    out3, out1 = np.full((3, 16), 42, F), np.full(16, 42, F)
    raw = [C.addressof(key), C.addressof(key), C.addressof(st), 8.0, a.ctypes.data, b.ctypes.data, a.ctypes.data, b.ctypes.data, a.ctypes.data, b.ctypes.data, o.ctypes.data, o.ctypes.data,
           rec.ctypes.data, 1, out3.ctypes.data, out1.ctypes.data, None]
    assert fn(*raw) == 0, "the counters are optional"
    out3[:], out1[:] = 42, 42
    for i in (0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15):
        assert fn(*[None if j == i else v for j, v in enumerate(raw)]) == 1, i
    assert (out3 == 42).all() and (out1 == 42).all(), "a refusal writes nothing"
    raw[12], raw[13] = None, 0
    assert fn(*raw) == 0, "no records: every owner is reserved or VOID"
    rfn = luminary_amd._lib().lumc_history_motion_records_host
    rfn.restype = C.c_int
    rfn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    t8 = np.ones((1, 8), F)
    assert rfn(None, t8.ctypes.data, 1, rec.ctypes.data, None) == 1 and rfn(t8.ctypes.data, None, 1, rec.ctypes.data, None) == 1 and rfn(t8.ctypes.data, t8.ctypes.data, 1, None, None) == 1
    assert rfn(None, None, 0, None, None) == 0


# ---- the twins under the sanitizers, the structs ----
def test_stand_alone_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/support/history_motion_check.cpp: the twins on hostile transforms, planes, owners and keys at frames down to 1 x 1, the hand case, their refusals, as a
    program of its own built with the sanitizers."""
    exe = str(tmp_path / "history_motion_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined,float-cast-overflow", "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "support", "history_motion_check.cpp"), os.path.join(ROOT, "luminary_amd", "csrc", "host", "history.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert ran.returncode == 0 and "history_motion_check: ok" in ran.stdout, ran.stdout


def test_the_structs_have_the_headers_layout():
    names = [("LumHistoryMotionParams", ["enabled", "motion_max_history"], core.HistoryMotionParams),
             ("LumHistoryMotionStats", [n for n, _ in core.HistoryMotionStats._fields_], core.HistoryMotionStats),
             ("LuminaryHistoryMotionSettings", ["enabled", "motion_max_history"], luminary_amd.HistoryMotionSettings),
             ("LuminaryHistoryMotionStats", [n for n, _ in luminary_amd.HistoryMotionStats._fields_], luminary_amd.HistoryMotionStats),
             # what the existing tests pin stays where it was
             ("LumHistoryParams", ["enabled", "max_history", "depth_tolerance", "normal_threshold", "clamp_sigma"], core.HistoryParams),
             ("LumHistoryStats", [n for n, _ in core.HistoryStats._fields_], core.HistoryStats)]
    rec_fields = ["cls", "t_new", "t_old", "L", "NL", "pad"]
    body = "".join('printf("%%zu ", sizeof(%s));' % s + "".join('printf("%%zu ", offsetof(%s, %s));' % (s, f) for f in fields) for s, fields, _ in names)
    body += 'printf("%zu ", sizeof(LumHistoryMotionRecord));' + "".join('printf("%%zu ", offsetof(LumHistoryMotionRecord, %s));' % f for f in rec_fields)
    body += 'printf("%d %d %d %d ", LUMC_FIRST_HIT_GUIDES, LUMC_FIRST_HIT_MATTES, LUMC_FIRST_HIT_OWNER, LUMC_KERNEL_COUNT);'
    src = '#include "luminary_amd.h"\n#include "lum_core.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){%s printf("\\n");return 0;}\n' % body
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "p")]).split()]
    want = []
    for _, fields, typ in names:
        want += [C.sizeof(typ)] + [getattr(typ, f).offset for f in fields]
    dt = core.HISTORY_MOTION_RECORD
    want += [dt.itemsize] + [dt.fields[f][1] for f in rec_fields]
    want += [core.FIRST_HIT_GUIDES, core.FIRST_HIT_MATTES, core.FIRST_HIT_OWNER, len(core.KERNELS)]
    assert got == want
    assert dt.itemsize == 128 and C.sizeof(core.HistoryMotionParams) == 8 and C.sizeof(luminary_amd.HistoryMotionSettings) == 8
