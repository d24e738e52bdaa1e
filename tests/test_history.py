"""Image history on the host side (include/lum_core.h lumc_history_reproject_host, lumc_history_blend_host; include/luminary_amd.h luminary_ext_set_history;
csrc/host/history.h, history.cpp, api.cpp), no GPU.

Reprojection and blend are one definition compiled twice; this file holds the host's compilation - the twins - to a numpy float32 restatement written from the
header's text (tests/history_cases.py: every operation on float32 arrays, one at a time, in the header's order), bit for bit - no operation had to be compared
within an ulp -; tests/test_history_gpu.py holds the device's compilation to the twins. Then the hand cases, the projection against a float64 pinhole ray, which
camera changes carry, what the setters refuse, the twins under the sanitizers as a program of its own, and the layout of the structs."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import history_cases as H
import luminary_amd
from luminary_amd import core, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U = np.float32, np.uint32
INVALID_API_ARGUMENT, API_EXCEPTION = 3, 7
KEYS = ("identical", "translated", "rotated", "fov", "turned", "half_off")


def run_twins(old, now, st, pl, samples=3):
    c, w, stats = core.history_reproject_host(now, old, st, pl["normal"], pl["depth"], pl["old_shown"], pl["old_weight"], pl["old_normal"], pl["old_depth"])
    image, shown, weight = core.history_blend_host(st, now.width, now.height, samples, pl["image"], c, w)
    return {"carried": c, "carried_weight": w, "stats": stats, "image": image, "shown": shown, "weight": weight}


def run_restatement(old, now, st, pl, samples=3):
    c, w, stats = H.reproject(now, old, st, pl["normal"], pl["depth"], pl["old_shown"], pl["old_weight"], pl["old_normal"], pl["old_depth"])
    image, shown, weight = H.blend(st, now.width, now.height, samples, pl["image"], c, w)
    return {"carried": c, "carried_weight": w, "stats": stats, "image": image, "shown": shown, "weight": weight}


# ---- the twins equal the restatement ----
@pytest.mark.parametrize("name", KEYS)
@pytest.mark.parametrize("frame", H.FRAMES)
def test_the_twins_equal_the_restatement(frame, name):
    old, now = H.keys(*frame)[name]
    for random_guides in (False, True):
        for clamp in (0.0, 1.5):
            st = core.history_params(clamp_sigma=clamp)
            pl = H.planes(old, now, seed=frame[0] + 100 * KEYS.index(name), random_guides=random_guides)
            got, want = run_twins(old, now, st, pl), run_restatement(old, now, st, pl)
            assert got["stats"] == want["stats"], (random_guides, clamp)
            for k in ("carried", "carried_weight", "image", "shown", "weight"):
                assert H.same_bits(got[k], want[k]), (k, random_guides, clamp)
            assert sum(got["stats"]) == frame[0] * frame[1]


def test_the_keys_do_what_their_names_say():
    """on the wall world at 50 x 31, tame planes: the conditions are on the twin's counters, so that the comparison above cannot pass empty"""
    P = 50 * 31
    stats = {}
    for name, (old, now) in H.keys(50, 31).items():
        pl = H.planes(old, now, 1, hostile=False)
        stats[name] = run_twins(old, now, core.history_params(), pl)["stats"]
    assert stats["identical"] == (P, 0, 0), "every pixel finds itself"
    assert stats["turned"] == (0, 0, P), "everything lies behind the old camera"
    assert stats["translated"][0] > P // 2 and stats["translated"][2] > 0
    assert stats["rotated"][0] > P // 2 and stats["rotated"][2] > 0
    old, now = H.keys(50, 31)["rotated"]
    pl = H.planes(old, now, 1, hostile=False)
    got = run_twins(old, now, core.history_params(), pl)
    sky = pl["depth"] < 0
    assert sky.any() and (got["carried_weight"][sky] > 0).sum() > sky.sum() // 2, "under a rotation alone the sky carries"
    assert stats["fov"][0] == P, "a narrower frame lies inside the old one"
    assert P // 3 < stats["half_off"][2] + stats["half_off"][1] and stats["half_off"][0] > P // 4 and stats["half_off"][2] > 0


# ---- hand cases ----
def flat_state(w, h, value=1.0, weight=8.0, depth=5.0):
    Q = w * h
    normal = np.zeros((3, Q), F)
    normal[2] = 1.0
    return {"old_shown": np.full((3, Q), value, F), "old_weight": np.full(Q, weight, F), "old_normal": normal, "old_depth": np.full(Q, depth, F)}


def test_taps_on_every_border_and_corner():
    """The sky of a rotated camera: a pixel whose direction lands between the old frame's last column (row) and the one beyond it has one (two) taps; it carries
    their values with ws < 1, and the weight shrinks by ws."""
    w, h = 9, 7
    base = core.history_key((0, 0, 0), (0, 0, 0, 1), H.FOV, w, h)
    state = flat_state(w, h, depth=-1.0)
    state["old_shown"] = np.arange(3 * w * h, dtype=F).reshape(3, w * h) + F(1)
    state["old_normal"][:] = 0
    normal, depth = np.zeros((3, w * h), F), np.full(w * h, -1.0, F)
    seen = set()
    for yaw, pitch in ((0.08, 0.0), (-0.08, 0.0), (0.0, 0.07), (0.0, -0.07), (0.08, 0.07), (-0.08, 0.07), (0.08, -0.07), (-0.08, -0.07)):
        rot = H.quat_mul(H.quat_y(yaw), (float(np.sin(pitch / 2)), 0.0, 0.0, float(np.cos(pitch / 2))))
        now = core.history_key((0, 0, 0), rot, H.FOV, w, h)
        c, cw, stats = core.history_reproject_host(now, base, core.history_params(), normal, depth, **state)
        rc, rw, rstats = H.reproject(now, base, core.history_params(), normal, depth, **state)
        assert H.same_bits(c, rc) and H.same_bits(cw, rw) and stats == rstats
        for p in range(w * h):
            v, fx, fy = H.project(base, H.centre_ray(now, np.array([p % w], F), np.array([p // w], F)))
            if not v[0]:
                continue
            x0, y0 = int(np.floor(fx[0])), int(np.floor(fy[0]))
            inside = [(0 <= x0 + dx < w) and (0 <= y0 + dy < h) for dy in (0, 1) for dx in (0, 1)]
            if 0 < sum(inside) < 4 and cw[p] > 0:
                seen.add(((x0 < 0) - (x0 + 1 >= w), (y0 < 0) - (y0 + 1 >= h)))
                assert cw[p] < F(8.0), "part of the footprint is missing: the weight shrinks with ws"
    assert seen == {(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)}, seen


def test_no_valid_tap_carries_nothing_and_the_cap_holds():
    w, h = 8, 6
    key = core.history_key((0, -0.7, -2.0), (0, 0, 0, 1), H.FOV, w, h)  # four units in front of the wall: it fills the frame
    normal, depth = H.guides_of(key)
    assert (depth > 0).all()
    state = {"old_shown": np.full((3, w * h), 2.0, F), "old_weight": np.full(w * h, 1000.0, F), "old_normal": normal.copy(), "old_depth": depth.copy()}
    c, cw, stats = core.history_reproject_host(key, key, core.history_params(max_history=32.0), normal, depth, **state)
    assert stats == (w * h, 0, 0) and np.all(cw <= F(32.0)) and np.all(cw > F(31.9)), "W = min(max_history, mean weight) ws"
    assert np.allclose(c, 2.0, rtol=1e-6)
    # zero weights everywhere: ws == 0, C = 0 and W = 0 with +0 bits, counted as rejected
    state["old_weight"][:] = 0.0
    c, cw, stats = core.history_reproject_host(key, key, core.history_params(), normal, depth, **state)
    assert stats == (0, w * h, 0) and not c.view(U).any() and not cw.view(U).any()
    # a depth step and a turned normal are refused; the tolerances are inclusive of equality
    state["old_weight"][:] = 4.0
    state["old_depth"] = (depth * F(1.5)).astype(F)
    assert core.history_reproject_host(key, key, core.history_params(), normal, depth, **state)[2] == (0, w * h, 0)
    state["old_depth"] = depth.copy()
    state["old_normal"] = -normal
    assert core.history_reproject_host(key, key, core.history_params(), normal, depth, **state)[2] == (0, w * h, 0)
    assert core.history_reproject_host(key, key, core.history_params(normal_threshold=-1.0), normal, depth, **state)[2] == (w * h, 0, 0)


def test_blend_hand_cases():
    w, h = 5, 4
    P = w * h
    st = core.history_params(clamp_sigma=2.0)
    cur = np.full((3, P), 0.5, F)
    carried, cw = np.full((3, P), 3.0, F), np.full(P, 6.0, F)
    # the clamp on a constant neighbourhood: sigma = 0, the carried colour is clamped onto cur itself, so the blend returns cur's value
    image, shown, weight = core.history_blend_host(st, w, h, 2, cur, carried, cw)
    assert np.all(shown == F(0.5)) and np.all(weight == F(8.0)) and H.same_bits(image, shown)
    # without the clamp: (6 * 3 + 2 * 0.5) / 8
    image, shown, weight = core.history_blend_host(core.history_params(), w, h, 2, cur, carried, cw)
    assert np.all(shown == F(19.0) / F(8.0))
    # W == 0 keeps cur's bits (a negative zero included) and weighs N
    cur2 = cur.copy()
    cur2[1, 3] = -0.0
    cw2 = cw.copy()
    cw2[3] = 0.0
    image, shown, weight = core.history_blend_host(core.history_params(), w, h, 2, cur2, carried, cw2)
    assert image[:, 3].view(U).tolist() == cur2[:, 3].view(U).tolist() and weight[3] == F(2.0)
    # a non-finite cur pixel keeps its bits and gets state weight 0; its finite neighbours are blended as if nothing were
    for bad in (np.nan, np.inf, -np.inf):
        cur3 = cur.copy()
        cur3[2, 7] = bad
        image, shown, weight = core.history_blend_host(core.history_params(), w, h, 2, cur3, carried, cw)
        assert image[:, 7].view(U).tolist() == cur3[:, 7].view(U).tolist() and weight[7] == 0 and weight[6] == F(8.0) and shown[0, 6] == F(19.0) / F(8.0)
    # nothing carried at all: the image keeps every bit, the weights are N
    image, shown, weight = core.history_blend_host(st, w, h, 5, cur3, None, None)
    assert H.same_bits(image, cur3) and weight[7] == 0 and weight[0] == F(5.0)
    # edge pixels use the taps that exist: the restatement counts 4, 6 and 9 of them
    rng = np.random.default_rng(3)
    cur4 = rng.random((3, P)).astype(F)
    got, want = core.history_blend_host(st, w, h, 1, cur4, carried, cw), H.blend(st, w, h, 1, cur4, carried, cw)
    assert all(H.same_bits(a, b) for a, b in zip(got, want))


# ---- the projection inverts the pinhole ray ----
def test_the_projection_returns_the_pixel_centre_of_the_pinhole_ray():
    """project(pos + t dir(pixel)) against a float64 restatement of camera_ray's thin-lens ray with aperture 0 and jitter (1/2, 1/2): within 2^-10 pixel at 50 x 31
    (about ten binary32 operations on coordinates below 64 stay under 2^-14)."""
    w, h = 50, 31
    old, now = H.keys(w, h)["identical"]
    q = np.array(list(now.rotation), np.float64)
    pos = np.array(list(now.pos), np.float64)

    def qapply(q, v):
        u, s = q[:3], q[3]
        return 2.0 * np.dot(u, v) * u + (s * s - np.dot(u, u)) * v + 2.0 * s * np.cross(u, v)
    step = 2.0 * (float(now.fov) / w)
    vfov = step * h * 0.5
    worst = 0.0
    for py in range(h):
        for px in range(w):
            sensor = np.array([float(now.fov) - step * (px + 0.5), -vfov + step * (py + 0.5), 1.0])
            d = qapply(q, -sensor / np.linalg.norm(sensor))
            mine = core.history_centre_ray_host(now, px, py)
            assert np.abs(mine - d).max() < 2.0 ** -20, "the centre ray is camera_ray's"
            for t in (0.3, 7.0, 55.0):
                X = pos + t * d
                got = core.history_project_host(now, (X - pos).astype(F))
                assert got is not None
                worst = max(worst, abs(float(got[0]) - px), abs(float(got[1]) - py))
    assert worst < 2.0 ** -10, worst
    assert core.history_project_host(now, -core.history_centre_ray_host(now, 3, 3)) is None, "a point behind the camera has no projection"


# ---- which camera changes carry ----
def test_only_a_move_of_the_thin_lens_camera_carries():
    lib = luminary_amd._lib()
    carries, restarts = lib.luminary_ext_camera_change_carries_history, lib.luminary_ext_change_restarts_integration
    carries.restype = restarts.restype = C.c_uint64
    host = luminary_amd.Host()
    try:
        old = host.get_camera()

        def ask(**fields):
            new = host.get_camera()
            for k, v in fields.items():
                target, names = new, k.split("__")
                for n in names[:-1]:
                    target = getattr(target, n)
                setattr(target, names[-1], v)
            a, b = C.c_bool(), C.c_bool()
            assert carries(C.byref(new), C.byref(old), C.byref(a)) == 0 and restarts(1, C.byref(new), C.byref(old), C.byref(b)) == 0
            return a.value, b.value
        assert ask() == (False, False), "no change restarts nothing and carries nothing"
        for fields in ({"pos__x": 1.5}, {"pos__z": -2.0}, {"rotation__y": 0.3}, {"thin_lens__fov": 0.7}, {"thin_lens__aperture_size": 0.01}, {"object_distance": 3.0},
                       {"pos__y": 0.1, "rotation__x": 0.2, "thin_lens__fov": 0.4}):
            assert ask(**fields) == (True, True), fields
        for fields in ({"exposure": 1.0}, {"bloom_blend": 0.2}, {"tonemap": 1}):
            assert ask(**fields) == (False, False), ("an output-only change", fields)
        for fields in ({"use_physical_camera": True}, {"camera_scale": 2.0}, {"russian_roulette_threshold": 0.5}, {"aperture_shape": 1},
                       {"pos__x": 1.5, "camera_scale": 2.0}, {"pos__x": 1.5, "use_physical_camera": True}):
            assert ask(**fields) == (False, True), ("restarts without carrying", fields)
        # a camera that is physical before and after: a move restarts and drops
        phys_old, phys_new = host.get_camera(), host.get_camera()
        phys_old.use_physical_camera = phys_new.use_physical_camera = True
        phys_new.pos.x = 4.0
        a = C.c_bool(True)
        assert carries(C.byref(phys_new), C.byref(phys_old), C.byref(a)) == 0 and a.value is False
        assert carries(None, C.byref(old), C.byref(a)) != 0 and carries(C.byref(old), C.byref(old), None) != 0
    finally:
        host.close()


# ---- refusals ----
def test_the_setter_refuses_and_the_getters_refuse_before_any_output():
    host = scenes.zoo_scene(32, 32, 2)
    try:
        d = host.get_history()
        assert (d.enabled, d.max_history, d.depth_tolerance, d.normal_threshold, d.clamp_sigma) == (False, 32.0, F(0.02), F(0.9), 0.0), "off by default"
        bad = [{"max_history": 0.0}, {"max_history": -1.0}, {"max_history": float("nan")}, {"max_history": float("inf")}, {"depth_tolerance": -0.1}, {"depth_tolerance": float("nan")},
               {"depth_tolerance": float("inf")}, {"normal_threshold": 1.5}, {"normal_threshold": -1.5}, {"normal_threshold": float("nan")}, {"clamp_sigma": -1.0},
               {"clamp_sigma": float("nan")}, {"clamp_sigma": float("inf")}]
        for fields in bad:
            with pytest.raises(luminary_amd.LuminaryError) as e:
                host.set_history(enabled=True, **fields)
            assert e.value.code == INVALID_API_ARGUMENT, fields
            d = host.get_history()
            assert (d.enabled, d.max_history, d.clamp_sigma) == (False, 32.0, 0.0), ("a refusal changes nothing", fields)
        host.set_history(enabled=True, max_history=16.0, depth_tolerance=0.0, normal_threshold=-1.0, clamp_sigma=2.5)
        d = host.get_history()
        assert (d.enabled, d.max_history, d.depth_tolerance, d.normal_threshold, d.clamp_sigma) == (True, 16.0, 0.0, -1.0, 2.5), "the limits are taken"
        lib = luminary_amd._lib()
        for fn in (lib.luminary_ext_set_history, lib.luminary_ext_get_history, lib.luminary_ext_get_history_image, lib.luminary_ext_get_history_stats):
            fn.restype = C.c_uint64
        assert lib.luminary_ext_set_history(None, C.byref(d)) != 0 and lib.luminary_ext_set_history(host._h, None) != 0 and lib.luminary_ext_get_history(host._h, None) != 0
        assert lib.luminary_ext_get_history_stats(host._h, None) != 0
        with pytest.raises(luminary_amd.LuminaryError) as e:
            host.history_image(32, 32)
        assert e.value.code == API_EXCEPTION, "nothing was shown yet"
        st = host.history_stats()
        assert st == {"frames_carried": 0, "frames_dropped": 0, "frames_skipped": 0, "last_carried": 0, "last_rejected": 0, "last_off": 0, "valid": 0, "bytes": 0, "seconds": 0.0,
                      "last_drop": ""}
    finally:
        host.close()


def test_the_twins_refuse_null_arrays_and_bad_frames():
    key = core.history_key((0, 0, 0), (0, 0, 0, 1), H.FOV, 4, 4)
    st = core.history_params()
    a, b = np.ones((3, 16), F), np.ones(16, F)
    with pytest.raises(ValueError):
        core.history_reproject_host(core.history_key((0, 0, 0), (0, 0, 0, 1), H.FOV, 0, 0), key, st, np.zeros((3, 0), F), np.zeros(0, F), a, b, a, b)
    with pytest.raises(ValueError):
        core.history_reproject_host(key, key, st, a, b, a, b, a, np.ones(15, F))
    with pytest.raises(ValueError):
        core.history_blend_host(st, 4, 4, 1, a, a, None)
    with pytest.raises(ValueError):
        core.history_blend_host(st, 0, 4, 1, np.zeros((3, 0), F))
    fn = luminary_amd._lib().lumc_history_reproject_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 12
    out3, out1 = np.full((3, 16), 42, F), np.full(16, 42, F)
    args = [C.addressof(key), C.addressof(key), C.addressof(st), a.ctypes.data, b.ctypes.data, a.ctypes.data, b.ctypes.data, a.ctypes.data, b.ctypes.data, out3.ctypes.data, out1.ctypes.data, None]
    assert fn(*args) == 0, "the counters are optional"
    out3[:], out1[:] = 42, 42
    for i in range(11):
        assert fn(*[None if j == i else v for j, v in enumerate(args)]) == 1, i
    assert (out3 == 42).all() and (out1 == 42).all(), "a refusal writes nothing"


# ---- the twins under the sanitizers, the structs ----
def test_stand_alone_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/support/history_check.cpp: the twins on hostile planes and keys at frames down to 1 x 1, their refusals, as a program of its own built with the sanitizers."""
    exe = str(tmp_path / "history_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined,float-cast-overflow", "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "support", "history_check.cpp"), os.path.join(ROOT, "luminary_amd", "csrc", "host", "history.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert ran.returncode == 0 and "history_check: ok" in ran.stdout, ran.stdout


def test_the_structs_have_the_headers_layout():
    names = [("LumHistoryParams", ["enabled", "max_history", "depth_tolerance", "normal_threshold", "clamp_sigma"], core.HistoryParams),
             ("LumHistoryKey", ["pos", "rotation", "fov", "width", "height"], core.HistoryKey),
             ("LumHistoryStats", [n for n, _ in core.HistoryStats._fields_], core.HistoryStats),
             ("LuminaryHistorySettings", [n for n, _ in luminary_amd.HistorySettings._fields_], luminary_amd.HistorySettings),
             ("LuminaryHistoryStats", [n for n, _ in luminary_amd.HistoryStats._fields_], luminary_amd.HistoryStats)]
    body = "".join('printf("%%zu ", sizeof(%s));' % s + "".join('printf("%%zu ", offsetof(%s, %s));' % (s, f) for f in fields) for s, fields, _ in names)
    src = '#include "luminary_amd.h"\n#include "lum_core.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){%s printf("%%d\\n", LUMC_KERNEL_COUNT);return 0;}\n' % body
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "p")]).split()]
    want = []
    for _, fields, typ in names:
        want += [C.sizeof(typ)] + [getattr(typ, f).offset for f in fields]
    assert got[:-1] == want
    assert got[-1] == len(core.KERNELS), "the history's launches are stamped by the history itself: the context's categories are as they were"
    assert C.sizeof(core.HistoryParams) == 20 and C.sizeof(core.HistoryKey) == 40 and C.sizeof(luminary_amd.HistorySettings) == 20
