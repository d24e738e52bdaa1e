"""Shutter on the host side (include/lum_core.h lumc_shutter_host; include/luminary_amd.h luminary_ext_shutter_open / _render_shutter; csrc/host/mesh_shutter.h,
mesh_shutter.cpp, update_plan.h, api.cpp), no GPU.

The blended vertex record is one function compiled twice; this file holds the host's compilation - the twin - to a numpy restatement of the definition, float32
one operation at a time with the normal packed in float64, byte for byte, and the blended normal to a float64 blend within a derived bound;
tests/test_mesh_shutter_gpu.py holds the device's compilation to the twin. Then what the twin and the public calls refuse, the plan's new bit, the twin under the
sanitizers as a program of its own, and the layout of the two stats structs.

The fallback branch of the normal (a blend of zero or not finite length takes the nearer key's word) needs two words that unpack to exact opposites; a search over
36 million candidate pairs found none, so the "opposite" records here are the nearest there is - the blend at t = 0.5 is tiny, not zero - and are held to the
restatement like every other record, whichever branch they take."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import luminary_amd
from luminary_amd import core
from luminary_amd.core import shutter_host
from test_mesh_skin import INVALID_API_ARGUMENT, _meshes, _raw, _snapshot, _zoo, pack_normal64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U = np.float32, np.uint32
CORNERS = [3, 189, 192, 195, 255, 258, 3000]
TIMES = [F(0.0), F(2.0 ** -24), F(0.25), F(0.5), F(0.75), F(1.0) - F(2.0 ** -24), F(1.0)]


# ---- keys shared with tests/test_mesh_shutter_gpu.py ----
def pack64(n):
    return pack_normal64(np.asarray(n, F).reshape(-1, 3))


def random_keys(rng, corners):
    """Two keys [corners, 4] uint32: random positions and unit normals; a fifth of the records with -0 coordinates, a fifth with equal normal words, a fifth with
    normals that are all but opposite."""
    keys = []
    n = rng.normal(size=(corners, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    for k in range(2):
        rec = np.zeros((corners, 4), U)
        rec[:, :3] = rng.uniform(-3.0, 3.0, (corners, 3)).astype(F).view(U)
        m = n if k == 0 else rng.normal(size=(corners, 3))
        rec[:, 3] = pack64(m / np.linalg.norm(m, axis=1, keepdims=True))
        keys.append(rec)
    a, b = keys
    c = np.arange(corners)
    a[c % 5 == 1, 0] = F(-0.0).view(U); b[c % 5 == 1, 1] = F(-0.0).view(U); a[c % 5 == 1, 2] = F(-0.0).view(U); b[c % 5 == 1, 2] = F(-0.0).view(U)
    b[c % 5 == 2, 3] = a[c % 5 == 2, 3]
    b[c % 5 == 3, 3] = pack64(-n[c % 5 == 3])
    return a, b


# ---- the definition, restated ----
def unpack_numpy(w):
    """dev_math.h normal_unpack, float32, one operation at a time ([c] uint32 -> [c, 3] float32)."""
    w = np.asarray(w, U)
    scale = F(1.0) / F(65535.0)
    x, y = (w & U(0xFFFF)).astype(F) * scale, (w >> U(16)).astype(F) * scale
    x, y = x * F(2.0) - F(1.0), y * F(2.0) - F(1.0)
    z = (F(1.0) - np.abs(x)) - np.abs(y)
    s = -z
    s = np.where(s < 0, F(0.0), np.where(s > 1, F(1.0), s)).astype(F)
    x, y = x + np.where(x >= 0, -s, s), y + np.where(y >= 0, -s, s)
    len2 = (x * x + y * y) + z * z
    rl = F(1.0) / np.sqrt(len2)
    out = np.stack([x * rl, y * rl, z * rl], axis=1)
    assert out.dtype == F
    return out


def lerp_numpy(a, b, t):
    d = b - a
    s = F(t) * d
    out = a + s
    assert out.dtype == F
    return out


def shutter_numpy(a, b, t):
    """(records [c, 4] uint32, flags)"""
    a, b, t = np.asarray(a, U), np.asarray(b, U), F(t)
    if t == 0:
        return a.copy(), 0
    if t == 1:
        return b.copy(), 0
    out = np.zeros_like(a)
    with np.errstate(all="ignore"):
        p = lerp_numpy(a[:, :3].copy().view(F), b[:, :3].copy().view(F), t)
        out[:, :3] = p.view(U)
        n = lerp_numpy(unpack_numpy(a[:, 3]), unpack_numpy(b[:, 3]), t)
        len2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        good = (len2 > 0) & np.isfinite(len2)
        rl = F(1.0) / np.sqrt(np.where(good, len2, F(1.0)))
        word = pack64(n * rl[:, None])
    word = np.where(good, word, a[:, 3] if t < F(0.5) else b[:, 3])
    out[:, 3] = np.where(a[:, 3] == b[:, 3], a[:, 3], word)
    return out, 0 if np.isfinite(p).all() else 1


@pytest.mark.parametrize("corners", CORNERS)
def test_the_twin_is_the_definition_byte_for_byte(corners):
    a, b = random_keys(np.random.RandomState(corners), corners)
    for t in TIMES:
        got, flags = shutter_host(a, b, t)
        want, want_flags = shutter_numpy(a, b, t)
        assert flags == want_flags == 0
        assert np.array_equal(got, want), "%d corners, t = %r: %d of %d words differ" % (corners, float(t), int((got != want).sum()), got.size)
    same = a[:, 3] == b[:, 3]
    assert same.any() and np.array_equal(shutter_host(a, b, F(0.5))[0][same, 3], a[same, 3]), "equal normal words are kept"


def test_a_difference_that_overflows_sets_the_flag_and_is_written_as_computed():
    big = np.finfo(F).max
    a = np.array([[-big, 1.0, -0.0, 0.0], [1.0, 2.0, 3.0, 0.0]], F).view(U)
    b = np.array([[big, 1.0, -0.0, 0.0], [2.0, 3.0, 4.0, 0.0]], F).view(U)
    a[:, 3], b[:, 3] = pack64([[0, 0, 1], [0, 1, 0]]), pack64([[0, 0, 1], [1, 0, 0]])
    for t in TIMES[1:-1]:
        got, flags = shutter_host(a, b, t)
        want, want_flags = shutter_numpy(a, b, t)
        assert flags == want_flags == 1 and np.array_equal(got, want)
        assert np.isinf(got[0, 0:1].view(F)[0]) and got[0, 2] == 0, "-0 + t * (-0 - -0) is +0 between the keys: only t = 0 and t = 1 keep the key's -0"
    for t, key in ((TIMES[0], a), (TIMES[-1], b)):
        got, flags = shutter_host(a, b, t)
        assert flags == 0 and np.array_equal(got, key)


def test_time_zero_and_time_one_return_the_keys_verbatim():
    rng = np.random.RandomState(7)
    a, b = (rng.randint(0, 2 ** 32, (100000, 4), dtype=np.uint64).astype(U) for _ in range(2))  # any bits: NaN payloads, infinities, -0, denormals
    got0, f0 = shutter_host(a, b, 0.0)
    got1, f1 = shutter_host(a, b, 1.0)
    assert np.array_equal(got0, a) and np.array_equal(got1, b) and f0 == 0 and f1 == 0
    assert np.array_equal(shutter_host(a, b, -0.0)[0], a), "-0 is 0"


def unpack64(w):
    """The decode in float64 ([c] uint32 -> [c, 3] unit vectors)."""
    w = np.asarray(w, np.uint64)
    x, y = (w & 0xFFFF) / 65535.0 * 2.0 - 1.0, (w >> 16) / 65535.0 * 2.0 - 1.0
    z = 1.0 - np.abs(x) - np.abs(y)
    s = np.clip(-z, 0.0, 1.0)
    x, y = x + np.where(x >= 0, -s, s), y + np.where(y >= 0, -s, s)
    n = np.stack([x, y, z], axis=1)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def test_the_blended_normal_against_float64():
    """The word the twin writes, decoded in float64, against the normalised float64 blend of the two unpacked normals (the float32 unpacked values, exact in
    float64). The bound, per record, in radians:
      quantisation  each of the two octahedral coordinates is rounded to a multiple of 2 / 65535: at most 1 / 65535 off each, so the point p on the octahedron
                    |x| + |y| + |z| = 1 is off by at most (1, 1, 2) / 65535, length sqrt(6) / 65535; |p| >= 1 / sqrt(3), and the angle subtended is at most
                    (pi / 2) sin(angle) <= (pi / 2) sqrt(18) / 65535 for the small angles here; sqrt(18) / 65535 * pi / 2 is used.
      binary32      the blend is three operations per component (subtract, multiply, add) on magnitudes <= 2: at most 3 * 2 * 2^-24 off per component, sqrt(3)
                    times that as a vector, seen from the blend's length L: 6 sqrt(3) 2^-24 / L * pi / 2. The normalisation (five operations for len2, a
                    square root, a divide, a multiply per component) scales all components by one factor and rounds each once more: 2^-24 * sqrt(3) * pi / 2.
    Records whose float64 blend is shorter than 1e-3 are left out of the angle (the direction of a vanishing blend means nothing); they are held to the
    restatement above."""
    rng = np.random.RandomState(11)
    a, b = random_keys(rng, 30000)
    eps = 2.0 ** -24
    for t in TIMES[1:-1]:
        got, _ = shutter_host(a, b, t)
        na, nb = unpack_numpy(a[:, 3]).astype(np.float64), unpack_numpy(b[:, 3]).astype(np.float64)
        blend = na + float(t) * (nb - na)
        length = np.linalg.norm(blend, axis=1)
        keep = (length >= 1e-3) & (a[:, 3] != b[:, 3])
        want = blend[keep] / length[keep, None]
        cos = np.clip((unpack64(got[keep, 3]) * want).sum(axis=1), -1.0, 1.0)
        angle = np.arccos(cos)
        bound = 0.5 * np.pi * (np.sqrt(18.0) / 65535.0 + 6.0 * np.sqrt(3.0) * eps / length[keep] + np.sqrt(3.0) * eps)
        print("t = %g: %d records, largest angle %.3e rad, smallest margin %.3e rad" % (float(t), int(keep.sum()), float(angle.max()), float((bound - angle).min())))
        assert keep.sum() >= 18000  # (three fifths of the records at the least: equal words and vanishing blends are left out)
        assert (angle <= bound).all(), "t = %r: %d records beyond the bound, worst %.3e of %.3e" % (
            float(t), int((angle > bound).sum()), float(angle.max()), float(bound[np.argmax(angle)]))


def test_the_twin_refuses_null_records_and_a_time_outside_the_interval():
    fn = luminary_amd._lib().lumc_shutter_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
    a, b, out = np.ones((4, 4), U), np.full((4, 4), 2, U), np.full((4, 4), 9, U)
    flags = C.c_uint32(42)
    for t in (-2.0 ** -24, 1.0 + 2.0 ** -23, float("nan"), float("inf"), -float("inf")):
        assert fn(a.ctypes.data, b.ctypes.data, 4, t, out.ctypes.data, C.addressof(flags)) == 1, t
    assert fn(None, b.ctypes.data, 4, 0.5, out.ctypes.data, C.addressof(flags)) == 1
    assert fn(a.ctypes.data, None, 4, 0.5, out.ctypes.data, C.addressof(flags)) == 1
    assert fn(a.ctypes.data, b.ctypes.data, 4, 0.5, None, C.addressof(flags)) == 1
    assert (out == 9).all() and flags.value == 42, "a refusal writes nothing"
    assert fn(a.ctypes.data, b.ctypes.data, 4, 0.5, out.ctypes.data, None) == 0, "the flags are optional"
    with pytest.raises(ValueError):
        shutter_host(a, b, 1.5)


# ---- the public calls: every refusal that needs no device ----
def _render_shutter(host, slices, samples, per_pass=2):
    return _raw("luminary_ext_render_shutter", host, C.c_uint32(slices), C.c_uint32(samples), C.c_uint32(per_pass))


def test_refusals_of_the_arguments_leave_the_host_as_it_was():
    host = _zoo()
    try:
        before = _snapshot(host)
        assert _render_shutter(host, 4, 2) == INVALID_API_ARGUMENT, "no open key"
        host.shutter_open()
        for slices, samples in ((0, 2), (1025, 2), (4, 0)):
            assert _render_shutter(host, slices, samples) == INVALID_API_ARGUMENT, (slices, samples)
        s = host.get_settings()
        s.enable_adaptive_sampling = True
        adaptive = _zoo()
        try:
            adaptive.set_settings(s)
            adaptive.shutter_open()
            assert _render_shutter(adaptive, 4, 2) == INVALID_API_ARGUMENT, "adaptive sampling"
        finally:
            adaptive.close()
        host.shutter_cancel()
        assert _render_shutter(host, 4, 2) == INVALID_API_ARGUMENT, "cancelled: no open key"
        after = _snapshot(host)
        assert before[0] == after[0] and before[3] == after[3]
        for k in before[1]:
            assert np.array_equal(before[1][k], after[1][k]), k
        st = host.shutter_stats()
        assert (st["renders"], st["slices"]) == (0, 0)
    finally:
        host.close()


def test_an_edit_the_shutter_cannot_blend_cancels_it():
    host = _zoo()
    try:
        emits, plain = _meshes(host)
        # a material edit between open and render
        host.shutter_open()
        m = host.get_material(0)
        m.roughness = 0.5 * m.roughness + 0.1
        host.set_material(0, m)
        edited = _snapshot(host)
        assert _render_shutter(host, 4, 2) == INVALID_API_ARGUMENT, "a material edit"
        assert _render_shutter(host, 4, 2) == INVALID_API_ARGUMENT, "... and the shutter is cancelled"
        after = _snapshot(host)
        assert edited[0] == after[0] and all(np.array_equal(edited[1][k], after[1][k]) for k in edited[1])
        # a moved emitter with the refit switch off: the light tree has to be built again
        host.shutter_open()
        p = host.get_mesh(emits)[0].copy()
        p[:, 1::3] += F(0.125)
        host.set_mesh_positions(emits, p)
        assert _render_shutter(host, 4, 2) == INVALID_API_ARGUMENT, "a moved emitter without luminary_ext_set_light_refit"
        # another camera field
        host.shutter_open()
        c = host.get_camera()
        c.thin_lens.fov = c.thin_lens.fov * 0.5
        host.set_camera(c)
        assert _render_shutter(host, 4, 2) == INVALID_API_ARGUMENT, "a camera field other than pos and rotation"
        assert host.shutter_stats()["renders"] == 0
    finally:
        host.close()


# ---- the plan's new bit, the twin under the sanitizers, the structs ----
def _build_and_run(tmp_path, name, sources, flags=()):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", *flags, "-ffp-contract=off", *sources, "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_the_plans_shutter_bit_for_every_input(tmp_path):
    support = os.path.join(ROOT, "tests", "support")
    ran = _build_and_run(tmp_path, "shutter_plan_check", [os.path.join(support, "shutter_plan_check.cpp")])
    assert ran.returncode == 0 and "262144 cases, 0 disagreements" in ran.stdout, ran.stdout
    old = _build_and_run(tmp_path, "update_plan_check", [os.path.join(support, "update_plan_check.cpp")])  # the old check program, unchanged
    assert old.returncode == 0, old.stdout
    assert core.DIRTY_MESH_SHUTTER == 2048 and not (core.DIRTY_ALL & core.DIRTY_MESH_SHUTTER)


def test_stand_alone_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/support/mesh_shutter_check.cpp: the twin over the corner counts and times, in place, its refusals, as a program of its own built with the sanitizers."""
    host = os.path.join(ROOT, "luminary_amd", "csrc", "host")
    ran = _build_and_run(tmp_path, "mesh_shutter_check", [os.path.join(ROOT, "tests", "support", "mesh_shutter_check.cpp"), os.path.join(host, "mesh_shutter.cpp")],
                         ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"])  # (linked statically: nothing is preloaded)
    assert ran.returncode == 0 and "mesh_shutter_check: ok" in ran.stdout, ran.stdout


def test_the_stats_structs_have_the_headers_layout():
    src = '#include "luminary_amd.h"\n#include "lum_core.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(LumShutterStats), ' \
          'sizeof(LuminaryShutterStats), offsetof(LumShutterStats, last_bytes_uploaded), offsetof(LumShutterStats, seconds), offsetof(LuminaryShutterStats, last_moved_meshes), ' \
          'offsetof(LuminaryShutterStats, last_slices), offsetof(LuminaryShutterStats, seconds_update), offsetof(LuminaryShutterStats, seconds_render));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "p")]).split()]
    a, b = core.ShutterStats, luminary_amd.ShutterStats
    assert got == [C.sizeof(a), C.sizeof(b), a.last_bytes_uploaded.offset, a.seconds.offset, b.last_moved_meshes.offset, b.last_slices.offset, b.seconds_update.offset,
                   b.seconds_render.offset] == [32, 48, 16, 24, 16, 28, 32, 40]
    assert [name for name, _ in a._fields_] == ["slices", "last_meshes", "last_launches", "last_bytes_uploaded", "seconds"]
    assert [name for name, _ in b._fields_] == ["renders", "slices", "last_moved_meshes", "last_moved_instances", "last_camera_moved", "last_slices", "seconds_update", "seconds_render"]
