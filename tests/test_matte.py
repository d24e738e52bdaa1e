"""ID mattes on the host side (include/lum_core.h lumc_matte_host, lumc_matte_mask_host_twin; include/luminary_amd.h luminary_ext_get_matte; csrc/host/matte.h,
matte.cpp, api.cpp), no GPU.

A pixel's table, its ranks and its mask are one definition compiled twice; this file holds the host's compilation - the twin - to a plain Python restatement of
the definition written from its text (slots in order of first appearance, a ninth id dropped; ranks by descending count, then ascending id, here by a sort where
the definition counts comparisons), byte for byte; tests/test_matte_gpu.py holds the device's compilation to the twin. Then the hand cases, what the twins and the
public getters refuse, the twin under the sanitizers as a program of its own, the hit words matte.h restates, and the layout of the structs."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import luminary_amd
from luminary_amd import core, scenes
from luminary_amd.core import MATTE_ID_EMPTY as EMPTY, MATTE_ID_MISS, MATTE_ID_OCEAN, MATTE_ID_PARTICLE, matte_host, matte_mask_host_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U = np.float32, np.uint32
INVALID_API_ARGUMENT, API_EXCEPTION = 3, 7
SLOTS = 8


# ---- the definition, restated ----
def matte_python(ids, ranks):
    """ids [S, P]; returns the dict matte_host returns. Pixel by pixel, sample by sample."""
    ids = np.asarray(ids, U)
    S, P = ids.shape
    out = {"slots_id": np.full((SLOTS, P), EMPTY, U), "slots_count": np.zeros((SLOTS, P), U), "ids": np.full((ranks, P), EMPTY, U),
           "coverage": np.zeros((ranks, P), F), "dropped": np.zeros(P, U), "rays": np.zeros(P, U)}
    for p in range(P):
        slots, dropped, rays = [], 0, 0  # [id, count] in order of first appearance
        for v in ids[:, p].tolist():
            if v == EMPTY:
                continue
            rays += 1
            for s in slots:
                if s[0] == v:
                    s[1] += 1
                    break
            else:
                if len(slots) < SLOTS:
                    slots.append([v, 1])
                else:
                    dropped += 1
        for k, (v, c) in enumerate(slots):
            out["slots_id"][k, p], out["slots_count"][k, p] = v, c
        for r, (v, c) in enumerate(sorted(slots, key=lambda s: (-s[1], s[0]))[:ranks]):
            out["ids"][r, p] = v
            out["coverage"][r, p] = F(c) / F(S)
        out["dropped"][p], out["rays"][p] = dropped, rays
    return out


def assert_same(a, b, what):
    for k in ("slots_id", "slots_count", "ids", "dropped", "rays"):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert a["coverage"].dtype == b["coverage"].dtype == F and np.array_equal(a["coverage"].view(U), b["coverage"].view(U)), (what, "coverage bits")


def stream(rng, samples, pixels, alphabet):
    """random ids from an alphabet that holds reserved ids where it has room, and samples without a path"""
    pool = rng.choice(5000, size=alphabet, replace=False).astype(U)
    for k, v in enumerate((MATTE_ID_MISS, MATTE_ID_OCEAN, MATTE_ID_PARTICLE)):
        if alphabet > 3 + k:
            pool[k] = v
    ids = pool[rng.integers(0, alphabet, size=(samples, pixels))]
    ids[rng.random((samples, pixels)) < 0.15] = EMPTY
    ids[:, 3] = EMPTY  # a pixel of no path at all
    return ids


@pytest.mark.parametrize("alphabet", [1, 3, 8, 9, 20])
@pytest.mark.parametrize("samples", [1, 5, 16, 64])
def test_the_twin_equals_the_restatement(samples, alphabet):
    rng = np.random.default_rng(1000 * samples + alphabet)
    ids = stream(rng, samples, 67, alphabet)
    for ranks in (1, 6, 8):
        assert_same(matte_host(ids, ranks), matte_python(ids, ranks), (samples, alphabet, ranks))
    got = matte_host(ids, 8)
    assert np.array_equal(got["slots_count"].sum(axis=0) + got["dropped"], (ids != EMPTY).sum(axis=0)), "sum of counts + dropped = samples with a path"
    if alphabet <= SLOTS:
        assert not got["dropped"].any()
    if alphabet == 20 and samples == 64:
        assert got["dropped"].any(), "twenty ids over 64 samples must overflow eight slots somewhere"


# ---- hand cases ----
def test_one_id_throughout_covers_exactly_one():
    got = matte_host(np.full((16, 2), 77, U), 8)
    assert (got["ids"][0] == 77).all() and (got["coverage"][0].view(U) == F(1.0).view(U)).all()
    assert (got["ids"][1:] == EMPTY).all() and (got["coverage"][1:].view(U) == 0).all(), "EMPTY and +0 beyond the occupied slots"
    assert (got["rays"] == 16).all() and not got["dropped"].any()


def test_equal_counts_rank_by_ascending_id():
    ids = np.array([[9], [4], [MATTE_ID_MISS], [4], [9], [MATTE_ID_MISS], [2]], U)
    got = matte_host(ids, 8)
    assert got["slots_id"][:4, 0].tolist() == [9, 4, MATTE_ID_MISS, 2], "slots in order of first appearance"
    assert got["ids"][:5, 0].tolist() == [4, 9, MATTE_ID_MISS, 2, EMPTY]
    assert got["coverage"][:4, 0].tolist() == [F(2) / F(7), F(2) / F(7), F(2) / F(7), F(1) / F(7)]


def test_a_ninth_id_stays_dropped_even_as_the_most_frequent():
    ids = np.array([[k] for k in range(10, 18)] + [[99]] * 20 + [[10]], U)
    got = matte_host(ids, 8)
    assert 99 not in got["slots_id"][:, 0] and 99 not in got["ids"][:, 0]
    assert got["dropped"][0] == 20 and got["rays"][0] == 29
    assert got["ids"][0, 0] == 10 and got["coverage"][0, 0] == F(2) / F(29)
    assert_same(got, matte_python(ids, 8), "ninth id")


def test_fewer_ranks_truncate_and_leave_dropped_alone():
    rng = np.random.default_rng(5)
    ids = stream(rng, 64, 67, 20)
    full, cut = matte_host(ids, 8), matte_host(ids, 3)
    assert np.array_equal(cut["ids"], full["ids"][:3]) and np.array_equal(cut["coverage"].view(U), full["coverage"][:3].view(U))
    for k in ("slots_id", "slots_count", "dropped", "rays"):
        assert np.array_equal(cut[k], full[k]), k
    assert full["dropped"].any()


def test_a_pixel_without_any_path():
    got = matte_host(np.full((5, 3), EMPTY, U), 8)
    assert not got["rays"].any() and not got["dropped"].any() and (got["ids"] == EMPTY).all() and (got["coverage"].view(U) == 0).all()
    assert (got["slots_id"] == EMPTY).all() and not got["slots_count"].any()


# ---- the mask ----
def mask_numpy(slots_id, slots_count, samples, ids):
    listed = np.isin(slots_id, np.asarray(ids, U)) & (slots_count > 0)
    return (np.where(listed, slots_count, 0).sum(axis=0).astype(U)).astype(F) / F(samples)


def test_the_mask_twin_equals_numpy():
    rng = np.random.default_rng(11)
    ids = stream(rng, 16, 67, 20)
    t = matte_host(ids, 8)
    present = np.unique(t["slots_id"][t["slots_count"] > 0])
    cases = [[], [int(present[0])], present[:5].tolist(), [4999999], present[:15].tolist() + [4999999], present[:16].tolist(), [int(present[1])] * 2, [EMPTY], [MATTE_ID_MISS, MATTE_ID_OCEAN]]
    for want in cases:
        got = matte_mask_host_twin(t["slots_id"], t["slots_count"], 16, want)
        assert np.array_equal(got.view(U), mask_numpy(t["slots_id"], t["slots_count"], 16, want).view(U)), want
    assert not matte_mask_host_twin(t["slots_id"], t["slots_count"], 16, [4999999]).any(), "an id in no slot covers nothing"
    assert not matte_mask_host_twin(t["slots_id"], t["slots_count"], 16, [EMPTY]).any(), "EMPTY is no id: unused slots cover nothing"
    # all of a pixel's ids and what was dropped: every sample that had a path
    for p in (0, 5, 40):
        own = t["slots_id"][:, p]
        m = matte_mask_host_twin(t["slots_id"], t["slots_count"], 16, own)
        assert m[p] == F(t["rays"][p] - t["dropped"][p]) / F(16)


# ---- refusals ----
def test_the_twins_refuse_bad_counts_and_null_arrays():
    fn = luminary_amd._lib().lumc_matte_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 6
    ids = np.ones((1025, 2), U)
    outs = [np.full((8, 2), 42, U), np.full((8, 2), 42, U), np.full((8, 2), 42, U), np.full((8, 2), 42, F), np.full(2, 42, U), np.full(2, 42, U)]
    ptrs = [a.ctypes.data for a in outs]
    for samples in (0, 1025, 1 << 20):
        assert fn(ids.ctypes.data, samples, 2, 8, *ptrs) == 1, samples
    for ranks in (0, 9, 1 << 20):
        assert fn(ids.ctypes.data, 4, 2, ranks, *ptrs) == 1, ranks
    assert fn(None, 4, 2, 8, *ptrs) == 1
    assert all((a == 42).all() for a in outs), "a refusal writes nothing"
    assert fn(ids.ctypes.data, 1024, 2, 8, *ptrs) == 0 and fn(ids.ctypes.data, 4, 2, 1, *([None] * 6)) == 0, "the limits are taken; every output is optional"
    for bad in (np.zeros((0, 2), U), np.ones((1025, 2), U)):
        with pytest.raises(ValueError):
            matte_host(bad, 8)
    for ranks in (0, 9):
        with pytest.raises(ValueError):
            matte_host(np.ones((4, 2), U), ranks)
    mk = luminary_amd._lib().lumc_matte_mask_host_twin
    mk.restype = C.c_int
    mk.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    si, sc, want, mask = np.ones((8, 2), U), np.ones((8, 2), U), np.ones(17, U), np.full(2, 42, F)
    assert mk(si.ctypes.data, sc.ctypes.data, 2, 4, want.ctypes.data, 17, mask.ctypes.data) == 1, "seventeen ids"
    assert mk(None, sc.ctypes.data, 2, 4, want.ctypes.data, 1, mask.ctypes.data) == 1 and mk(si.ctypes.data, None, 2, 4, want.ctypes.data, 1, mask.ctypes.data) == 1
    assert mk(si.ctypes.data, sc.ctypes.data, 2, 4, want.ctypes.data, 1, None) == 1 and mk(si.ctypes.data, sc.ctypes.data, 2, 4, None, 1, mask.ctypes.data) == 1
    assert mk(si.ctypes.data, sc.ctypes.data, 2, 0, want.ctypes.data, 1, mask.ctypes.data) == 1 and mk(si.ctypes.data, sc.ctypes.data, 2, 1025, want.ctypes.data, 1, mask.ctypes.data) == 1
    assert (mask == 42).all()
    assert mk(si.ctypes.data, sc.ctypes.data, 2, 4, want.ctypes.data, 16, mask.ctypes.data) == 0 and (mask == F(2.0)).all()
    with pytest.raises(ValueError):
        matte_mask_host_twin(si, sc, 4, want)


def test_the_public_getters_refuse_before_any_matte_render():
    host = scenes.zoo_scene(32, 32, 2)
    try:
        lib = luminary_amd._lib()
        ids, cov, mask, want = np.full((8, 32, 32), 42, U), np.full((8, 32, 32), 42, F), np.full((32, 32), 42, F), np.array([1, 2], U)
        get, get_mask, render = lib.luminary_ext_get_matte, lib.luminary_ext_get_matte_mask, lib.luminary_ext_render_mattes
        for fn in (get, get_mask, render):
            fn.restype = C.c_uint64
        get.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        get_mask.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
        render.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        for layer in (0, 3, 4):
            assert get(host._h, layer, 8, ids.ctypes.data, cov.ctypes.data, 32, 32) == INVALID_API_ARGUMENT, layer
            assert get_mask(host._h, layer, want.ctypes.data, 2, mask.ctypes.data, 32, 32) == INVALID_API_ARGUMENT, layer
        for ranks in (0, 9):
            assert get(host._h, 1, ranks, ids.ctypes.data, cov.ctypes.data, 32, 32) == INVALID_API_ARGUMENT, ranks
        assert get_mask(host._h, 1, want.ctypes.data, 17, mask.ctypes.data, 32, 32) == INVALID_API_ARGUMENT, "seventeen ids"
        for layers in (0, 4, 7):
            assert render(host._h, 4, layers) == INVALID_API_ARGUMENT, layers
        assert render(host._h, 1025, 3) == INVALID_API_ARGUMENT
        assert get(None, 1, 8, ids.ctypes.data, cov.ctypes.data, 32, 32) != 0 and get(host._h, 1, 8, None, None, 32, 32) != 0 and get_mask(host._h, 1, want.ctypes.data, 2, None, 32, 32) != 0
        # nothing rendered yet: an exception, not an argument error, for both layers
        for layer in (luminary_amd.MATTE_LAYER_INSTANCE, luminary_amd.MATTE_LAYER_MATERIAL):
            assert get(host._h, layer, 8, ids.ctypes.data, cov.ctypes.data, 32, 32) == API_EXCEPTION
            assert get_mask(host._h, layer, want.ctypes.data, 2, mask.ctypes.data, 32, 32) == API_EXCEPTION
        with pytest.raises(luminary_amd.LuminaryError) as e:
            host.matte(luminary_amd.MATTE_LAYER_INSTANCE, 4, 32, 32)
        assert e.value.code == API_EXCEPTION
        assert (ids == 42).all() and (cov == 42).all() and (mask == 42).all(), "a refusal writes nothing"
        st = host.matte_stats()
        assert st == {"renders": 0, "bytes": 0, "valid": 0, "samples": 0, "layers": 0, "dropped_pixels": [0, 0], "reserved": 0, "seconds": 0.0}
    finally:
        host.close()


# ---- the twin under the sanitizers, the restated hit words, the structs ----
def test_stand_alone_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/support/matte_check.cpp: the twins over the suite's alphabets, sample counts and every rank count, their refusals, as a program of its own built with the
    sanitizers."""
    exe = str(tmp_path / "matte_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",  # (linked statically: nothing is preloaded)
           "-ffp-contract=off", os.path.join(ROOT, "tests", "support", "matte_check.cpp"), os.path.join(ROOT, "luminary_amd", "csrc", "host", "matte.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert ran.returncode == 0 and "matte_check: ok" in ran.stdout, ran.stdout


def test_matte_h_restates_the_device_codes_hit_words():
    """matte.h is compiled by the host compiler too and cannot include the device headers: the words it classifies a hit by are theirs, compared as text."""
    csrc = os.path.join(ROOT, "luminary_amd", "csrc")
    device = "".join(open(os.path.join(csrc, "device", f)).read() for f in ("dev_ocean.h", "dev_particle.h", "dev_volume.h", "kernels.h"))
    matte = open(os.path.join(csrc, "host", "matte.h")).read()

    def word(text, name):
        m = re.search(r"\b%s = (0x[0-9A-Fa-f]+)u" % name, text)
        assert m, name
        return int(m.group(1), 16)
    for mine, theirs in (("kMatteHitOcean", "kHitOcean"), ("kMatteHitParticleMin", "kHitParticleMin"), ("kMatteHitParticleMax", "kHitParticleMax"),
                         ("kMatteHitTriangleLimit", "kHitTriangleLimit"), ("kMatteHitTriMask", "kHitTriMask")):
        assert word(matte, mine) == word(device, theirs), (mine, theirs)
    header = open(os.path.join(ROOT, "include", "lum_core.h")).read()
    for name, value in (("EMPTY", EMPTY), ("MISS", MATTE_ID_MISS), ("OCEAN", MATTE_ID_OCEAN), ("PARTICLE", MATTE_ID_PARTICLE)):
        assert int(re.search(r"#define LUMC_MATTE_ID_%s (0x[0-9A-F]+)u" % name, header).group(1), 16) == value == word(matte, "kMatteId" + name.capitalize())
    assert (EMPTY, MATTE_ID_MISS, MATTE_ID_OCEAN, MATTE_ID_PARTICLE) == (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC)
    assert (luminary_amd.MATTE_ID_EMPTY, luminary_amd.MATTE_ID_MISS, luminary_amd.MATTE_ID_OCEAN, luminary_amd.MATTE_ID_PARTICLE) == (EMPTY, MATTE_ID_MISS, MATTE_ID_OCEAN, MATTE_ID_PARTICLE)


def test_the_structs_have_the_headers_layout():
    src = '#include "luminary_amd.h"\n#include "lum_core.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", ' \
          'sizeof(LumMatteStats), sizeof(LuminaryMatteStats), offsetof(LumMatteStats, bytes), offsetof(LumMatteStats, dropped_pixels), offsetof(LumMatteStats, valid), ' \
          'offsetof(LumMatteStats, seconds), offsetof(LuminaryMatteStats, bytes), offsetof(LuminaryMatteStats, valid), offsetof(LuminaryMatteStats, samples), ' \
          'offsetof(LuminaryMatteStats, layers), offsetof(LuminaryMatteStats, dropped_pixels), offsetof(LuminaryMatteStats, seconds), LUMC_KERNEL_MATTE, LUMC_KERNEL_COUNT);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "p")]).split()]
    a, b = core.MatteStats, luminary_amd.MatteStats
    assert got == [C.sizeof(a), C.sizeof(b), a.bytes.offset, a.dropped_pixels.offset, a.valid.offset, a.seconds.offset, b.bytes.offset, b.valid.offset, b.samples.offset,
                   b.layers.offset, b.dropped_pixels.offset, b.seconds.offset, core.KERNELS.index("matte"), len(core.KERNELS)] == [40, 48, 8, 16, 24, 32, 8, 16, 20, 24, 28, 40, 11, 12]
    assert [name for name, _ in a._fields_] == ["samples", "layers", "bytes", "dropped_pixels", "valid", "reserved", "seconds"]
    assert [name for name, _ in b._fields_] == ["renders", "bytes", "valid", "samples", "layers", "dropped_pixels", "reserved", "seconds"]
    assert (core.FIRST_HIT_GUIDES, core.FIRST_HIT_MATTES, core.MATTE_INSTANCE, core.MATTE_MATERIAL) == (1, 2, 1, 2)
