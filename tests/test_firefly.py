"""Firefly rejection on the host side (include/lum_core.h lumc_firefly_resolve_host; include/luminary_amd.h luminary_ext_set_firefly_rejection; csrc/host/firefly.h,
firefly.cpp, api.cpp), no GPU.

The resolved pixel is one function compiled twice; this file holds the host's compilation - the twin - to a numpy restatement of the definition (firefly.h's header
comment), float32 one operation at a time, byte for byte; tests/test_firefly_gpu.py holds the device's compilation to the twin. Then the hand cases of the
definition on the restatement (and, with it, on the twin), what the twin and the public setters refuse, the twin under the sanitizers as a program of its own, and
the layout of the structs. (lumc_set_firefly_buckets needs a context, which needs a device: its refusals of K = 1, 3, 17 are in tests/test_firefly_gpu.py.)"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import luminary_amd
from luminary_amd import core, scenes
from luminary_amd.core import firefly_resolve_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U = np.float32, np.uint32
INVALID_API_ARGUMENT = 3
BUCKETS = [4, 5, 8, 16]


def counts_of(K, S):
    """ids [0, S) dealt to K buckets"""
    return np.bincount(np.arange(S) % K, minlength=K).astype(U)


def sample_counts(K):
    return [1, 3, K - 1, K, K + 1, 8 * K, 8 * K + 3]


# ---- the definition, restated ----
def resolve_numpy(sums, counts, image):
    """firefly.h, steps 1 to 9, float32 one operation at a time, over all pixels at once. sums [K, 3, P], counts [K], image [3, P].
    Returns (image after the resolve, (rewritten, trimmed, nonfinite), c [P], written [P])."""
    sums, counts, image = np.asarray(sums, F), np.asarray(counts, U), np.asarray(image, F).copy()
    K, _, P = sums.shape
    used = [b for b in range(K) if counts[b] > 0]
    m = len(used)
    mean, key, finite = np.zeros((K, 3, P), F), np.zeros((K, P), F), np.zeros((K, P), bool)
    with np.errstate(all="ignore"):
        for b in used:
            mean[b] = sums[b] / F(counts[b])
            finite[b] = np.isfinite(mean[b]).all(axis=0)
            lum = (F(0.212655) * mean[b, 0] + F(0.715158) * mean[b, 1]) + F(0.072187) * mean[b, 2]
            assert lum.dtype == F
            key[b] = np.where(finite[b] & (lum > 0), lum, F(0.0))
        mf = finite.sum(axis=0).astype(U)
        rank = np.zeros((K, P), U)
        for b in range(K):
            for j in range(K):
                if j != b:
                    rank[b] += (finite[j] & ((key[j] < key[b]) | ((key[j] == key[b]) & (j < b)))).astype(U)
        num, den = np.zeros(P, F), np.zeros(P, F)
        for b in range(K):
            t = (rank[b] + U(1)).astype(F) * key[b]
            num = np.where(finite[b], num + t, num)
            den = np.where(finite[b], den + key[b], den)
        fm = mf.astype(F)
        d = (F(2.0) * num) / (fm * den) - (mf + U(1)).astype(F) / fm
        G = np.where(d > 0, np.where(d < 1, d, F(1.0)), F(0.0)).astype(F)
        gc = G * (mf >> U(1)).astype(F)
        trims = (mf >= 4) & (den > 0)
        c = np.where(trims, np.minimum(gc.astype(U), np.maximum(mf >> U(1), U(1)) - U(1)), U(0)).astype(U)
        written = ~((c == 0) & (mf == m))
        s = np.zeros((3, P), F)
        for b in range(K):
            keep = finite[b] & (rank[b] >= c) & (rank[b] < mf - c)
            s = np.where(keep[None, :], s + mean[b], s)
        out = s / (mf - U(2) * c).astype(F)[None, :]
        out = np.where((mf == 0)[None, :], F(0.0), out).astype(F)
    assert num.dtype == den.dtype == d.dtype == gc.dtype == out.dtype == F
    image[:, written] = out[:, written]
    return image, (int(written.sum()), int((2 * c[written].astype(np.int64)).sum()), int((mf != m).sum())), c, written


def random_buckets(rng, K, counts, P):
    """Bucket sums [K, 3, P] of a plausible accumulation - a pixel's level times the bucket's count, a few percent of noise - with, by pixel index mod 10: one
    bucket 10 ... 10^6 times brighter, two such buckets, a NaN channel, a +Inf bucket, an all-black pixel, negative sums, equal buckets (every key ties), -Inf and a
    huge finite bucket; the others plain."""
    level = np.exp(rng.normal(0.0, 2.0, (1, 3, P)))
    sums = (level * counts[:, None, None] * rng.uniform(0.8, 1.25, (K, 3, P))).astype(F)
    kind, px = np.arange(P) % 10, np.arange(P)
    b1, b2 = rng.randint(0, K, P), rng.randint(0, K, P)
    big = (10.0 ** rng.uniform(1.0, 6.0, P)).astype(F)
    for k in (1, 2):
        sel = kind == k
        sums[b1[sel], :, px[sel]] *= big[sel, None]
    sel = kind == 2
    sums[b2[sel], :, px[sel]] *= big[sel, None]
    sel = kind == 3
    sums[b1[sel], 1, px[sel]] = np.nan
    sel = kind == 4
    sums[b1[sel], :, px[sel]] = np.inf
    sums[:, :, kind == 5] = 0.0
    sums[:, :, kind == 6] *= F(-1.0)
    sel = kind == 7
    sums[:, :, sel] = (level[0][:, sel] * counts[:, None, None]).astype(F)
    sel = kind == 8
    sums[b1[sel], 0, px[sel]] = -np.inf
    sums[b2[sel], :, px[sel]] = F(3.0e38)
    return sums


def words(a):
    return np.ascontiguousarray(a, F).view(U)


@pytest.mark.parametrize("K", BUCKETS)
def test_the_twin_is_the_definition_byte_for_byte(K):
    rng = np.random.RandomState(K)
    P = 1000
    for S in sample_counts(K):
        counts = counts_of(K, S)
        sums = random_buckets(rng, K, counts, P)
        image = rng.uniform(0.0, 2.0, (3, P)).astype(F)
        got, stats = firefly_resolve_host(sums, counts, image)
        want, want_stats, c, written = resolve_numpy(sums, counts, image)
        assert np.array_equal(words(got), words(want)), "K = %d, S = %d: %d of %d words differ" % (K, S, int((words(got) != words(want)).sum()), got.size)
        assert stats == want_stats, (K, S, stats, want_stats)
        if S < 4:
            assert not c.any(), "fewer than four buckets with samples are never trimmed"
        if S >= 8 * K:
            assert c.any() and written.any() and not written.all() and stats[2] > 0, "the random pixels cover rewritten, trimmed, untouched and non-finite ones"


# ---- hand cases, on the restatement and the twin alike ----
def both(sums, counts, image):
    sums = np.asarray(sums, F)
    want, want_stats, c, written = resolve_numpy(sums, counts, image)
    got, stats = firefly_resolve_host(sums, counts, image)
    assert np.array_equal(words(got), words(want)) and stats == want_stats
    return want, want_stats, c, written


def level_buckets(K, S, spread=0.1, seed=0):
    """one pixel; bucket means within +-spread of each other, around (1, 2, 0.5)"""
    rng = np.random.RandomState(seed)
    counts = counts_of(K, S)
    mean = np.array([1.0, 2.0, 0.5])[None, :] * (1.0 + spread * rng.uniform(-1.0, 1.0, (K, 1)))
    return (mean * counts[:, None]).astype(F)[:, :, None], counts, (mean.astype(F))


@pytest.mark.parametrize("K", BUCKETS)
def test_hand_cases(K):
    S = 8 * K
    image = np.array([[7.0], [8.0], [9.0]], F)
    # all bucket means within +-10 % of each other: untouched. The Gini coefficient of keys in [0.9, 1.1] is at most 0.05 (half of them at either end), and
    # 0.05 * (K >> 1) <= 0.4 truncates to c = 0 for every K <= 16.
    sums, counts, mean = level_buckets(K, S)
    out, stats, c, written = both(sums, counts, image)
    assert c[0] == 0 and not written[0] and np.array_equal(out, image) and stats == (0, 0, 0)
    # the same with one bucket at 1000 x: trimmed, and every channel within [min, max] of the other buckets' means
    for hot in (0, K // 2, K - 1):
        spiked = sums.copy()
        spiked[hot] *= F(1000.0)
        out, stats, c, written = both(spiked, counts, image)
        others = np.delete(mean, hot, axis=0)
        assert c[0] >= 1 and written[0] and stats == (1, 2 * int(c[0]), 0)
        lo, hi = others.min(axis=0), others.max(axis=0)
        assert ((out[:, 0] >= lo) & (out[:, 0] <= hi)).all(), (out[:, 0], lo, hi)
    # all-zero buckets: untouched
    out, stats, c, written = both(np.zeros_like(sums), counts, image)
    assert not written[0] and np.array_equal(out, image) and stats == (0, 0, 0)
    # one NaN or +Inf bucket among equal finite ones: the finite mean, counted as a non-finite pixel
    equal = (np.array([1.5, 0.25, 3.0])[None, :] * counts[:, None]).astype(F)[:, :, None]
    for bad in (np.nan, np.inf):
        for where in (0, K - 1):
            for ch in range(3):
                broken = equal.copy()
                broken[where, ch, 0] = bad
                out, stats, c, written = both(broken, counts, image)
                assert written[0] and c[0] == 0 and stats == (1, 0, 1)
                assert np.array_equal(out[:, 0], np.array([1.5, 0.25, 3.0], F)), out[:, 0]
    # all buckets non-finite: 0
    out, stats, c, written = both(np.full_like(sums, np.nan), counts, image)
    assert written[0] and np.array_equal(words(out), np.zeros((3, 1), U)) and stats == (1, 0, 1)
    mixed = equal.copy()
    mixed[::2, 0, 0] = np.inf
    mixed[1::2, 2, 0] = np.nan
    out, stats, _, _ = both(mixed, counts, image)
    assert np.array_equal(words(out), np.zeros((3, 1), U)) and stats == (1, 0, 1)


@pytest.mark.parametrize("K", BUCKETS)
def test_fewer_than_four_finite_buckets_are_never_trimmed(K):
    image = np.array([[7.0], [8.0], [9.0]], F)
    for S in (1, 2, 3):  # S < 4: m < 4
        counts = counts_of(K, S)
        sums = np.zeros((K, 3, 1), F)
        sums[:S] = F(1.0)
        sums[0] = F(1.0e6)
        out, stats, c, written = both(sums, counts, image)
        assert c[0] == 0 and not written[0] and stats == (0, 0, 0) and np.array_equal(out, image)
    # m = K but m' = 3: the three finite ones are averaged, outlier and all
    counts = counts_of(K, 8 * K)
    sums = np.full((K, 3, 1), np.nan, F)
    sums[:3] = F(8.0)
    sums[1] = F(8.0e6)
    out, stats, c, written = both(sums, counts, image)
    want = (F(1.0) + F(1.0e6) + F(1.0)) / F(3.0)
    assert c[0] == 0 and written[0] and stats == (1, 0, 1) and (out == want).all()


@pytest.mark.parametrize("K", BUCKETS)
def test_equal_keys_rank_by_bucket_index(K):
    """Buckets of negative radiance all have the key 0 whatever their values: K - 1 of them, each with a value of its own, tie, and one bright bucket makes the
    Gini coefficient (K - 1) / K, so c = (uint32) ((K - 1) / K * (K >> 1)) >= 1 buckets go at either end. Which of the tied ones go is decided by the bucket index
    alone, and the output - the mean of the values that are left - shows it. The expected order is a stable sort of the keys."""
    counts = counts_of(K, K)  # one id per bucket: mean = sum
    image = np.zeros((3, 1), F)
    for bright in (K - 1, 0, K // 2):
        values = -(np.arange(K) + 1.0)
        values[bright] = 1000.0
        sums = np.repeat(values.astype(F)[:, None, None], 3, axis=1)
        out, stats, c, written = both(sums, counts, image)
        assert int(c[0]) == int((K - 1) / K * (K >> 1)) >= 1 and written[0] and stats == (1, 2 * int(c[0]), 0)
        order = np.argsort(np.where(values > 0, values, 0.0), kind="stable")  # ties keep the index order
        kept = sorted(order[int(c[0]):K - int(c[0])])
        assert bright not in kept
        want = F(0.0)
        for b in kept:
            want = want + F(values[b])
        want = want / F(len(kept))
        assert (out == want).all(), (bright, out[:, 0], want, kept)
    # all keys equal, one bucket non-finite: nothing trimmed, the mean of the rest
    flat = np.full((K, 3, 1), 2.0, F)
    flat[1, 1, 0] = np.nan
    out, stats, c, written = both(flat, counts, image)
    assert c[0] == 0 and stats == (1, 0, 1) and (out == F(2.0)).all()


def test_the_twin_refuses_bad_bucket_counts_null_arrays_and_empty_buckets():
    fn = luminary_amd._lib().lumc_firefly_resolve_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    sums, counts, image, stats = np.ones((17, 3, 2), F), np.ones(17, U), np.full((3, 2), 9, F), np.full(3, 42, U)
    for K in (0, 1, 3, 17, 1000):
        assert fn(sums.ctypes.data, counts.ctypes.data, K, 2, image.ctypes.data, stats.ctypes.data) == 1, K
    assert fn(None, counts.ctypes.data, 4, 2, image.ctypes.data, stats.ctypes.data) == 1
    assert fn(sums.ctypes.data, None, 4, 2, image.ctypes.data, stats.ctypes.data) == 1
    assert fn(sums.ctypes.data, counts.ctypes.data, 4, 2, None, stats.ctypes.data) == 1
    assert fn(sums.ctypes.data, np.zeros(4, U).ctypes.data, 4, 2, image.ctypes.data, stats.ctypes.data) == 1, "no bucket has samples"
    assert (image == 9).all() and (stats == 42).all(), "a refusal writes nothing"
    assert fn(sums.ctypes.data, counts.ctypes.data, 4, 2, image.ctypes.data, None) == 0, "the stats are optional"
    with pytest.raises(ValueError):
        firefly_resolve_host(np.ones((3, 3, 2), F), np.ones(3, U), image)


# ---- the public setters: every refusal that needs no device ----
def test_the_public_setter_refuses_bad_bucket_counts_and_keeps_its_settings():
    host = scenes.zoo_scene(32, 32, 2)
    try:
        f = host.get_firefly_rejection()
        assert (bool(f.enabled), int(f.buckets)) == (False, 8), "off by default, eight buckets"
        fn = luminary_amd._lib().luminary_ext_set_firefly_rejection
        fn.restype = C.c_uint64
        for buckets in (0, 1, 3, 17, 1 << 20):
            for enabled in (False, True):
                bad = luminary_amd.FireflySettings(enabled, buckets)
                assert fn(host._h, C.byref(bad)) == INVALID_API_ARGUMENT, (enabled, buckets)
        f = host.get_firefly_rejection()
        assert (bool(f.enabled), int(f.buckets)) == (False, 8), "a refusal changes nothing"
        assert fn(host._h, None) != 0 and fn(None, C.byref(f)) != 0
        host.set_firefly_rejection(enabled=True, buckets=5)
        f = host.get_firefly_rejection()
        assert (bool(f.enabled), int(f.buckets)) == (True, 5)
        st = host.firefly_stats()
        assert st == {"frames_resolved": 0, "frames_skipped": 0, "last_rewritten": 0, "last_trimmed": 0, "last_nonfinite": 0, "buckets": 0, "bytes": 0}
        out = np.zeros((32, 32, 3), F)
        get = luminary_amd._lib().luminary_ext_get_robust_radiance
        get.restype = C.c_uint64
        assert get(host._h, out.ctypes.data_as(C.c_void_p), C.c_uint32(32), C.c_uint32(32)) != 0, "nothing rendered yet"
    finally:
        host.close()


# ---- the twin under the sanitizers, the structs ----
def test_stand_alone_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/support/firefly_check.cpp: the twin over every bucket count and the suite's sample counts, its refusals, as a program of its own built with the sanitizers."""
    exe = str(tmp_path / "firefly_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",  # (linked statically: nothing is preloaded)
           "-ffp-contract=off", os.path.join(ROOT, "tests", "support", "firefly_check.cpp"), os.path.join(ROOT, "luminary_amd", "csrc", "host", "firefly.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert ran.returncode == 0 and "firefly_check: ok" in ran.stdout, ran.stdout


def test_the_structs_have_the_headers_layout():
    src = '#include "luminary_amd.h"\n#include "lum_core.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", ' \
          'sizeof(LumFireflyStats), sizeof(LuminaryFireflyStats), sizeof(LuminaryFireflySettings), offsetof(LumFireflyStats, bytes), offsetof(LumFireflyStats, resolves), ' \
          'offsetof(LumFireflyStats, last_rewritten), offsetof(LumFireflyStats, samples), offsetof(LuminaryFireflySettings, buckets), ' \
          'offsetof(LuminaryFireflyStats, last_rewritten), offsetof(LuminaryFireflyStats, buckets), offsetof(LuminaryFireflyStats, bytes));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "p")]).split()]
    a, b, s = core.FireflyStats, luminary_amd.FireflyStats, luminary_amd.FireflySettings
    assert got == [C.sizeof(a), C.sizeof(b), C.sizeof(s), a.bytes.offset, a.resolves.offset, a.last_rewritten.offset, a.samples.offset, s.buckets.offset,
                   b.last_rewritten.offset, b.buckets.offset, b.bytes.offset] == [40, 40, 8, 8, 16, 24, 36, 4, 16, 28, 32]
    assert [name for name, _ in a._fields_] == ["buckets", "reserved", "bytes", "resolves", "last_rewritten", "last_trimmed", "last_nonfinite", "samples"]
    assert [name for name, _ in b._fields_] == ["frames_resolved", "frames_skipped", "last_rewritten", "last_trimmed", "last_nonfinite", "buckets", "bytes"]
    assert [name for name, _ in s._fields_] == ["enabled", "buckets"]
