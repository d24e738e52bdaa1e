"""Refit of a 4-wide tree to moved primitives on the host (csrc/host/bvh_build.cpp refit_bvh4, bvh4_cost; lum_core.h lumc_bvh_refit_probe), no GPU.

A refit keeps the topology - child words, prims, depth - and rewrites every occupied child box as the builders' pad of the exact union of what lies
below it. Min and max are exact, so a refit to the boxes a tree was built from must give the built nodes back byte for byte; under any motion the tree
stays valid (every primitive in exactly one leaf, every box holds what is below it), however bad it becomes. The cost - sum of the child boxes' half
areas - is what a caller judges that by. tests/test_mesh_refit_gpu.py holds the device's kernels to this implementation."""
import os
import subprocess

import numpy as np
import pytest

from luminary_amd import build as lum_build
from luminary_amd.core import bvh_refit_probe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 3, 5, 257, 7500]
EMPTY = 0xFFFFFFFF
FLT_MAX = np.float32(3.4028234663852886e38)


def soup(rng, n, spread=10.0):
    """The soup of tests/test_lbvh.py test_gpu_builders_on_triangle_soups."""
    c = rng.uniform(-1.0, 1.0, (n, 1, 3)) * spread
    return (c + rng.normal(size=(n, 3, 3)) * rng.choice([0.05, 0.5, 4.0], size=(n, 1, 1))).astype(np.float32)


def boxes_of(tris):
    t = np.asarray(tris, dtype=np.float32)
    return np.concatenate([t.min(axis=1), t.max(axis=1)], axis=1)


def motions(n):
    """name -> (triangles the tree is built from, triangles it is refitted to)"""
    tris = soup(np.random.RandomState(n), n)
    half = tris.copy()
    half[::2] += np.float32(1e4)
    return tris, {"fresh draw": soup(np.random.RandomState(n + 1000), n), "one point": np.broadcast_to(np.float32([1.5, -2.25, 3.0]), tris.shape).copy(), "half moved by 1e4": half}


def assert_same_topology(built, refit, where):
    assert built.shape == refit.shape, where
    assert np.array_equal(built[:, 24:28], refit[:, 24:28]), "%s: child words changed" % where
    empty = built[:, 24:28] == EMPTY
    lo = np.stack([refit[:, 4 * a:4 * a + 4].view(np.float32) for a in range(3)])
    hi = np.stack([refit[:, 12 + 4 * a:16 + 4 * a].view(np.float32) for a in range(3)])
    assert (lo[:, empty] == FLT_MAX).all() and (hi[:, empty] == -FLT_MAX).all(), "%s: an empty slot was touched" % where
    assert np.array_equal(built[:, 28:], refit[:, 28:]), where


@pytest.mark.parametrize("n", SIZES)
def test_a_refit_to_the_same_boxes_is_the_built_tree(n):
    b = boxes_of(soup(np.random.RandomState(n), n))
    r = bvh_refit_probe(b, b, "sah", on_gpu=False)
    assert r["valid"] == 1 and sorted(r["prims"]) == list(range(n))
    assert r["refit"] is not None and r["built"].tobytes() == r["refit"].tobytes(), "host builder: a child box is not the padded union of what lies below it"
    assert r["cost"][0] > 0.0 and r["cost"][1] / r["cost"][0] == 1.0


@pytest.mark.parametrize("n", SIZES)
def test_a_refit_stays_valid_under_hostile_motion(n):
    tris, to = motions(n)
    for name, moved in to.items():
        r = bvh_refit_probe(boxes_of(tris), boxes_of(moved), "sah", on_gpu=False)
        assert r["valid"] == 1, "%s, n = %d" % (name, n)
        assert_same_topology(r["built"], r["refit"], "%s, n = %d" % (name, n))
        print("n = %d, %s: cost x %.3f" % (n, name, r["cost"][1] / r["cost"][0]))


@pytest.mark.parametrize("n", SIZES)
def test_doubling_every_coordinate_quadruples_the_cost_exactly(n):
    """x2 is exact in binary32, for the coordinates and - with coordinates in [0.1, 10], where the pad's 1e-30 term is far below half an ulp of its 1e-5 * |x| term -
    for the padded boxes; the areas are products of two such differences, summed in double: every term, and every partial sum, is exactly 4 times its counterpart."""
    tris = np.random.RandomState(n).uniform(0.1, 10.0, (n, 3, 3)).astype(np.float32)
    r = bvh_refit_probe(boxes_of(tris), boxes_of(tris * np.float32(2.0)), "sah", on_gpu=False)
    assert r["valid"] == 1 and r["cost"][1] / r["cost"][0] == 4.0


def test_a_tree_with_other_references_than_primitives_cannot_be_refitted():
    b = boxes_of(soup(np.random.RandomState(5), 257))
    r = bvh_refit_probe(b, b[:256], "sah", on_gpu=False)
    assert r["refit"] is None and r["valid"] == 0 and r["cost"][1] == 0.0
    r = bvh_refit_probe(b, np.concatenate([b, b[:1]]), "sah", on_gpu=False)
    assert r["refit"] is None and r["valid"] == 0


def test_stand_alone_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/support/bvh_refit_check.cpp: identity, hostile motion and the unrefittable tree again, as a program of its own built with the sanitizers."""
    exe = str(tmp_path / "bvh_refit_check")
    host = os.path.join(ROOT, "luminary_amd", "csrc", "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
           "-I", os.path.join(lum_build.ROCM, "include"), os.path.join(ROOT, "tests", "support", "bvh_refit_check.cpp"), os.path.join(host, "bvh_build.cpp"), "-lpthread", "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)  # (the runtimes are linked statically: the program needs nothing preloaded)
    assert ran.returncode == 0 and "bvh_refit_check: ok" in ran.stdout, ran.stdout
