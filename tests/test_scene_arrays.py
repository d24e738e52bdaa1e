"""SceneArrays (luminary_amd/csrc/host/scene_arrays.h): who owns each array of the scene on the device, and how scene_device.hip uses the owners.

The checker is tests/support/scene_arrays_check.cpp over the counting fake of the HIP runtime that tests/test_device_buffer.py uses (tests/support/fake_hip.h):
compiled the way the host sources are (g++, -D__HIP_PLATFORM_AMD__, the ROCm headers), not linked against HIP, so it needs no GPU. Its cases: the whole scene
freed by one assignment, one part released and refilled with every other part's pointers unchanged, moved vertices (the traversal triangles keep their address),
the resident re-layout (ids, transforms and rows keep theirs), and a part or a re-layout whose n-th allocation fails. The other tests read the sources: the
ownership that used to be found by comparing addresses, and the writes through a cast view, must not come back."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HOST = os.path.join(ROOT, "luminary_amd", "csrc", "host")


def _code(path):
    return "\n".join(line.split("//")[0] for line in open(path).read().splitlines())


def test_scene_arrays_free_what_they_hold_exactly_once_part_by_part(tmp_path):
    exe = str(tmp_path / "scene_arrays_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"),
                           os.path.join(ROOT, "tests", "support", "scene_arrays_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok (0 failures)"), r.stdout


def test_the_header_is_host_only_and_includes_the_two_it_names():
    code = _code(os.path.join(HOST, "scene_arrays.h"))
    assert "__device__" not in code and "__global__" not in code
    assert [line.strip() for line in code.splitlines() if line.strip().startswith("#include")] == ['#include "bvh_build.h"', '#include "device_buffer.h"']


def test_the_allocation_groups_are_gone():
    for d, _, files in os.walk(os.path.join(ROOT, "luminary_amd", "csrc")):
        for f in files:
            text = open(os.path.join(d, f), errors="replace").read()
            for name in ("scene_allocs", "AllocGroup", "kGrp"):
                assert name not in text, (f, name)


def test_the_scene_unit_writes_through_owners_and_never_looks_an_owner_up_by_address():
    code = _code(os.path.join(HOST, "scene_device.hip"))
    assert "const_cast" not in code
    # no buffer's address is compared with a view of the scene (sc.<view>, ctx->scene.<view>), in either order
    view = r"(?:reinterpret_cast<[^>]*>\()?\s*(?:sc|ctx->scene)\.\w+\)?"
    assert not re.search(r"get\(\)\s*[=!]=\s*" + view, code)
    assert not re.search(view + r"\s*[=!]=\s*[\w.>\[\]-]+\.get\(\)", code)
