"""The work buffers' two arenas (csrc/host/work_layout.h): a pass's arrays are named once per arena, the arena's size is what that layout adds up to.

tests/support/work_layout_check.cpp lays both arenas out over host memory of exactly the derived size for every path count around the 256-byte rounding,
with and without volumes and clouds, and holds the result to its own table of arrays; it is built with the address and undefined-behaviour sanitizers and
run as a program of its own, so an array that leaves its block is reported even where the arithmetic checks were wrong. No GPU."""
import os
import subprocess

from luminary_amd import build as lum_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stand_alone_layout_check_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "work_layout_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__",
           "-I", os.path.join(lum_build.ROCM, "include"), os.path.join(ROOT, "tests", "support", "work_layout_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)  # (the runtimes are linked statically: the program needs nothing preloaded)
    assert ran.returncode == 0 and "work_layout_check: ok (20 cases)" in ran.stdout, ran.stdout
