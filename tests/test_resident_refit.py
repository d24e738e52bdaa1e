"""What the refit in the resident node array rests on, on the host (csrc/host/bvh_build.cpp layout_resident_nodes with its slot map, resident_depth_slots), no GPU.

A mesh's nodes are no range of the resident array - the tops of all meshes come first -, so the device's refit walks per-mesh slot lists by depth below the
mesh's root. tests/support/resident_refit_check.cpp holds the slot map, the depth lists and a host twin of the device's loop to layout_resident_nodes over
refit_bvh4's trees, byte for byte. tests/test_resident_refit_gpu.py holds the device's kernels to the same bytes."""
import os
import subprocess

import pytest

from luminary_amd import build as lum_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stand_alone_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "resident_refit_check")
    host = os.path.join(ROOT, "luminary_amd", "csrc", "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
           "-I", os.path.join(lum_build.ROCM, "include"), os.path.join(ROOT, "tests", "support", "resident_refit_check.cpp"), os.path.join(host, "bvh_build.cpp"), "-lpthread", "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)  # (the runtimes are linked statically: the program needs nothing preloaded)
    assert ran.returncode == 0 and "resident_refit_check: ok" in ran.stdout, ran.stdout


def test_the_switch_is_refused_by_name_and_the_stats_have_the_header_s_layout():
    """No device: the ctypes mirrors against the C headers, compiled."""
    import ctypes as C
    import luminary_amd
    from luminary_amd import core
    src = '#include "luminary_amd.h"\n#include "lum_core.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(LumResidentRefitStats), ' \
          'sizeof(LuminaryResidentRefitStats), offsetof(LumResidentRefitStats, seconds), offsetof(LuminaryResidentRefitStats, seconds_top_level));return 0;}\n'
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "p")]).split()]
    assert got == [C.sizeof(core.ResidentRefitStats), C.sizeof(luminary_amd.ResidentRefitStats), core.ResidentRefitStats.seconds.offset, luminary_amd.ResidentRefitStats.seconds_top_level.offset] == [80, 80, 32, 72]
    # the two structs the issue leaves alone
    assert C.sizeof(core.InstanceUpdateStats) == 88 and C.sizeof(core.MeshRefitStats) == 96
    host = luminary_amd.Host()
    try:
        with pytest.raises(luminary_amd.LuminaryError, match="luminary_ext_set_mesh_refit_in_place"):
            host.set_mesh_refit_in_place(2)
        host.set_mesh_refit_in_place(1)
        host.set_mesh_refit_in_place(0)
        stats = host.resident_refit_stats()  # (no context yet: zeros)
        assert stats["updates"] == 0 and stats["fallbacks"] == 0
    finally:
        host.close()
