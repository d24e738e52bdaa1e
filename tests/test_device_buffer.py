"""DeviceBuffer (luminary_amd/csrc/host/device_buffer.h), the host layer's one owner of device memory, against a counting fake of the HIP runtime.

The checker is tests/support/device_buffer_check.cpp: a stand-alone program that defines hipMalloc / hipFree / hipMemcpy itself over malloc and keeps the
set of live pointers. It is compiled the way the host sources are (g++, -D__HIP_PLATFORM_AMD__, the ROCm headers) and is not linked against HIP, so it needs
no GPU. It fails on a free of a pointer that is not live, on a second free, and on any allocation still live when a case ends; the cases are every resize
order, assign from nothing, the moves, a vector of buffers that outgrows its capacity, a struct of buffers reset by assignment, and a function shaped like
the *_host entry points with each of its allocations failing in turn."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_device_buffer_frees_what_it_holds_exactly_once(tmp_path):
    exe = str(tmp_path / "device_buffer_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"),
                           os.path.join(ROOT, "tests", "support", "device_buffer_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok (0 failures)"), r.stdout


def test_the_header_is_host_only_and_leans_on_the_runtime_api_alone():
    text = open(os.path.join(ROOT, "luminary_amd", "csrc", "host", "device_buffer.h")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "__device__" not in code and "__global__" not in code
    assert [line.strip() for line in code.splitlines() if line.strip().startswith("#include")] == ["#include <hip/hip_runtime_api.h>"]


def test_raw_allocations_live_in_the_header_alone():
    """Every hipMalloc / hipFree of the library is DeviceBuffer's: a buffer allocated beside it would have to be freed by hand again."""
    csrc = os.path.join(ROOT, "luminary_amd", "csrc")
    found = set()
    for d, _, files in os.walk(csrc):
        for f in files:
            text = open(os.path.join(d, f), errors="replace").read()
            if "hipMalloc(" in text or "hipFree(" in text:
                found.add(f)
    assert found == {"device_buffer.h"}
