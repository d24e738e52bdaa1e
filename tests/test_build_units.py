"""Which translation unit compiles which kernel (luminary_amd/build.py HIP_SOURCES), read off the objects the build leaves in luminary_amd/lib/obj, and the
launcher table every flavour fills (csrc/device/wavefront_table_impl.h).

A kernel compiled into two units would exist twice on the device with two seed tables and two sets of attributes; a wavefront kernel that found its way
back into a host unit would make every host edit recompile it. Needs no GPU: nm over the objects, and the sources' text."""
import functools
import os
import re
import subprocess

from luminary_amd import build as lum_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "luminary_amd", "csrc", "device")
STUB = re.compile(r"^(?:void )?lum::(?:exact|fast)::__device_stub__(k_\w+)")  # "void": the demangler names a template instance's return type


@functools.lru_cache(maxsize=None)
def _stubs():
    """{demangled kernel with its flavour and arguments: [objects that define its host stub]}, {object: source}"""
    lum_build.build()
    source_of = {os.path.basename(s) + ".o": s for s, _ in lum_build.HIP_SOURCES}
    defined = {}
    for obj in sorted(source_of):
        out = subprocess.run(["nm", "-C", "--defined-only", os.path.join(lum_build.OBJ_DIR, obj)], stdout=subprocess.PIPE, text=True, check=True).stdout
        for line in out.splitlines():
            parts = line.split(" ", 2)
            if len(parts) == 3 and parts[1] in "TW" and STUB.match(parts[2]):
                defined.setdefault(parts[2].replace("__device_stub__", ""), []).append(obj)
    return defined, source_of


def test_every_kernel_is_compiled_in_exactly_one_unit():
    defined, source_of = _stubs()
    names = {STUB.match(k.replace("::k_", "::__device_stub__k_", 1)).group(1) for k in defined}
    # a sample of what must have been seen at all: wavefront kernels, a template among them, and shared kernels
    assert {"k_trace", "k_shade", "k_shadow_rays", "k_generate_adaptive", "k_pixel_ray", "k_generate_lut", "k_sky_hdri", "k_accumulate", "k_to_argb8", "k_cloud_noise_shape"} <= names, sorted(names)
    twice = {k: objs for k, objs in defined.items() if len(objs) != 1}
    assert not twice, twice
    # the wavefront kernels belong to the flavours' own units: no object built from csrc/host/ holds one
    in_host = sorted(k for k, objs in defined.items() if source_of[objs[0]].startswith("host/") and re.search(r"::(k_shade\w*|k_trace)[<(]", k))
    assert not in_host, in_host
    shade = [k for k in defined if re.search(r"::k_shade<", k)]
    assert {source_of[defined[k][0]] for k in shade} == {"device/wavefront_exact.hip", "device/wavefront_fast.hip"}


def test_the_flavour_neutral_kernels_exist_in_the_exact_namespace_of_core_alone():
    """kernels_shared.h belongs to core.hip, kernels_scene.h to scene_device.hip: every kernel of either header is defined by that unit's object and no other."""
    defined, source_of = _stubs()
    for header, unit, count in (("kernels_shared.h", "core.hip", 17), ("kernels_scene.h", "scene_device.hip", 9)):
        text = open(os.path.join(DEVICE, header)).read()
        kernels = set(re.findall(r"^__global__[^\n]*?\bvoid (k_\w+)\(", text, re.M))
        assert len(kernels) == count, (header, sorted(kernels))
        for name in sorted(kernels):
            where = {k: objs for k, objs in defined.items() if re.search(r"::%s\(" % name, k)}
            assert list(where.values()) == [[unit + ".o"]] and next(iter(where)).startswith("lum::exact::"), (name, where)
        including = sorted(s for s, _ in lum_build.HIP_SOURCES if re.search(r'#include\s+"[^"]*\b%s"' % re.escape(header), open(os.path.join(lum_build.CSRC, s)).read()))
        assert including == ["host/" + unit], (header, including)


def test_kernels_h_has_no_switch_that_places_a_kernel():
    """kernels.h and the dev_*.h it includes hold no `#if !LUM_FAST` around a kernel: where something is compiled is decided by which unit includes it."""
    for f in sorted(os.listdir(DEVICE)):
        if f.endswith(".h"):
            assert not re.search(r"^#if\s+!\s*LUM_FAST", open(os.path.join(DEVICE, f)).read(), re.M), f
    for unit in ("core.hip", "scene_device.hip"):
        text = open(os.path.join(ROOT, "luminary_amd", "csrc", "host", unit)).read()
        assert not re.search(r'#include\s+"[^"]*\b(kernels|wavefront_table_impl)\.h"', text), unit


def test_the_launcher_table_assigns_every_member_by_name():
    """A member make_table() leaves out stays null and would be called through at run time; a member assigned another launcher's name is a swap."""
    decl = open(os.path.join(DEVICE, "wavefront_table.h")).read()
    struct = decl[decl.index("struct WavefrontKernels {"):decl.index("};", decl.index("struct WavefrontKernels {"))]
    code = "\n".join(line.split("//")[0] for line in struct.splitlines())
    pointers = re.findall(r"\(\*(\w+)\)\(", code)
    plain = re.findall(r"^\s*(?:const char\*|uint32_t|bool)\s+(\w+);", code, re.M)
    assert len(pointers) == 34 and plain == ["flavour", "trace_block", "fused_resolve"], (len(pointers), plain)
    impl = open(os.path.join(DEVICE, "wavefront_table_impl.h")).read()
    body = impl[impl.index("make_table() {"):impl.index("return t;")]
    assigned = dict(re.findall(r"\bt\.(\w+) = ([^;]+);", body))
    assert sorted(assigned) == sorted(pointers + plain)
    assert all(assigned[p] == p for p in pointers), {p: assigned[p] for p in pointers if assigned[p] != p}
    for p in pointers:  # each name is a launcher defined in the same header
        assert re.search(r"^static (?:int|void) %s\(" % p, impl, re.M), p
    # the tests' probes have one table of their own, filled the same way by each flavour's probe unit
    impl = open(os.path.join(DEVICE, "kernels_probe.h")).read()
    assert decl.count("struct Wavefront") == 2 and not re.search(r"WavefrontSkyProbes|wavefront_sky_probes", decl + impl)
    probes = decl[decl.index("struct WavefrontProbes {"):decl.index("};", decl.index("struct WavefrontProbes {"))]
    probe_pointers = re.findall(r"\(\*(\w+)\)\(", "\n".join(line.split("//")[0] for line in probes.splitlines()))
    body = impl[impl.index("make_probes() {"):impl.index("return p;")]
    assigned = dict(re.findall(r"\bp\.(\w+) = ([^;]+);", body))
    assert probe_pointers == ["init_sampler_seeds", "light_query_probe", "light_sample_probe", "bounce_probe", "sky_probe", "sun_probe", "sky_math_probe"]
    assert assigned == {p: p for p in probe_pointers}
    for p in probe_pointers:
        assert re.search(r"^static (?:int|void) %s\(" % p, impl, re.M), p
    assert sorted(re.findall(r"^const WavefrontProbes\* (\w+)\(\);", decl, re.M)) == ["wavefront_probes_exact", "wavefront_probes_fast"]


PROBE_UNITS = {"lum::exact::": "device/wavefront_exact_probes.hip", "lum::fast::": "device/wavefront_fast_probes.hip"}


def test_the_probe_kernels_belong_to_the_probe_units_alone():
    """Every k_*_probe stub is defined by exactly one of the two probe units, its flavour's; neither main unit nor any object built from csrc/host/ defines one."""
    defined, source_of = _stubs()
    probes = {k: objs for k, objs in defined.items() if re.search(r"::k_\w+_probe[<(]", k)}
    names = {re.search(r"::(k_\w+_probe)[<(]", k).group(1) for k in probes}
    assert names == {"k_light_query_probe", "k_light_sample_probe", "k_bounce_probe", "k_sky_probe", "k_sun_probe", "k_sky_math_probe"}, sorted(names)
    for flavour, unit in PROBE_UNITS.items():  # both flavours hold all six (k_light_sample_probe in its two forms)
        mine = [k for k in probes if k.replace("void ", "").startswith(flavour)]
        assert {re.search(r"::(k_\w+_probe)[<(]", k).group(1) for k in mine} == names and len(mine) == 7, (flavour, mine)
        for k in mine:
            assert [source_of[o] for o in probes[k]] == [unit], (k, probes[k])
    assert len(probes) == 14
    # ... and the probe units hold nothing else
    others = sorted(k for k, objs in defined.items() if k not in probes and any(source_of[o] in PROBE_UNITS.values() for o in objs))
    assert not others, others


def test_kernels_h_names_no_probe_and_probes_hip_defines_no_kernel():
    assert not re.search(r"k_\w+_probe", open(os.path.join(DEVICE, "kernels.h")).read())
    for header in ("wavefront_table_impl.h", "kernel_shadow.h"):
        assert not re.search(r"k_\w+_probe|kernels_probe\.h", open(os.path.join(DEVICE, header)).read()), header
    probe = open(os.path.join(DEVICE, "kernels_probe.h")).read()
    assert not re.search(r'#include\s+"(kernels|kernel_shadow)\.h"', probe)
    defined, source_of = _stubs()
    assert "host/probes.hip" in source_of.values()
    in_probes_hip = sorted(k for k, objs in defined.items() if "probes.hip.o" in objs)
    assert not in_probes_hip, in_probes_hip
    out = subprocess.run(["nm", "-C", "--defined-only", os.path.join(lum_build.OBJ_DIR, "probes.hip.o")], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "__device_stub__" not in out and "lumc_bounce_probe_host" in out
    host = open(os.path.join(ROOT, "luminary_amd", "csrc", "host", "probes.hip")).read()
    assert "__global__" not in host and not re.search(r'#include\s+"[^"]*\b(kernels\w*|wavefront_table_impl)\.h"', host)
