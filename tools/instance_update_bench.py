#!/usr/bin/env python3
"""What moving instances costs per frame, on the device (mode 0) against the host's assembly (mode 1), and what the resident layout costs the ray kernels.

  LUM_BVH_SHARE=0 python tools/instance_update_bench.py [--frames 8] [--scenes hall,hall5,example,example100k] [--out profiles/instance_update.json]

Per scene two contexts take the same moved views, frame by frame: one in mode 0 (lumc_set_instance_update), one in mode 1 - the path every instance edit took before
there was a device path, and therefore the baseline. Every frame moves and rotates a third of the instances (luminary_ext_set_instance_transforms) and both
contexts take lumc_scene_update(LUMC_DIRTY_INSTANCE_TRANSFORMS | LUMC_DIRTY_LIGHTS). Reported per scene, warm (frame 0 is not reported), medians over the frames:
the instance part's `seconds` of both modes (lumc_instance_update_stats: host wall clock with the device synchronised), mode 0's split, and the wall clock around
the whole update call (light tree, light BVH and tables included: the same work in both modes). After the last frame: k_trace and k_shadow_rays milliseconds per
render step over the resident layout (mode 0's context) and over the host-assembled layout (mode 1's) of the same scene, fast flavour, the median of three steps,
the two contexts alternating, with the nodes the rays visited and how many of those were staged in LDS. One JSON document on stdout (and in --out)."""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("LUM_BVH_SHARE", "0")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from luminary_amd import Vec3, scenes  # noqa: E402
from luminary_amd.core import CNT_NODES, CNT_NODES_LDS, CNT_NODES_LDS_SHADOW, CNT_NODES_SHADOW, DIRTY_INSTANCE_TRANSFORMS, DIRTY_LIGHTS, Core  # noqa: E402

SPLIT = ("seconds", "seconds_relayout", "seconds_upload", "seconds_boxes", "seconds_build", "seconds_leaves")


def make_scene(name, width, height):
    if name == "hall":
        return scenes.hall_scene(width, height, 8)
    if name == "hall5":  # a handful of instances of the hall's largest mesh, side by side
        host = scenes.hall_scene(width, height, 8)
        mesh = max(range(host.get_num_meshes()), key=lambda m: len(host.get_mesh(m)[3]))
        for k in range(4):
            host.new_instance(mesh, position=(60.0 * (k + 1), 0.0, 0.0))
        return host
    if name == "example":
        return scenes.example_scene(width, height, 8)
    if name == "example100k":
        return scenes.example_scene(width, height, 8, sphere_segments=6, ground_res=16, num_objects=100_000)
    raise SystemExit("unknown scene " + name)


def move(host, frame, instances):
    """Every third instance (another third every frame) moved and rotated a little."""
    out = []
    for i in range(frame % 3, len(instances), 3):
        inst = instances[i]
        inst.position = Vec3(inst.position.x + 0.02, inst.position.y + 0.01 * ((i % 5) - 2), inst.position.z - 0.015)
        inst.rotation = Vec3(inst.rotation.x + 0.05, inst.rotation.y - 0.03, inst.rotation.z + 0.01 * (i % 4))
        out.append(inst)
    host.set_instance_transforms(out)


def ray_kernels(cores, spp, first):
    out = {name: {"k_trace_ms": [], "k_shadow_rays_ms": []} for name in cores}
    for c in cores.values():
        c.set_pixels(None)
        c.render(first, spp, samples_per_pass=spp)  # warm
        c.synchronize()
    for k in range(3):
        for name, c in cores.items():  # alternating
            c.reset_counters()
            c.set_profiling(True)
            c.render(first + (k + 1) * spp, spp, samples_per_pass=spp)
            c.synchronize()
            t = c.kernel_times()
            c.set_profiling(False)
            out[name]["k_trace_ms"].append(t["trace"][0]); out[name]["k_shadow_rays_ms"].append(t["shadow"][0])
            cnt = c.counters()
            out[name]["nodes"] = int(cnt[CNT_NODES]); out[name]["nodes_lds"] = int(cnt[CNT_NODES_LDS])
            out[name]["nodes_shadow"] = int(cnt[CNT_NODES_SHADOW]); out[name]["nodes_lds_shadow"] = int(cnt[CNT_NODES_LDS_SHADOW])
    for name in out:
        for key in ("k_trace_ms", "k_shadow_rays_ms"):
            runs = out[name][key]
            out[name][key] = statistics.median(runs); out[name][key + "_runs"] = runs
    return out


def run_scene(name, a):
    t0 = time.perf_counter()
    host = make_scene(name, a.width, a.height)
    n = host.get_num_instances()
    instances = [host.get_instance(i) for i in range(n)]
    cores = {"mode0": Core(0), "mode1": Core(0)}
    view = host.device_scene()
    for mode, c in enumerate(cores.values()):
        c.set_flavour("fast")
        c.set_instance_update(mode)
        c.upload(view)
    report = {"scene": name, "instances": n, "meshes": host.get_num_meshes(), "triangles": int(cores["mode0"].bvh_stats()[1]), "setup_s": time.perf_counter() - t0, "frames": []}
    for f in range(a.frames + 1):  # frame 0 warms both paths up (and lays the resident array out)
        t = time.perf_counter()
        move(host, f, instances)
        t1 = time.perf_counter()
        view = host.device_scene()
        row = {"frame": f, "host_set_transforms_s": t1 - t, "host_encode_s": time.perf_counter() - t1}
        for cname, c in cores.items():
            c.synchronize()
            t = time.perf_counter()
            c.update(view, DIRTY_INSTANCE_TRANSFORMS | DIRTY_LIGHTS)
            c.synchronize()
            row[cname + "_update_call_s"] = time.perf_counter() - t
            s = c.instance_update_stats()
            row[cname] = {k: getattr(s, k) for k in SPLIT + ("device_updates", "fallbacks", "relayouts", "tlas_nodes", "tlas_depth", "tlas_capacity", "hittable")}
        if f > 0:
            report["frames"].append(row)
    med = lambda fn: statistics.median(fn(r) for r in report["frames"])
    report["median_s"] = {"mode0_seconds": med(lambda r: r["mode0"]["seconds"]), "mode1_seconds": med(lambda r: r["mode1"]["seconds"]),
                          "mode0_update_call": med(lambda r: r["mode0_update_call_s"]), "mode1_update_call": med(lambda r: r["mode1_update_call_s"]),
                          "host_set_transforms": med(lambda r: r["host_set_transforms_s"]), "host_encode": med(lambda r: r["host_encode_s"])}
    report["median_s"].update({"mode0_" + k: med(lambda r, k=k: r["mode0"][k]) for k in SPLIT[1:]})
    report["took_fallback"] = report["frames"][-1]["mode0"]["fallbacks"] > 0
    report["bvh_stats"] = {cname: c.bvh_stats() for cname, c in cores.items()}
    if not a.no_rays:
        report["ray_kernels"] = ray_kernels(cores, a.spp, 100)
        report["ray_kernels"]["layout"] = {"mode0": "host-assembled (fallback)" if report["took_fallback"] else "resident", "mode1": "host-assembled"}
    for c in cores.values():
        c.close()
    host.close()
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scenes", default="hall,hall5,example,example100k")
    ap.add_argument("--no-rays", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    report = {"frames_per_scene": a.frames, "spp_per_step": a.spp, "width": a.width, "height": a.height, "LUM_BVH_SHARE": os.environ.get("LUM_BVH_SHARE"), "scenes": []}
    for name in a.scenes.split(","):
        report["scenes"].append(run_scene(name, a))
        if a.out:  # after every scene: a later scene that runs out of time keeps what is there
            with open(a.out, "w") as fh:
                fh.write(json.dumps(report, indent=1) + "\n")
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
