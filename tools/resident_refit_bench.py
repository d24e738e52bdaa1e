#!/usr/bin/env python3
"""What a moved mesh costs per frame on the hall when its tree is refitted where the nodes live, against the refit in a copy with the host's assembly.

  python tools/resident_refit_bench.py [--frames 8] [--spp 2] [--out profiles/resident_refit.json]

The scene is the hall of tools/mesh_refit_bench.py (one mesh, 1.43 M triangles) with a second, small instance of a small mesh added, so that two instances can be
hit - the moved instances' device path, which the in-place refit builds on, needs two. The motion is that tool's sine bend of the largest mesh, its amplitude
growing over the frames. Per frame the same view goes to two contexts of this process, both in mesh refit mode 0:
  in_place  lumc_set_mesh_refit_in_place(1): lumc_scene_update(LUMC_DIRTY_MESH_POSITIONS | LIGHTS) refits in the resident node array and rebuilds the top level
  copy      the switch off: the refit in a copy of the tree, the node download, assemble_scene_tree on the host, the upload of the node array
warm (frame 0 is not reported: it lays the resident array out), wall clock around the call with the device synchronised, split by lumc_resident_refit_stats and
lumc_mesh_refit_stats. After frames 1, 4 and the last: k_trace and k_shadow_rays milliseconds per render step over both contexts' trees - the same boxes in the
resident order and in the host's order -, fast flavour, medians of three steps, the contexts alternating. One JSON document on stdout (and in --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from luminary_amd import scenes  # noqa: E402
from luminary_amd.core import DIRTY_LIGHTS, DIRTY_MESH_POSITIONS, Core  # noqa: E402
from mesh_refit_bench import bend, ray_kernel_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--triangles", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    host = scenes.hall_scene(a.width, a.height, 8, target_triangles=a.triangles)
    mesh = max(range(host.get_num_meshes()), key=lambda m: len(host.get_mesh(m)[3]))
    p0, n0 = host.get_mesh(mesh)[0], host.get_mesh(mesh)[1]
    lo, hi = p0.reshape(-1, 3).min(axis=0), p0.reshape(-1, 3).max(axis=0)
    centre, size = 0.5 * (lo + hi), float((hi - lo).max())
    box, _ = scenes._box()
    prop = host.add_mesh(box, np.full(len(box), host.get_mesh(mesh)[3][0], dtype=np.uint16))
    host.new_instance(prop, tuple(float(x) for x in centre), (0.2, 0.4, 0.0), (0.01 * size,) * 3)
    cores = {"in_place": Core(0), "copy": Core(0)}
    view = host.device_scene()
    for name, c in cores.items():
        c.set_flavour("fast")
        c.set_mesh_refit(0, 0.0)
        c.set_mesh_refit_in_place(1 if name == "in_place" else 0)
        c.upload(view)
        c.set_pixels(None)
    report = {"scene": "hall + one small instance", "triangles": int(len(p0)) + int(len(box)), "instances": host.get_num_instances(), "frames": [], "ray_kernels": [],
              "spp_per_step": a.spp, "width": a.width, "height": a.height}
    sample_at = {1, 4, a.frames}
    for f in range(a.frames + 1):  # frame 0 warms both paths up and lays the resident array out
        moved = bend(p0, 0.01 * f / max(a.frames, 1) + (0.001 if f == 0 else 0.0), 0.4 * f)
        host.set_mesh_positions(mesh, moved, n0)
        view = host.device_scene()
        row = {"frame": f}
        for name, c in cores.items():
            c.synchronize()
            t = time.perf_counter()
            c.update(view, DIRTY_MESH_POSITIONS | DIRTY_LIGHTS)
            c.synchronize()
            row[name + "_update_s"] = time.perf_counter() - t
            s = c.mesh_refit_stats()
            row[name] = {k: getattr(s, k) for k in ("last_refits", "last_rebuilds", "max_cost_growth", "seconds", "seconds_upload", "seconds_refit", "seconds_assemble", "seconds_hash", "seconds_download", "seconds_lights")}
            if name == "in_place":
                r = c.resident_refit_stats()
                row["resident"] = {k: getattr(r, k) for k, _ in r._fields_}
                i = c.instance_update_stats()
                row["relayouts"] = i.relayouts
        if f > 0:
            report["frames"].append(row)
        if f in sample_at and f > 0:
            entry = {"frame": f, "cost_growth": row["in_place"]["max_cost_growth"]}
            for name in ("in_place", "copy"):
                entry[name] = ray_kernel_ms(cores[name], a.spp, 100 * f)
            report["ray_kernels"].append(entry)
    frames = report["frames"]
    med = lambda fn: statistics.median(fn(r) for r in frames)
    report["median_s"] = {"in_place_update_s": med(lambda r: r["in_place_update_s"]), "copy_update_s": med(lambda r: r["copy_update_s"]),
                          "in_place": {k: med(lambda r, k=k: r["resident"][k]) for k in ("seconds", "seconds_upload", "seconds_hash", "seconds_refit", "seconds_cost", "seconds_top_level")},
                          "copy": {k: med(lambda r, k=k: r["copy"][k]) for k in ("seconds", "seconds_upload", "seconds_refit", "seconds_hash", "seconds_download", "seconds_assemble")}}
    report["in_place_updates"], report["fallbacks"] = frames[-1]["resident"]["updates"], frames[-1]["resident"]["fallbacks"]
    text = json.dumps(report, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    for c in cores.values():
        c.close()
    host.close()


if __name__ == "__main__":
    main()
