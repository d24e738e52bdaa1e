#!/usr/bin/env python3
"""What a moved mesh costs per frame on the hall (one mesh, 1.43 M triangles), and what the refitted tree costs the ray kernels.

  python tools/mesh_refit_bench.py [--frames 8] [--spp 2] [--out profiles/mesh_refit.json]

The motion is a sine bend of the largest mesh whose amplitude grows over the frames. Per frame, three ways of bringing the same view onto the device:
  refit     luminary_ext_set_mesh_positions + lumc_scene_update(LUMC_DIRTY_MESH_POSITIONS | LIGHTS), mode 0
  rebuild   the same in mode 1
  baseline  lumc_scene_update(LUMC_DIRTY_MESHES | LIGHTS) of that view: what a mesh edit cost before there was a refit
each on a context of its own, warm (frame 0 is not reported), wall clock around the call with the device synchronised, split by lumc_mesh_refit_stats.
After frames 1, 4 and 8 (or the last): k_trace and k_shadow_rays milliseconds per render step over the refitted and over the rebuilt tree, fast flavour,
medians of three steps, next to the refitted tree's cost growth. One JSON document on stdout (and in --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from luminary_amd import scenes  # noqa: E402
from luminary_amd.core import DIRTY_LIGHTS, DIRTY_MESH_POSITIONS, DIRTY_MESHES, Core  # noqa: E402


def bend(p0, amplitude, phase):
    p = p0.reshape(-1, 3).astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    size = float((hi - lo).max())
    u = (p - lo) / size
    out = p.copy()
    out[:, 1] += amplitude * size * np.sin(6.0 * u[:, 0] + phase) * np.cos(5.0 * u[:, 2])
    return out.astype(np.float32).reshape(-1, 9)


def ray_kernel_ms(core, spp, first):
    core.set_pixels(None)
    core.render(first, spp, samples_per_pass=spp)  # warm
    core.synchronize()
    trace, shadow = [], []
    for k in range(3):
        core.set_profiling(True)
        core.render(first + (k + 1) * spp, spp, samples_per_pass=spp)
        core.synchronize()
        t = core.kernel_times()
        core.set_profiling(False)
        trace.append(t["trace"][0]); shadow.append(t["shadow"][0])
    return {"k_trace_ms": statistics.median(trace), "k_shadow_rays_ms": statistics.median(shadow)}


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
    cores = {"refit": Core(0), "rebuild": Core(0), "baseline": Core(0)}
    view = host.device_scene()
    for name, c in cores.items():
        c.set_flavour("fast")
        c.upload(view)
        c.set_pixels(None)
    cores["refit"].set_mesh_refit(0, 0.0)
    cores["rebuild"].set_mesh_refit(1, 0.0)
    report = {"scene": "hall", "triangles": int(len(p0)), "frames": [], "ray_kernels": [], "spp_per_step": a.spp, "width": a.width, "height": a.height}
    sample_at = {1, 4, a.frames}
    for f in range(a.frames + 1):  # frame 0 warms every path up
        moved = bend(p0, 0.01 * f / max(a.frames, 1) + (0.001 if f == 0 else 0.0), 0.4 * f)
        t0 = time.perf_counter()
        host.set_mesh_positions(mesh, moved, n0)
        t1 = time.perf_counter()
        view = host.device_scene()
        t2 = time.perf_counter()
        row = {"frame": f, "host_set_positions_s": t1 - t0, "host_encode_s": t2 - t1}
        for name, c in cores.items():
            c.synchronize()
            t = time.perf_counter()
            c.update(view, (DIRTY_MESHES if name == "baseline" else DIRTY_MESH_POSITIONS) | DIRTY_LIGHTS)
            c.synchronize()
            row[name + "_update_s"] = time.perf_counter() - t
            if name == "baseline":
                row[name + "_bvh_build_s"] = c.bvh_build_seconds()
            else:
                s = c.mesh_refit_stats()
                row[name] = {k: getattr(s, k) for k in ("last_refits", "last_rebuilds", "max_cost_growth", "seconds", "seconds_upload", "seconds_refit", "seconds_rebuild", "seconds_assemble", "seconds_hash", "seconds_download", "seconds_lights")}
        if f > 0:
            report["frames"].append(row)
        if f in sample_at and f > 0:
            entry = {"frame": f, "cost_growth": row["refit"]["max_cost_growth"]}
            for name in ("refit", "rebuild"):
                entry[name] = ray_kernel_ms(cores[name], a.spp, 100 * f)
            report["ray_kernels"].append(entry)
    med = lambda key: statistics.median(r[key] for r in report["frames"])
    report["median_s"] = {k: med(k) for k in ("host_set_positions_s", "host_encode_s", "refit_update_s", "rebuild_update_s", "baseline_update_s")}
    text = json.dumps(report, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    for c in cores.values():
        c.close()


if __name__ == "__main__":
    main()
