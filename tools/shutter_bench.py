#!/usr/bin/env python3
"""What a shutter render costs on the hall, against the only route the library offered for the same image before it had one.

  python tools/shutter_bench.py [--parent-lib PATH] [--runs 3] [--slices 4] [--width 640 --height 360] [--out profiles/shutter.json]

The scene is the hall of tools/mesh_skin_bench.py (one mesh, 1.43 M triangles, and a second, small instance), warm, the refit in the resident node array on and the
light refit on. Between the keys every vertex of the large mesh moves (a smooth wave). Two routes, each run in a process of its own, alternating, --runs times:
  shutter    luminary_ext_shutter_open, luminary_ext_set_mesh_positions, luminary_ext_render_shutter(slices, n, n) for n = 1, 8 and 64 ids per slice, then the
             same call again without an edit (the keys are kept: its update time is slices + 1 applications of a time and nothing else). Per slice: the
             update - k_shutter_vertices, the refit in place, the top level, the lights - and the pass; and the whole call, wall clock.
  reference  a core context, no shutter call: per slice the caller blends the mesh's records on the CPU (numpy float32 a + t * (b - a) on the positions, the
             nearer key's normal word - cheaper than the library's blended normal, which favours this route), writes them into the view and hands the mesh's vertex
             range over through lumc_scene_update(..., LUMC_DIRTY_MESH_POSITIONS), then renders the slice's ids. With --parent-lib that process loads the parent
             commit's library (LUM_LIB); without it, this tree's.
One JSON document on stdout (and in --out): per route and n the median and the range over the runs."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
IDS = (1, 8, 64)


def moved(p0):
    p = p0.reshape(-1, 3).astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    size = float((hi - lo).max())
    out = p.copy()
    out[:, 1] += 0.004 * size * np.sin(9.0 * (p[:, 0] - lo[0]) / size) * np.cos(7.0 * (p[:, 2] - lo[2]) / size)
    return out.astype(np.float32).reshape(-1, 9)


def route_shutter(a):
    import luminary_amd
    from luminary_amd import core
    from tools.mesh_skin_bench import make_host
    host, mesh = make_host(a)
    host.set_light_refit(1)
    p0, n0 = host.get_mesh(mesh)[:2]
    p1 = moved(p0)
    host.render_samples(0, 1, samples_per_pass=1)
    rows = {}
    for n in (1,) + IDS:  # the first round warms the route up and is overwritten
        host.set_mesh_positions(mesh, p0, n0)
        host.shutter_open()
        host.set_mesh_positions(mesh, p1)
        t = time.perf_counter()
        host.render_shutter(a.slices, n, n)
        first_call = time.perf_counter() - t
        first = host.shutter_stats()
        t = time.perf_counter()
        host.render_shutter(a.slices, n, n)
        second_call = time.perf_counter() - t
        st = host.shutter_stats()
        cs = core.ShutterStats()
        fn = luminary_amd._lib().lumc_shutter_stats
        fn.restype = C.c_int
        fn(C.c_void_p(host.core_context()), C.byref(cs))
        rr, lr = host.resident_refit_stats(), host.light_refit_stats()
        rows[n] = {"call_s": first_call, "call_update_s": first["seconds_update"], "call_render_s": first["seconds_render"], "kept_keys_call_s": second_call,
                   "slice_update_s": st["seconds_update"] / (a.slices + 1), "slice_pass_s": st["seconds_render"] / a.slices,
                   "last_update": {"kernel_and_flags_s": cs.seconds, "launches": cs.last_launches, "bytes_uploaded": cs.last_bytes_uploaded, "refit_s": rr["seconds_refit"],
                                   "top_level_s": rr["seconds_top_level"], "resident_s": rr["seconds"], "lights_s": lr.get("seconds", 0.0), "fallbacks": rr["fallbacks"] + lr["fallbacks"]}}
    report = {"triangles": int(len(p0)), "kernel_bytes": 48 * 3 * int(len(p0)), "ids": {str(n): rows[n] for n in IDS}}
    host.close()
    return report


def route_reference(a):
    from luminary_amd.core import DIRTY_MESH_POSITIONS, Core
    from tools.mesh_skin_bench import make_host
    host, mesh = make_host(a)
    p0, n0 = host.get_mesh(mesh)[:2]
    view = host.device_scene()
    offsets = np.ctypeslib.as_array(C.cast(view.mesh_tri_offset, C.POINTER(C.c_uint32)), shape=(view.num_meshes + 1,))
    first, count = 3 * int(offsets[mesh]), 3 * len(p0)
    store = np.frombuffer((C.c_uint32 * (4 * count)).from_address(view.vertices + 16 * first), dtype=np.uint32).reshape(count, 4)
    rec_a = store.copy()
    host.set_mesh_positions(mesh, moved(p0))
    view = host.device_scene()
    store = np.frombuffer((C.c_uint32 * (4 * count)).from_address(view.vertices + 16 * first), dtype=np.uint32).reshape(count, 4)
    rec_b = store.copy()
    core = Core(0)
    core.set_flavour(os.environ.get("LUM_FLAVOUR", "fast"))
    core.set_mesh_refit_in_place(1)
    core.upload(view)
    core.set_pixels(None)
    core.render(0, 1, samples_per_pass=1)
    core.synchronize()
    pa, pb = rec_a[:, :3].copy().view(np.float32), rec_b[:, :3].copy().view(np.float32)
    rows = {}
    for n in (1,) + IDS:
        core.clear()
        blend_s = update_s = pass_s = 0.0
        t_call = time.perf_counter()
        for k in range(a.slices):
            t = np.float32(2 * k + 1) / np.float32(2 * a.slices)
            t0 = time.perf_counter()
            store[:, :3] = (pa + t * (pb - pa)).view(np.uint32)
            store[:, 3] = rec_a[:, 3] if t < 0.5 else rec_b[:, 3]
            t1 = time.perf_counter()
            core.update(view, DIRTY_MESH_POSITIONS)
            t2 = time.perf_counter()
            core.render(k * n, n, samples_per_pass=n)
            core.synchronize()
            t3 = time.perf_counter()
            blend_s += t1 - t0; update_s += t2 - t1; pass_s += t3 - t2
        rows[n] = {"call_s": time.perf_counter() - t_call, "slice_blend_s": blend_s / a.slices, "slice_update_s": update_s / a.slices, "slice_pass_s": pass_s / a.slices,
                   "bytes_uploaded_per_slice": 16 * count}
    report = {"triangles": int(len(p0)), "ids": {str(n): rows[n] for n in IDS}}
    core.close(); host.close()
    return report


def summary(runs):
    """Median and range of every number over the runs (dicts of the same shape)."""
    if isinstance(runs[0], dict):
        return {k: summary([r[k] for r in runs]) for k in runs[0]}
    if isinstance(runs[0], (int, float)) and len(set(runs)) > 1:
        return {"median": statistics.median(runs), "min": min(runs), "max": max(runs)}
    return runs[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=["shutter", "reference"], default=None, help="run one route in this process and print its report")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--slices", type=int, default=4)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--triangles", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.route:
        print(json.dumps(route_shutter(a) if a.route == "shutter" else route_reference(a)))
        return
    common = [sys.executable, os.path.abspath(__file__), "--slices", str(a.slices), "--width", str(a.width), "--height", str(a.height), "--triangles", str(a.triangles)]
    results = {"shutter": [], "reference": []}
    for run in range(a.runs):  # alternating: a drift of the machine hits both routes alike
        for route in ("shutter", "reference"):
            env = dict(os.environ)
            if route == "reference" and a.parent_lib:
                env["LUM_LIB"] = os.path.abspath(a.parent_lib)
            out = subprocess.run(common + ["--route", route], env=env, stdout=subprocess.PIPE, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit("route %s failed (exit %d)" % (route, out.returncode))
            results[route].append(json.loads(out.stdout.strip().splitlines()[-1]))
    report = {"scene": "hall + one small instance, refit in place, light refit on", "width": a.width, "height": a.height, "slices": a.slices, "runs": a.runs,
              "reference_library": "parent commit" if a.parent_lib else "this tree", "shutter": summary(results["shutter"]), "reference": summary(results["reference"])}
    text = json.dumps(report, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
