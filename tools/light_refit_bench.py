#!/usr/bin/env python3
"""What a moved emitter costs per frame when the devices refit the light tree (luminary_ext_set_light_refit), against the host building it again.

  python tools/light_refit_bench.py [--frames 8] [--runs 3] [--soup 100000] [--out profiles/light_refit.json]

The scene is the hall of tools/mesh_skin_bench.py (one mesh, 1.43 M triangles of which 64 emit, and a second, small instance), the refit in the resident node array
on. Two hosts of this process take every frame: `refit` with the switch on, `rebuild` with it off - the route before there was one. Three kinds of frame:
  skinned    luminary_ext_set_mesh_pose of the large mesh (a two-bone bend whose angle grows)
  morph      luminary_ext_set_mesh_weights of the same mesh (one target over every 16th triangle, its weight grows)
  instances  luminary_ext_set_instance_transforms of every instance (a drift)
With --soup N a second scene follows: N emissive triangles in one mesh, moved by luminary_ext_set_mesh_positions - there the long ranges of the root's top slots
show in k_light_slot_stats, and the host's build is no longer milliseconds.
A frame's update is the edit call plus the host call that brings the device up to date, luminary_ext_render_samples of one sample of a small frame (the same on
both hosts; its own time is measured on an unchanged scene and reported as render_s), wall clock. Warm: frame 0 of every kind is not reported. Every kind runs
--runs times; per frame the median over the runs is recorded, with the split of lumc_light_refit_stats. One JSON document on stdout (and in --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

os.environ.setdefault("LUM_LIGHT_REFIT_TIMING", "1")  # the per-part split of the stats (a synchronisation per part; set it to 0 for the untimed refit)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from luminary_amd import Host, scenes  # noqa: E402
from mesh_skin_bench import bone, make_host, rotation_z, two_bone_weights  # noqa: E402


def frame(host, edit):
    t = time.perf_counter()
    edit()
    t_edit = time.perf_counter() - t
    host.render_samples(0, 1, samples_per_pass=1)
    return t_edit, time.perf_counter() - t


def split(host):
    s = host.light_refit_stats()
    return {"refit_s": s["seconds"], "fragments_s": s["seconds_fragments"], "stats_s": s["seconds_stats"], "nodes_s": s["seconds_nodes"], "light_bvh_s": s["seconds_light_bvh"],
            "table_s": s["seconds_table"], "launches": s["last_launches"], "bytes_uploaded": s["last_bytes_uploaded"], "bytes_downloaded": s["last_bytes_downloaded"],
            "cost_growth": s["cost_growth"], "refits": s["refits"], "fallbacks": s["fallbacks"], "host_rebuilds": s["host_rebuilds"],
            "host_materialisations": host.mesh_skin_stats()["host_materialisations"]}


def run_kind(hosts, frames, runs, edit_of):
    """edit_of(host, frame, run) -> the edit as a callable. Returns the per-frame medians."""
    rows = {f: [] for f in range(1, frames + 1)}
    refit, rebuild = hosts
    for run in range(runs):
        for f in range(frames + 1):
            r_edit, r_all = frame(refit, edit_of(refit, f, run))
            b_edit, b_all = frame(rebuild, edit_of(rebuild, f, run))
            t = time.perf_counter()
            refit.render_samples(1, 1, samples_per_pass=1)
            render = time.perf_counter() - t
            if f == 0:
                continue
            rows[f].append({"refit_update_s": r_all, "refit_edit_s": r_edit, "rebuild_update_s": b_all, "rebuild_edit_s": b_edit, "render_s": render,
                            "lights_s_rebuild": rebuild.mesh_refit_stats()["seconds_lights"], "refit": split(refit)})

    def median(items):
        out = {}
        for k, v in items[0].items():
            out[k] = median([i[k] for i in items]) if isinstance(v, dict) else statistics.median(i[k] for i in items)
        return out

    per_frame = [dict(frame=f, **median(rows[f])) for f in sorted(rows)]
    keys = ("refit_update_s", "rebuild_update_s", "refit_edit_s", "rebuild_edit_s", "render_s")
    return {"frames": per_frame, "median_s": {k: statistics.median(r[k] for r in per_frame) for k in keys},
            "range_s": {k: [min(r[k] for r in per_frame), max(r[k] for r in per_frame)] for k in keys}}


def soup_host(n, width, height, on):
    rng = np.random.RandomState(17)
    host = Host()
    scenes.apply_benchmark_settings(host, width, height, 2, sky=(0.02, 0.02, 0.03))
    grey = host.add_material(scenes._material((0.6, 0.6, 0.6), 0.6))
    lamp = host.add_material(scenes._material((0.8, 0.8, 0.8), 0.5, emission=(4.0, 4.0, 4.0)))
    floor = np.float32([[-60, -12, -60, 60, -12, -60, 60, -12, 60], [-60, -12, -60, 60, -12, 60, -60, -12, 60]])
    host.new_instance(host.add_mesh(floor, np.full(2, grey, dtype=np.uint16)))
    c = rng.uniform(-40.0, 40.0, (n, 1, 3))
    tris = (c + rng.normal(size=(n, 3, 3)) * 0.3).astype(np.float32).reshape(n, 9)
    mesh = host.add_mesh(tris, np.full(n, lamp, dtype=np.uint16))
    host.new_instance(mesh, rotation=(0.1, 0.2, 0.0))
    scenes.set_camera(host, (0.0, 0.0, 120.0), (0.0, 0.0, 0.0))
    host.set_mesh_refit_in_place(1)
    host.set_light_refit(on)
    return host, mesh, tris


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--height", type=int, default=36)
    ap.add_argument("--triangles", type=int, default=1_000_000)
    ap.add_argument("--soup", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    (refit, mesh), (rebuild, _) = make_host(a), make_host(a)
    refit.set_light_refit(1)
    hosts = (refit, rebuild)
    rest_p, rest_n = refit.get_mesh(mesh)[:2]
    emitters = int(refit.device_scene().num_lights)
    ids, w = two_bone_weights(rest_p)
    pivot = 0.5 * (rest_p.reshape(-1, 3).min(axis=0) + rest_p.reshape(-1, 3).max(axis=0)).astype(np.float64)
    size = float((rest_p.reshape(-1, 3).max(axis=0) - rest_p.reshape(-1, 3).min(axis=0)).max())
    for h in hosts:
        h.render_samples(0, 1, samples_per_pass=1)
        h.bind_mesh_skin(mesh, ids, w, 2)
    report = {"scene": "hall + one small instance, refit in place", "triangles": int(len(rest_p)), "emitters": emitters, "runs": a.runs, "frames_per_run": a.frames, "width": a.width,
              "height": a.height}

    def pose(host, f, run):
        angle = 0.02 * f / max(a.frames, 1) + (0.001 if f == 0 else 0.0) + 1e-4 * run
        bones = np.stack([bone(np.eye(3), pivot), bone(rotation_z(angle), pivot)])
        return lambda: host.set_mesh_pose(mesh, bones)

    report["skinned"] = run_kind(hosts, a.frames, a.runs, pose)
    for h in hosts:
        h.unbind_mesh_skin(mesh)
    corners = np.arange(0, 3 * len(rest_p), 48, dtype=np.uint32)
    deltas = np.tile(np.float32([0.0, 0.01 * size, 0.0]), (len(corners), 1))
    for h in hosts:
        h.bind_mesh_morph(mesh, len(rest_p), [0, len(corners)], corners, deltas)

    def weights(host, f, run):
        value = np.float32([0.1 + 0.1 * f + 0.01 * run])
        return lambda: host.set_mesh_weights(mesh, value)

    report["morph"] = run_kind(hosts, a.frames, a.runs, weights)
    for h in hosts:
        h.unbind_mesh_morph(mesh)

    def drift(host, f, run):
        instances = [host.get_instance(i) for i in range(host.get_num_instances())]
        for k, inst in enumerate(instances):
            inst.position.x += 0.001 * size * (1 + k)
        return lambda: host.set_instance_transforms(instances)

    report["instances"] = run_kind(hosts, a.frames, a.runs, drift)
    for h in hosts:
        h.close()
    if a.soup:
        (on, m, tris), (off, _, _) = soup_host(a.soup, a.width, a.height, 1), soup_host(a.soup, a.width, a.height, 0)
        for h in (on, off):
            h.render_samples(0, 1, samples_per_pass=1)

        def jitter(host, f, run):
            moved = tris + np.float32(0.01 * (f + 1) + 0.001 * run)
            return lambda: host.set_mesh_positions(m, moved)

        report["soup"] = dict(emitters=a.soup, **run_kind((on, off), a.frames, a.runs, jitter))
        on.close(); off.close()
    text = json.dumps(report, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
