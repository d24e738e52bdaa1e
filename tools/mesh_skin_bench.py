#!/usr/bin/env python3
"""What a skinned mesh costs per frame on the hall when the library takes the bones, against the caller skinning on the CPU and handing over every vertex.

  python tools/mesh_skin_bench.py [--frames 8] [--runs 3] [--out profiles/mesh_skin.json]

The scene is the hall of tools/resident_refit_bench.py (one mesh, 1.43 M triangles, and a second, small instance so that two instances can be hit), the refit in
the resident node array on. The motion is a two-bone bend of the large mesh whose angle grows over the frames. Two hosts of this process take every frame:
  skin      luminary_ext_bind_mesh_skin once, then luminary_ext_set_mesh_pose per frame: 96 bytes go to the device, k_deform_mesh writes the vertices there
  baseline  the route before there was one: the same positions and normals - from lumc_skin_host, the same bytes - handed to luminary_ext_set_mesh_positions
A frame's update is the edit call plus the host call that brings the device up to date, luminary_ext_render_samples of one sample of a small frame (the same on
both hosts; its own time is measured on an unchanged scene and reported as render_s), wall clock. The CPU skinning that the baseline's caller has to do is timed
apart (caller_skin_s): the baseline's update does not include it. Warm: frame 0 is not reported. The whole animation runs --runs times; per frame the median over
the runs is recorded, with the split of lumc_mesh_skin_stats / lumc_resident_refit_stats / lumc_mesh_refit_stats and the bytes moved. One JSON document on stdout
(and in --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from luminary_amd import scenes  # noqa: E402
from luminary_amd.core import skin_host  # noqa: E402


def rotation_z(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def bone(r, pivot):
    return np.concatenate([r, (pivot - r @ pivot).reshape(3, 1)], axis=1).astype(np.float32).reshape(12)


def two_bone_weights(p0):
    p = p0.reshape(-1, 3).astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    axis = int(np.argmax(hi - lo))
    u = (p[:, axis] - lo[axis]) / (hi[axis] - lo[axis])
    s = (u * u * (3.0 - 2.0 * u)).astype(np.float32)
    w = np.zeros((len(p), 4), np.float32)
    w[:, 0], w[:, 1] = np.float32(1.0) - s, s
    ids = np.zeros((len(p), 4), np.uint16)
    ids[:, 1] = 1
    return ids.reshape(-1, 12), w.reshape(-1, 12)


def make_host(a):
    host = scenes.hall_scene(a.width, a.height, 2, target_triangles=a.triangles)
    mesh = max(range(host.get_num_meshes()), key=lambda m: len(host.get_mesh(m)[3]))
    p0 = host.get_mesh(mesh)[0]
    lo, hi = p0.reshape(-1, 3).min(axis=0), p0.reshape(-1, 3).max(axis=0)
    centre, size = 0.5 * (lo + hi), float((hi - lo).max())
    box, _ = scenes._box()
    prop = host.add_mesh(box, np.full(len(box), host.get_mesh(mesh)[3][0], dtype=np.uint16))
    host.new_instance(prop, tuple(float(x) for x in centre), (0.2, 0.4, 0.0), (0.01 * size,) * 3)
    host.set_mesh_refit_in_place(1)
    return host, mesh


def frame(host, edit):
    t = time.perf_counter()
    edit()
    t_edit = time.perf_counter() - t
    host.render_samples(0, 1, samples_per_pass=1)
    return t_edit, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--height", type=int, default=36)
    ap.add_argument("--triangles", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    (skin, mesh), (base, _) = make_host(a), make_host(a)
    rest_p, rest_n = skin.get_mesh(mesh)[:2]
    ids, w = two_bone_weights(rest_p)
    pivot = 0.5 * (rest_p.reshape(-1, 3).min(axis=0) + rest_p.reshape(-1, 3).max(axis=0)).astype(np.float64)
    for h in (skin, base):
        h.render_samples(0, 1, samples_per_pass=1)
    skin.bind_mesh_skin(mesh, ids, w, 2)
    rows = {f: [] for f in range(1, a.frames + 1)}
    for run in range(a.runs):
        for f in range(a.frames + 1):  # frame 0 warms both routes up and lays the resident arrays out
            angle = 0.02 * f / max(a.frames, 1) + (0.001 if f == 0 else 0.0) + 1e-4 * run
            bones = np.stack([bone(np.eye(3), pivot), bone(rotation_z(angle), pivot)])
            t = time.perf_counter()
            p, n, _ = skin_host(rest_p, rest_n, ids, w, bones)
            caller = time.perf_counter() - t
            s_edit, s_all = frame(skin, lambda: skin.set_mesh_pose(mesh, bones))
            b_edit, b_all = frame(base, lambda: base.set_mesh_positions(mesh, p, n))
            t = time.perf_counter()
            skin.render_samples(1, 1, samples_per_pass=1)
            render = time.perf_counter() - t
            if f == 0:
                continue
            ss, sr, sm = skin.mesh_skin_stats(), skin.resident_refit_stats(), skin.mesh_refit_stats()
            br, bm = base.resident_refit_stats(), base.mesh_refit_stats()
            rows[f].append({"skin_update_s": s_all, "skin_edit_s": s_edit, "baseline_update_s": b_all, "baseline_edit_s": b_edit, "caller_skin_s": caller, "render_s": render,
                            "skin": {"skinning_s": ss["seconds"], "palette_upload_s": ss["seconds_upload"], "kernel_s": ss["seconds_skin"], "bytes_uploaded": ss["last_bytes_uploaded"],
                                     "resident_s": sr["seconds"], "vertex_upload_s": sr["seconds_upload"], "hash_s": sr["seconds_hash"], "refit_s": sr["seconds_refit"], "cost_s": sr["seconds_cost"],
                                     "top_level_s": sr["seconds_top_level"], "bytes_downloaded": sr["last_bytes_downloaded"], "lights_s": sm["seconds_lights"], "refits": sm["last_refits"],
                                     "host_materialisations": ss["host_materialisations"], "fallbacks": sr["fallbacks"]},
                            "baseline": {"resident_s": br["seconds"], "vertex_upload_s": br["seconds_upload"], "hash_s": br["seconds_hash"], "refit_s": br["seconds_refit"], "cost_s": br["seconds_cost"],
                                         "top_level_s": br["seconds_top_level"], "bytes_uploaded": 48 * int(p.size // 9), "lights_s": bm["seconds_lights"], "refits": bm["last_refits"],
                                         "fallbacks": br["fallbacks"]}})

    def median(items):
        out = {}
        for k, v in items[0].items():
            out[k] = median([i[k] for i in items]) if isinstance(v, dict) else statistics.median(i[k] for i in items)
        return out

    frames = [dict(frame=f, **median(rows[f])) for f in sorted(rows)]
    report = {"scene": "hall + one small instance, refit in place", "triangles": int(len(rest_p)), "bones": 2, "runs": a.runs, "frames_per_run": a.frames,
              "width": a.width, "height": a.height, "frames": frames,
              "median_s": {k: statistics.median(r[k] for r in frames) for k in ("skin_update_s", "baseline_update_s", "skin_edit_s", "baseline_edit_s", "caller_skin_s", "render_s")}}
    text = json.dumps(report, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    skin.close(); base.close()


if __name__ == "__main__":
    main()
