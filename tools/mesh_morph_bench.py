#!/usr/bin/env python3
"""What a morphed mesh costs per frame on the hall when the library takes the weights, against the caller blending on the CPU and handing over every vertex.

  python tools/mesh_morph_bench.py [--frames 8] [--runs 3] [--out profiles/mesh_morph.json]

The scene is the hall of tools/mesh_skin_bench.py (one mesh, 1.43 M triangles, and a second, small instance so that two instances can be hit), the refit in the
resident node array on. Eight targets, each a bulge over a region of the large mesh, with weights animated over the frames. Two cases, each with two hosts of this
process that take every frame:
  morph       luminary_ext_bind_mesh_morph once, then luminary_ext_set_mesh_weights per frame: 32 bytes go to the device, k_deform_mesh writes the vertices there
  morph+skin  the same mesh also bound to the two-bone bend of tools/mesh_skin_bench.py: weights and a pose per frame, 32 + 96 bytes, one kernel
  baseline    the route before there was one: the same positions and normals - from lumc_morph_host, the same bytes - handed to luminary_ext_set_mesh_positions
A frame's update is the edit call(s) plus the host call that brings the device up to date, luminary_ext_render_samples of one sample of a small frame (the same on
both hosts; its own time is measured on an unchanged scene and reported as render_s), wall clock. The CPU blend that the baseline's caller has to do is timed apart
(caller_blend_s): the baseline's update does not include it. Warm: frame 0 is not reported. The whole animation runs --runs times; per frame the median over the
runs is recorded, with the split of lumc_mesh_morph_stats / lumc_resident_refit_stats / lumc_mesh_refit_stats, the bytes moved, and the bytes the kernel reads and
writes over its time (the flags' download included). One JSON document on stdout (and in --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from luminary_amd.core import morph_host  # noqa: E402
from tools.mesh_skin_bench import bone, frame, make_host, rotation_z, two_bone_weights  # noqa: E402

TARGETS = 8


def region_targets(p0, count=TARGETS, radius=0.18, strength=0.01):
    """`count` bulges along the mesh's longest axis: (offsets, corners, delta positions, delta normals), target-major, every corner within `radius` of the mesh's
    size of a target's centre, with a smooth fall-off. Shared vertices stay shared."""
    p = p0.reshape(-1, 3).astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    size, axis = float((hi - lo).max()), int(np.argmax(hi - lo))
    offsets, corners, dp, dn = [0], [], [], []
    for t in range(count):
        centre = 0.5 * (lo + hi)
        centre[axis] = lo[axis] + (hi[axis] - lo[axis]) * (t + 0.5) / count
        d = np.linalg.norm(p - centre, axis=1) / (radius * size)
        inside = np.nonzero(d < 1.0)[0]
        fall = (1.0 - d[inside] ** 2) ** 2
        out = p[inside] - centre
        out /= np.maximum(np.linalg.norm(out, axis=1, keepdims=True), 1e-9)
        corners.append(inside.astype(np.uint32))
        dp.append((strength * size * fall[:, None] * out).astype(np.float32))
        dn.append((0.25 * fall[:, None] * out).astype(np.float32))
        offsets.append(offsets[-1] + len(inside))
    return np.asarray(offsets, np.uint32), np.concatenate(corners), np.concatenate(dp), np.concatenate(dn)


def weights_of(f, frames, run):
    phase = 2.0 * np.pi * (f / max(frames, 1) + 0.01 * run)
    return (0.5 + 0.5 * np.sin(phase + 0.7 * np.arange(TARGETS)) + (0.01 if f == 0 else 0.0)).astype(np.float32)


def run_case(a, with_skin):
    (fast, mesh), (base, _) = make_host(a), make_host(a)
    rest_p, rest_n = fast.get_mesh(mesh)[:2]
    lists = region_targets(rest_p)
    ids, sw = two_bone_weights(rest_p) if with_skin else (None, None)
    pivot = 0.5 * (rest_p.reshape(-1, 3).min(axis=0) + rest_p.reshape(-1, 3).max(axis=0)).astype(np.float64)
    for h in (fast, base):
        h.render_samples(0, 1, samples_per_pass=1)
    fast.bind_mesh_morph(mesh, len(rest_p), *lists)
    if with_skin:
        fast.bind_mesh_skin(mesh, ids, sw, 2)
    corners, entries = 3 * len(rest_p), int(lists[0][-1])
    kernel_bytes = corners * (32 + 8 + 16 + (32 if with_skin else 0)) + entries * 32
    rows = {f: [] for f in range(1, a.frames + 1)}
    for run in range(a.runs):
        for f in range(a.frames + 1):  # frame 0 warms both routes up and lays the resident arrays out
            w = weights_of(f, a.frames, run)
            bones = None
            if with_skin:
                bones = np.stack([bone(np.eye(3), pivot), bone(rotation_z(0.02 * f / max(a.frames, 1) + (0.001 if f == 0 else 0.0) + 1e-4 * run), pivot)])
            t = time.perf_counter()
            p, n, _ = morph_host(rest_p, rest_n, *lists, w, ids, sw, bones)
            caller = time.perf_counter() - t

            def edit():
                fast.set_mesh_weights(mesh, w)
                if with_skin:
                    fast.set_mesh_pose(mesh, bones)

            m_edit, m_all = frame(fast, edit)
            b_edit, b_all = frame(base, lambda: base.set_mesh_positions(mesh, p, n))
            t = time.perf_counter()
            fast.render_samples(1, 1, samples_per_pass=1)
            render = time.perf_counter() - t
            if f == 0:
                continue
            ms, ss, sr, sm = fast.mesh_morph_stats(), fast.mesh_skin_stats(), fast.resident_refit_stats(), fast.mesh_refit_stats()
            br, bm = base.resident_refit_stats(), base.mesh_refit_stats()
            rows[f].append({"morph_update_s": m_all, "morph_edit_s": m_edit, "baseline_update_s": b_all, "baseline_edit_s": b_edit, "caller_blend_s": caller, "render_s": render,
                            "morph": {"morph_s": ms["seconds"], "weights_upload_s": ms["seconds_upload"], "kernel_s": ms["seconds_morph"],
                                      "bytes_uploaded": ms["last_bytes_uploaded"] + (ss["last_bytes_uploaded"] if with_skin else 0), "kernel_bytes": kernel_bytes,
                                      "kernel_gb_per_s": kernel_bytes / max(ms["seconds_morph"], 1e-12) * 1e-9, "launches": ms["last_launches"],
                                      "resident_s": sr["seconds"], "vertex_upload_s": sr["seconds_upload"], "hash_s": sr["seconds_hash"], "refit_s": sr["seconds_refit"], "cost_s": sr["seconds_cost"],
                                      "top_level_s": sr["seconds_top_level"], "bytes_downloaded": sr["last_bytes_downloaded"], "lights_s": sm["seconds_lights"], "refits": sm["last_refits"],
                                      "host_materialisations": ms["host_materialisations"], "fallbacks": sr["fallbacks"]},
                            "baseline": {"resident_s": br["seconds"], "vertex_upload_s": br["seconds_upload"], "hash_s": br["seconds_hash"], "refit_s": br["seconds_refit"], "cost_s": br["seconds_cost"],
                                         "top_level_s": br["seconds_top_level"], "bytes_uploaded": 48 * int(p.size // 9), "lights_s": bm["seconds_lights"], "refits": bm["last_refits"],
                                         "fallbacks": br["fallbacks"]}})

    def median(items):
        out = {}
        for k, v in items[0].items():
            out[k] = median([i[k] for i in items]) if isinstance(v, dict) else statistics.median(i[k] for i in items)
        return out

    frames = [dict(frame=f, **median(rows[f])) for f in sorted(rows)]
    report = {"triangles": int(len(rest_p)), "targets": TARGETS, "entries": entries, "bones": 2 if with_skin else 0, "frames": frames,
              "median_s": {k: statistics.median(r[k] for r in frames) for k in ("morph_update_s", "baseline_update_s", "morph_edit_s", "baseline_edit_s", "caller_blend_s", "render_s")},
              "median_kernel_gb_per_s": statistics.median(r["morph"]["kernel_gb_per_s"] for r in frames)}
    fast.close(); base.close()
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--height", type=int, default=36)
    ap.add_argument("--triangles", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    report = {"scene": "hall + one small instance, refit in place", "runs": a.runs, "frames_per_run": a.frames, "width": a.width, "height": a.height,
              "morph": run_case(a, False), "morph_and_skin": run_case(a, True)}
    text = json.dumps(report, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
