#!/usr/bin/env python3
"""Firefly rejection (lumc_set_firefly_buckets / lumc_firefly_resolve): what it costs and what it does, measured on the GPU.

  python tools/firefly_bench.py [--cost] [--effect] [--buckets 8] [--repeats 5] [--width 480 --height 270] [--reference-ids 16384] [--out FILE.json]

  --cost    the bench's hall at 1920 x 1080, 8 bounces, 64 ids per pass (bench.py's step), in the library's default flavour. Steps with the switch off and on
            alternate in one session, a host clock around each step up to the device's synchronise; then, with the core's kernel stamps on, the `accumulate`
            category of a step with the switch on minus that of a step with it off is k_bucket_accumulate, and the `output` category around lumc_firefly_resolve
            alone is k_firefly_resolve. Bytes are computed from the shapes: results re-read (16 B per path), planes read and written once per pass.
  --effect  a firefly-prone scene - the zoo under water, the sun through the waves: caustics - at 64 and 1024 ids against a plain render of --reference-ids other
            ids (first id 65536: independent of the images it judges). For the plain image and for the resolved one at K = 4, 8, 16: the relative L2 error,
            the ratio of the image's mean to the reference's (below 1: the estimator's dark bias) and the share of pixels rewritten.
Without either flag both parts run. Prints as it goes and writes everything to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from luminary_amd import SKY_MODE_DEFAULT, scenes  # noqa: E402
from luminary_amd.core import Core  # noqa: E402

PASS = 64


def cost(K, repeats):
    width, height = 1920, 1080
    P = width * height
    host, label = bench.build_workload("hall", width, height, 8), bench.WORKLOADS["hall"]
    core = Core(0)
    try:
        core.upload(host.device_scene())
        core.set_pixels(None)

        def step(first):
            t = time.perf_counter()
            core.render(first, PASS, samples_per_pass=PASS)
            core.synchronize()
            return 1e3 * (time.perf_counter() - t)

        for on in (0, 1):  # both shapes warmed up
            core.set_firefly_buckets(K if on else 0)
            step(0)
        ms = {0: [], 1: []}
        for r in range(repeats):
            for on in (0, 1):
                core.set_firefly_buckets(K if on else 0)  # (clears the accumulators: every step starts from the same state)
                core.synchronize()
                ms[on].append(step(PASS * r))
        core.set_profiling(True)
        cat = {}
        for on in (0, 1):
            core.set_firefly_buckets(K if on else 0)
            before = core.kernel_times()["accumulate"]
            for r in range(repeats):
                step(PASS * r)
            after = core.kernel_times()["accumulate"]
            cat[on] = ((after[0] - before[0]) / repeats, (after[1] - before[1]) // repeats)
        core.generate_result(uniform_samples=PASS * repeats)
        before = core.kernel_times()["output"]
        for r in range(repeats):
            core._call("lumc_firefly_resolve", None, None)
        core.synchronize()
        after = core.kernel_times()["output"]
        resolve_ms = (after[0] - before[0]) / repeats
        stats = core.firefly_stats()
        core.set_profiling(False)
        bucket_ms = cat[1][0] - cat[0][0]
        bucket_bytes = 16.0 * P * PASS + 2.0 * 12.0 * K * P
        resolve_bytes = 12.0 * K * P + 12.0 * stats.last_rewritten
        out = {
            "workload": label, "width": width, "height": height, "ids_per_pass": PASS, "buckets": K, "flavour": core.flavour, "repeats": repeats,
            "step_ms_off": ms[0], "step_ms_on": ms[1], "step_ms_off_median": float(np.median(ms[0])), "step_ms_on_median": float(np.median(ms[1])),
            "step_on_over_off": float(np.median(ms[1]) / np.median(ms[0])),
            "spread_off": float((max(ms[0]) - min(ms[0])) / np.median(ms[0])), "spread_on": float((max(ms[1]) - min(ms[1])) / np.median(ms[1])),
            "accumulate_category_ms_off": cat[0][0], "accumulate_category_ms_on": cat[1][0], "accumulate_category_launches_off": cat[0][1], "accumulate_category_launches_on": cat[1][1],
            "k_bucket_accumulate_ms": bucket_ms, "k_bucket_accumulate_bytes": bucket_bytes, "k_bucket_accumulate_tb_s": bucket_bytes / (bucket_ms * 1e-3) / 1e12 if bucket_ms > 0 else None,
            "k_firefly_resolve_ms": resolve_ms, "k_firefly_resolve_bytes": resolve_bytes, "k_firefly_resolve_tb_s": resolve_bytes / (resolve_ms * 1e-3) / 1e12 if resolve_ms > 0 else None,
            "resolve_pixels_rewritten_share": stats.last_rewritten / P, "plane_bytes": int(stats.bytes),
        }
        print("cost, %s, K = %d, %s flavour" % (label, K, core.flavour))
        print("  step (64 ids): off %s ms, on %s ms; medians %.2f / %.2f ms, on / off = %.4f (spread of the repeats: %.2f %% / %.2f %%)" % (
            ["%.1f" % x for x in ms[0]], ["%.1f" % x for x in ms[1]], out["step_ms_off_median"], out["step_ms_on_median"], out["step_on_over_off"], 100 * out["spread_off"], 100 * out["spread_on"]))
        print("  k_bucket_accumulate: %.3f ms per pass (accumulate category %.3f -> %.3f ms), %.2f GB by the shapes = %.2f TB/s" % (
            bucket_ms, cat[0][0], cat[1][0], bucket_bytes / 1e9, out["k_bucket_accumulate_tb_s"] or 0.0))
        print("  k_firefly_resolve: %.3f ms, %.2f GB = %.2f TB/s, %.2f %% of the pixels rewritten" % (
            resolve_ms, resolve_bytes / 1e9, out["k_firefly_resolve_tb_s"] or 0.0, 100 * out["resolve_pixels_rewritten_share"]))
        return out
    finally:
        core.close()


def effect_scene(width, height):
    host = scenes.zoo_scene(width, height, 8, sky_mode=SKY_MODE_DEFAULT)
    o = host.get_ocean()
    o.active, o.height, o.amplitude, o.frequency, o.caustics_active = True, 4.5, 0.3, 0.5, True
    host.set_ocean(o)
    return host


def effect(width, height, reference_ids):
    P = width * height
    view = effect_scene(width, height).device_scene()
    rows = []
    core = Core(0)
    try:
        core.upload(view)
        core.set_pixels(None)
        t = time.perf_counter()
        core.render(65536, reference_ids, samples_per_pass=PASS)
        reference = core.generate_result(uniform_samples=reference_ids).astype(np.float64)
        print("effect, zoo under water with caustics, %d x %d, %s flavour: reference of %d ids in %.1f s, mean %.5g, %d values not finite" % (
            width, height, core.flavour, reference_ids, time.perf_counter() - t, float(np.nanmean(reference)), int((~np.isfinite(reference)).sum())))
        good = np.isfinite(reference).all(axis=0)  # (a pixel the reference itself lost to a NaN judges nothing)
        norm = float(np.sqrt((reference[:, good] ** 2).sum()))

        def judge(image):
            image = image.astype(np.float64)[:, good]
            finite = np.isfinite(image)
            err = np.where(finite, image - reference[:, good], reference[:, good])
            return float(np.sqrt((err ** 2).sum()) / norm), float(np.where(finite, image, 0.0).mean() / reference[:, good].mean()), int((~finite).sum())

        for K in (4, 8, 16):
            core.set_firefly_buckets(K)
            done = 0
            for ids in (64, 1024):
                core.render(done, ids - done, samples_per_pass=PASS)
                done = ids
                plain = core.generate_result(uniform_samples=ids)
                robust = core.firefly_resolve()
                st = core.firefly_stats()
                row = {"buckets": K, "ids": ids, "plain": judge(plain), "robust": judge(robust), "rewritten_share": st.last_rewritten / P,
                       "trimmed_per_rewritten_pixel": st.last_trimmed / max(st.last_rewritten, 1), "nonfinite_pixels": st.last_nonfinite}
                rows.append(row)
                print("  K = %2d, %4d ids: relative L2 error plain %.4f robust %.4f | mean over reference's plain %.4f robust %.4f | %.2f %% of the pixels rewritten, %.2f buckets trimmed each, %d with a non-finite bucket" % (
                    K, ids, row["plain"][0], row["robust"][0], row["plain"][1], row["robust"][1], 100 * row["rewritten_share"], row["trimmed_per_rewritten_pixel"], row["nonfinite_pixels"]))
        return {"scene": "zoo_scene under water (ocean height 4.5, caustics)", "width": width, "height": height, "flavour": core.flavour, "reference_ids": reference_ids,
                "reference_first_id": 65536, "columns": "plain / robust: [relative L2 error, mean over the reference's mean, values not finite]", "rows": rows}
    finally:
        core.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--effect", action="store_true")
    ap.add_argument("--buckets", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--reference-ids", type=int, default=16384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    both = not (a.cost or a.effect)
    record = {}
    if a.cost or both:
        record["cost"] = cost(a.buckets, a.repeats)
    if a.effect or both:
        record["effect"] = effect(a.width, a.height, a.reference_ids)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
