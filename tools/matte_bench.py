#!/usr/bin/env python3
"""ID mattes (lumc_render_first_hits): what they add to the first-hit passes, measured on the GPU.

  python tools/matte_bench.py [--samples 4 16] [--repeats 5] [--width 1920 --height 1080] [--parent-lib PATH] [--out FILE.json]

The bench's hall at 1920 x 1080 in the library's default flavour. Per sample count, in one session and alternating: lumc_render_first_hits with GUIDES alone, with
GUIDES | MATTES (both layers), and with MATTES alone; a host clock around each call up to the device's synchronise. Then, with the core's kernel stamps on, the
`matte` category: k_matte_accumulate per pass, k_matte_resolve (a download of eight ranks, the copies not counted: stamps only) and k_matte_mask. Bytes are computed
from the shapes: 68 B read and 8 B written per pixel, layer and pass.

--parent-lib: a library built from the parent commit (python -m luminary_amd.build in a checkout of it). Its lumc_render_guides is timed by a child process of this
tool that loads that library, the same scene, sample counts and repeats, before and after this process's own measurements; the guides-only time of this library
has to stay within the run-to-run spread of the parent's, and the tool says whether it does."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(core, fn):
    core.synchronize()
    t = time.perf_counter()
    fn()
    core.synchronize()
    return 1e3 * (time.perf_counter() - t)


def guides_only(core, samples, repeats):
    """lumc_render_guides alone: what a parent library can run too"""
    core.render_guides(samples)
    return [timed(core, lambda: core._call("lumc_render_guides", samples, None)) for _ in range(repeats)]


def summary(ms):
    return {"ms": ms, "median": float(np.median(ms)), "spread": float((max(ms) - min(ms)) / np.median(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--guides-only", action="store_true", help="(the child's mode: lumc_render_guides alone, one JSON line)")
    a = ap.parse_args()

    def parent_run():
        env = dict(os.environ, LUM_LIB=os.path.abspath(a.parent_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--guides-only", "--repeats", str(a.repeats), "--width", str(a.width), "--height", str(a.height), "--samples"] + [str(s) for s in a.samples]
        out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, check=True, timeout=600).stdout
        return json.loads(out.strip().splitlines()[-1])

    parent = [parent_run()] if a.parent_lib and not a.guides_only else []
    import bench
    from luminary_amd.core import FIRST_HIT_GUIDES, FIRST_HIT_MATTES, MATTE_INSTANCE, Core
    host = bench.build_workload("hall", a.width, a.height, 8)
    core = Core(0)
    P = a.width * a.height
    try:
        core.upload(host.device_scene())
        if a.guides_only:
            print(json.dumps({str(s): guides_only(core, s, a.repeats) for s in a.samples}))
            return
        result = {"workload": bench.WORKLOADS["hall"], "width": a.width, "height": a.height, "flavour": core.flavour, "repeats": a.repeats, "by_samples": {}}
        for S in a.samples:
            modes = {"guides": (FIRST_HIT_GUIDES, 3), "guides+mattes": (FIRST_HIT_GUIDES | FIRST_HIT_MATTES, 3), "mattes": (FIRST_HIT_MATTES, 3),
                     "guides+instance layer": (FIRST_HIT_GUIDES | FIRST_HIT_MATTES, MATTE_INSTANCE)}
            ms = {k: [] for k in modes}
            for what, layers in modes.values():  # every shape warmed up, the planes allocated
                core.render_first_hits(S, what, layers)
            for _ in range(a.repeats):
                for k, (what, layers) in modes.items():
                    ms[k].append(timed(core, lambda: core.render_first_hits(S, what, layers)))
            entry = {k: summary(v) for k, v in ms.items()}
            entry["render_guides"] = summary(guides_only(core, S, a.repeats))
            entry["mattes_over_guides"] = entry["guides+mattes"]["median"] / entry["guides"]["median"]
            # the kernels by their stamps
            core.set_profiling(True)
            before = core.kernel_times()["matte"]
            for _ in range(a.repeats):
                core.render_first_hits(S, FIRST_HIT_GUIDES | FIRST_HIT_MATTES, 3)
            core.synchronize()
            acc = core.kernel_times()["matte"]
            for _ in range(a.repeats):
                core.mattes(MATTE_INSTANCE, 8)
            res = core.kernel_times()["matte"]
            ids = np.unique(core.mattes(MATTE_INSTANCE, 1)[0])[:16]
            mid = core.kernel_times()["matte"]
            for _ in range(a.repeats):
                core.matte_mask(MATTE_INSTANCE, ids)
            mask = core.kernel_times()["matte"]
            core.set_profiling(False)
            per = lambda hi, lo: (hi[0] - lo[0]) / max(hi[1] - lo[1], 1)  # noqa: E731
            entry["k_matte_accumulate_ms_per_pass"] = per(acc, before)
            entry["k_matte_accumulate_GBps"] = 2 * (68.0 + 8.0) * P / (per(acc, before) * 1e-3) / 1e9
            entry["k_matte_resolve_ms"] = per(res, acc)
            entry["k_matte_resolve_GBps"] = (68.0 + 8.0 * 8 + 8.0) * P / (per(res, acc) * 1e-3) / 1e9
            entry["k_matte_mask_ms"] = per(mask, mid)
            entry["k_matte_mask_GBps"] = (64.0 + 4.0) * P / (per(mask, mid) * 1e-3) / 1e9
            st = core.matte_stats()
            entry["stats"] = {"bytes": int(st.bytes), "dropped_pixels": list(st.dropped_pixels), "seconds": float(st.seconds)}
            result["by_samples"][str(S)] = entry
            print("%4d samples: guides %.3f ms (spread %.2f %%), guides + mattes %.3f ms (x %.4f), mattes alone %.3f ms, guides + one layer %.3f ms; lumc_render_guides %.3f ms" % (
                S, entry["guides"]["median"], 100 * entry["guides"]["spread"], entry["guides+mattes"]["median"], entry["mattes_over_guides"], entry["mattes"]["median"],
                entry["guides+instance layer"]["median"], entry["render_guides"]["median"]))
            print("             k_matte_accumulate %.4f ms per pass (%.0f GB/s), k_matte_resolve %.4f ms (%.0f GB/s), k_matte_mask %.4f ms (%.0f GB/s); %s pixels dropped samples" % (
                entry["k_matte_accumulate_ms_per_pass"], entry["k_matte_accumulate_GBps"], entry["k_matte_resolve_ms"], entry["k_matte_resolve_GBps"], entry["k_matte_mask_ms"],
                entry["k_matte_mask_GBps"], entry["stats"]["dropped_pixels"]))
    finally:
        core.close()
        host.close()
    if a.parent_lib:
        parent.append(parent_run())
        for S in a.samples:
            runs = [summary(p[str(S)]) for p in parent]
            both = [x for p in parent for x in p[str(S)]]
            lo, hi = min(both), max(both)
            mine = result["by_samples"][str(S)]["render_guides"]["median"]
            result["by_samples"][str(S)]["parent_render_guides"] = {"runs": runs, "min": lo, "max": hi, "within": bool(lo <= mine <= hi)}
            print("%4d samples: parent's lumc_render_guides %.3f / %.3f ms (medians of the two runs; all repeats %.3f ... %.3f), this library %.3f ms: %s" % (
                S, runs[0]["median"], runs[1]["median"], lo, hi, mine, "within the parent's spread" if lo <= mine <= hi else ("FASTER than every repeat of the parent" if mine < lo else "SLOWER than every repeat of the parent")))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
