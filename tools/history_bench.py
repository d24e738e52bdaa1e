#!/usr/bin/env python3
"""Image history (lumc_history_carry / lumc_history_blend): what it costs and what it buys, measured on the GPU.

  python tools/history_bench.py [--width 1920 --height 1080] [--repeats 20] [--skip-effect] [--skip-motion] [--out FILE.json]

The bench's hall in the library's default flavour.
  cost     with the core's profiling on, k_history_reproject (for a moved camera) and k_history_blend (without and with the clamp) by the history's own launch stamps, each against the bytes by shape: carry 28 B of guides + 32 B of state gathered + 16 B written per pixel, blend
           44 B read + 44 B written (the clamp adds a 24 B device copy of the image, stamped with the kernel). Beside them, in the same session: the denoiser's five
           iterations (the `output` stamps around lumc_denoise) and one sample id of the hall (host clock around lumc_render of one id, synchronised).
  motion   the moving-instance case (lumc_set_history_motion): the scene's first instance moved by 0.3 along x between two shown frames; k_history_owner,
           k_history_motion and k_history_reproject_motion by the history's launch stamps, with the records' classes and the pixels whose owner moved.
  effect   for three fixed camera moves and a table of settings: 64 ids, the move, then the shown image at 1, 4 and 16 ids with history against the plain mean of the
           same ids, both as relative L2 distance to 256 ids of the moved camera."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MOVES = {"strafe": ((0.5, 0.0, 0.0), 0.0), "turn": ((0.0, 0.0, 0.0), 0.05), "walk": ((0.3, 0.1, -1.0), 0.02)}
CONFIGS = {"default": {}, "max_history 8": {"max_history": 8.0}, "max_history 128": {"max_history": 128.0}, "depth_tolerance 0.005": {"depth_tolerance": 0.005},
           "depth_tolerance 0.1": {"depth_tolerance": 0.1}, "normal_threshold 0.5": {"normal_threshold": 0.5}, "normal_threshold 0.99": {"normal_threshold": 0.99},
           "clamp_sigma 1.5": {"clamp_sigma": 1.5}, "clamp_sigma 3": {"clamp_sigma": 3.0}}
DEFAULTS = {"max_history": 32.0, "depth_tolerance": 0.02, "normal_threshold": 0.9, "clamp_sigma": 0.0}


def moved(host, base, move):
    c = type(base).from_buffer_copy(base)
    (dx, dy, dz), yaw = move
    c.pos.x += dx
    c.pos.y += dy
    c.pos.z += dz
    c.rotation.y += yaw
    host.set_camera(c)


def timed(core, fn):
    core.synchronize()
    t = time.perf_counter()
    fn()
    core.synchronize()
    return 1e3 * (time.perf_counter() - t)


def cost(host, base, a):
    from luminary_amd.core import Core, history_params
    P = a.width * a.height
    core = Core(0)
    out = {"flavour": core.flavour}
    try:
        core.upload(host.device_scene())
        core.set_pixels(None)
        core.render(0, 8, samples_per_pass=8)
        core.generate_result(uniform_samples=8)
        core.render_guides(4)
        core.set_history(history_params())
        core.history_blend(8)
        moved(host, base, MOVES["walk"])
        core.upload(host.device_scene())
        core.set_pixels(None)
        core.render(0, 1)
        core.generate_result(uniform_samples=1)
        core.render_guides(4)
        core.history_carry()
        st = core.history_stats()
        out["pixels"] = {"carried": st.last_carried, "rejected": st.last_rejected, "off": st.last_off}
        core.set_profiling(True)

        def stamped(fn, which):
            before = core.history_stats()
            for _ in range(a.repeats):
                fn()
            after = core.history_stats()
            ms = (getattr(after, which + "_ms") - getattr(before, which + "_ms")) / max(getattr(after, which + "_launches") - getattr(before, which + "_launches"), 1)
            return ms
        ms = stamped(core.history_carry, "carry")
        out["k_history_reproject"] = {"ms": ms, "GBps": 76.0 * P / (ms * 1e-3) / 1e9}
        for name, clamp, extra in (("k_history_blend", 0.0, 0.0), ("k_history_blend with the clamp", 1.5, 24.0)):
            core.set_history(history_params(clamp_sigma=clamp))
            core.history_blend(1)
            ms = stamped(lambda: core.history_blend(1), "blend")
            out[name] = {"ms": ms, "GBps": (88.0 + extra) * P / (ms * 1e-3) / 1e9}
        before = core.kernel_times()["output"]
        for _ in range(a.repeats):
            core.denoise(None, uniform_samples=1)
        after = core.kernel_times()["output"]
        out["denoise_5_iterations_ms"] = (after[0] - before[0]) / max(after[1] - before[1], 1)
        core.set_profiling(False)
        core.render(1, 1)
        out["one_sample_id_ms"] = float(np.median([timed(core, lambda k=k: core.render(2 + k, 1)) for k in range(5)]))
    finally:
        core.close()
        host.set_camera(base)
    for k, v in out.items():
        print("cost  ", k, v)
    return out


def motion_cost(host, a):
    from luminary_amd.core import FIRST_HIT_GUIDES, FIRST_HIT_OWNER, Core, history_params
    core = Core(0)
    out = {"instances": host.get_num_instances()}
    inst = host.get_instance(0)
    home = type(inst).from_buffer_copy(inst)
    try:
        def frame(ids):
            core.upload(host.device_scene())
            core.set_pixels(None)
            core.render(0, ids, samples_per_pass=ids)
            core.generate_result(uniform_samples=ids)
            core.render_first_hits(4, FIRST_HIT_GUIDES | FIRST_HIT_OWNER, 0)
        core.set_history(history_params())
        core.set_history_motion(True, 8.0)
        frame(8)
        core.history_blend(8)
        inst.position.x += 0.3
        host.set_instance_transforms([inst])
        frame(1)
        core.set_profiling(True)
        before = core.history_motion_stats()
        for _ in range(a.repeats):
            core.render_first_hits(4, FIRST_HIT_GUIDES | FIRST_HIT_OWNER, 0)
            core.history_carry()
        after = core.history_motion_stats()
        for name in ("owner", "motion", "reproject"):
            launches = getattr(after, name + "_launches") - getattr(before, name + "_launches")
            out["k_history_" + name + ("_motion" if name == "reproject" else "")] = {"ms": (getattr(after, name + "_ms") - getattr(before, name + "_ms")) / max(launches, 1)}
        st = core.history_stats()
        out["records"] = {"moved": after.instances_moved, "same": after.instances_same, "void": after.instances_void}
        out["pixels"] = {"carried": st.last_carried, "rejected": st.last_rejected, "off": st.last_off, "owner_moved": after.last_moved_pixels, "owner_moved_carried": after.last_moved_carried}
        out["bytes"] = after.bytes
    finally:
        core.close()
        host.set_instance_transforms([home])
    for k, v in out.items():
        print("motion", k, v)
    return out


def effect(host, base, a):
    w, h = a.width, a.height

    def radiance(n):
        fm, _ = host.accumulators()
        return fm.reshape(3, h, w).transpose(1, 2, 0).astype(np.float64) / n

    def rel(img, ref):
        return float(np.sqrt(((img - ref) ** 2).sum() / (ref ** 2).sum()))
    refs = {}
    host.set_output_properties(w, h, enabled=False)
    for name, move in MOVES.items():
        moved(host, base, move)
        host.render(256)
        refs[name] = radiance(256)
    table = {}
    for cname, fields in CONFIGS.items():
        table[cname] = {}
        for name, move in MOVES.items():
            host.set_history(enabled=False)  # whatever is held goes
            host.set_camera(base)
            host.set_history(enabled=True, **dict(DEFAULTS, **fields))
            host.set_output_properties(w, h)
            host.render(64)
            moved(host, base, move)
            row, done = {}, 0
            for n in (1, 4, 16):
                host.render(n - done)
                done = n
                shown = host.history_image(w, h)[0].astype(np.float64)
                row[str(n)] = {"history": rel(shown, refs[name]), "plain": rel(radiance(n), refs[name])}
            st = host.history_stats()
            row["carried_share"] = st["last_carried"] / float(w * h)
            table[cname][name] = row
            print("effect %-22s %-7s carried %.3f  " % (cname, name, row["carried_share"]) + "  ".join("%2s ids: %.4f (plain %.4f)" % (n, row[n]["history"], row[n]["plain"]) for n in ("1", "4", "16")))
    host.set_history(enabled=False)
    host.set_camera(base)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--skip-effect", action="store_true")
    ap.add_argument("--skip-motion", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import bench
    host = bench.build_workload("hall", a.width, a.height, 8)
    result = {"workload": bench.WORKLOADS["hall"], "width": a.width, "height": a.height, "repeats": a.repeats}
    try:
        base = host.get_camera()
        result["cost"] = cost(host, base, a)
        if not a.skip_motion:
            result["motion"] = motion_cost(host, a)
        if not a.skip_effect:
            result["effect"] = effect(host, base, a)
    finally:
        host.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
