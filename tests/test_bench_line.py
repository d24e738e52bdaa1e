"""The one line bench.py prints must stay small enough for the driver to keep it whole (round 3: 21.9 KB, of which the driver kept the last 8 KB and
parsed nothing) and must carry the measurement contract's fields. A plain run measures the headline alone and can dump what its timed steps computed;
--full adds the other measurements."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("lum_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_headline_of_a_full_record_is_small_and_complete():
    b = _bench()
    with open(os.path.join(ROOT, "profiles", "r03_bench.json")) as f:  # a full record of a real run (22 KB)
        detail = json.load(f)
    detail["value_exact"] = {"value": 2612.3456789, "unit": "Mrays/s", "flavour": "exact", "steps": 4, "warmup": 1, "ms_per_step": 471.23456789, "samples_per_s": 140812345.678}
    line = json.dumps(b.headline(detail))
    assert len(line) <= 4096
    h = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in h, k
    assert h["config"]["workload"].startswith("C3")
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_ms"):
        assert k in h["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in h["cpu_baseline"], k
    assert h["value_exact"]["flavour"] == "exact"
    assert set(h["secondary"]) == {"example", "scan"}
    assert abs(h["value"] - detail["value"]) / detail["value"] < 1e-4  # rounding to 5 digits only


def test_shade_is_priced_against_the_guides_vector_peak():
    b = _bench()
    assert b.VALU_PEAK_GINST == 1228.8 and b.VALU_MEASURED_FMA_GINST == 614.4


def test_dump_outputs_are_the_frame_moments_in_frame_order(tmp_path):
    """--dump-outputs writes the planar accumulators as [3, H, W] and [H, W] float32, scattered back to frame order when the paths took the
    pixels in another order (--pixel-tile)."""
    import numpy as np
    import torch
    b = _bench()
    w, h = 40, 24
    fm = torch.arange(3 * w * h, dtype=torch.float32)
    sm = torch.arange(w * h, dtype=torch.float32) * 0.5
    b.dump_outputs(str(tmp_path / "rows"), fm, sm, None, w, h)
    first, second = np.load(tmp_path / "rows" / "first_moment.npy"), np.load(tmp_path / "rows" / "second_moment.npy")
    assert first.dtype == np.float32 and first.shape == (3, h, w) and second.shape == (h, w)
    assert np.array_equal(first.reshape(3, -1), fm.view(3, -1).numpy()) and np.array_equal(second.reshape(-1), sm.numpy())
    order = np.random.default_rng(3).permutation(w * h).astype(np.uint32)
    idx = torch.from_numpy(order.astype(np.int64))
    b.dump_outputs(str(tmp_path / "tiles"), fm.view(3, -1)[:, idx].reshape(-1), sm[idx], order, w, h)
    assert np.array_equal(np.load(tmp_path / "tiles" / "first_moment.npy"), first)
    assert np.array_equal(np.load(tmp_path / "tiles" / "second_moment.npy"), second)


def test_dump_outputs_of_a_large_frame_are_a_fixed_sample_within_the_limit(tmp_path, monkeypatch):
    """Above the size limit the same seeded pixel sample is written every time, with the pixels' frame indices."""
    import numpy as np
    import torch
    b = _bench()
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 200_000)
    w, h = 160, 100  # 16 bytes per pixel: 256 KB in full
    fm, sm = torch.rand(3 * w * h), torch.rand(w * h)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), fm, sm, None, w, h)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["first_moment.npy", "sample_pixels.npy", "second_moment.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 200_000
    idx = np.load(tmp_path / "a" / "sample_pixels.npy")
    assert idx.dtype == np.float64 and np.array_equal(idx, np.load(tmp_path / "b" / "sample_pixels.npy"))
    px = idx.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "first_moment.npy"), fm.view(3, -1).numpy()[:, px])
    assert np.array_equal(np.load(tmp_path / "a" / "second_moment.npy"), sm.numpy()[px])


def _run_bench(args, env=None, timeout=600):
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_times_the_headline_alone_and_dumps_what_it_computed(tmp_path):
    """A plain run prints the contract's fields for exactly --steps timed steps and nothing of --full; --dump-outputs holds the accumulators a caller
    of the same steps receives (warm-up and timed steps, 4 sample ids each, on a fresh context)."""
    import numpy as np
    from luminary_amd import scenes
    from luminary_amd.core import Core
    w, h, spp, warmup, steps = 96, 64, 4, 1, 2
    out = _run_bench(["--gpus", "1", "--workload", "cornell", "--width", str(w), "--height", str(h), "--samples-per-pass", str(spp), "--flavour", "exact",
                      "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "out")])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == steps and out["warmup"] == warmup and out["ms_per_step"] > 0 and out["value"] > 0
    for k in ("secondary", "cpu_baseline", "value_exact", "detail"):
        assert k not in out, k
    first, second = np.load(tmp_path / "out" / "first_moment.npy"), np.load(tmp_path / "out" / "second_moment.npy")
    assert first.dtype == np.float32 and first.shape == (3, h, w) and second.shape == (h, w)
    host = scenes.cornell_host(str(tmp_path / "scene"), w, h, 8)
    core = Core(0)
    core.set_flavour("exact")
    core.upload(host.device_scene())
    core.set_pixels(None)
    for i in range(warmup + steps):
        core.render(i * spp, spp, spp)
    fm, sm = core.accumulators()
    assert first.sum() > 0
    assert np.array_equal(first.reshape(3, -1), fm) and np.array_equal(second.reshape(-1), sm)


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements_and_the_record():
    """--full keeps what a plain run leaves out: the bit-exact flavour's value, the CPU baseline, the secondaries, and the full record on disk."""
    env = dict(os.environ)
    env.pop("LUM_FLAVOUR", None)  # the bench's own default (fast), so that value_exact is measured
    out = _run_bench(["--gpus", "1", "--workload", "cornell", "--width", "96", "--height", "64", "--samples-per-pass", "4", "--steps", "1", "--warmup", "1",
                      "--full", "--secondary", "example", "--secondary-steps", "1", "--exact-steps", "1", "--cpu-budget", "0.5"], env=env)
    assert out["steps"] == 1 and out["value"] > 0
    assert out["value_exact"]["flavour"] == "exact" and out["value_exact"]["value"] > 0
    assert out["cpu_baseline"]["value"] > 0
    assert set(out["secondary"]) == {"example"}
    b = _bench()
    assert out["detail"] == b.DETAIL_FILE
    with open(os.path.join(ROOT, b.DETAIL_FILE)) as f:
        detail = json.load(f)
    assert detail["secondary"]["example"]["steps"] == 1 and detail["config"]["output_chain_rank0"] is not None
