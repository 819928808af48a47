"""bench.py's driver contract on the GPU: one short N = 1 run as a child
process (the driver runs `python bench.py` the same way) must print exactly one
JSON line with the contract's fields and, with --full, a roofline object and a
passing check; a plain run prints the headline fields alone and --dump-outputs
writes the arrays its last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_contract_n1():
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--full",
           "--no-extra", "--no-cpu-baseline"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in out, k
    assert out["n_gpus"] == 1 and out["steps"] == 2 and out["warmup"] == 1
    assert out["unit"] == "holograms/s" and out["higher_is_better"] is True and out["scaling"] == "weak"
    assert out["dtype"] == "f32" and out["check"] == "ok" and out["value"] > 0
    assert "workload" in out["config"] and out["config"]["height"] == 1024 and out["config"]["iters"] == 200
    roof = out["roofline"]
    assert roof["bound"] == "hbm" and roof["unit"] == "GB/s" and roof["peak"] == 8000.0
    assert 0 < roof["frac"] < 1.5 and 0 < roof["frac_physical"] < 1
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    # the step is 200 iterations of two launches: the kernels fit inside it
    assert 200 * roof["avg_us"] * 1e-3 < out["ms_per_step"]
    print(f"[bench] N=1 short run: {out['value']:.1f} holograms/s, frac {roof['frac']:.3f}")


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_last_step(gpu, tmp_path):
    """A plain run measures the headline value only (none of the --full
    objects), and --dump-outputs writes the phases and error curves of its last
    timed step: bit for bit what the plan API gives for the same seeded targets."""
    sys.path.insert(0, ROOT)
    import bench

    b, n, iters = 3, 256, 20
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--size", str(n), "--batch-per-gpu", str(b), "--iters", str(iters), "--dump-outputs", str(tmp_path / "o")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "holograms/s" and out["dtype"] == "f32"
    assert out["higher_is_better"] is True and out["ms_per_step"] > 0
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 / b - 1) < 1e-3  # value = holograms per timed second
    for k in ("roofline", "check", "ranks", "extra", "parity", "cpu_baseline", "summary"):
        assert k not in out, k
    assert sorted(os.listdir(tmp_path / "o")) == ["error.npy", "phase.npy"]
    phase, err = np.load(tmp_path / "o" / "phase.npy"), np.load(tmp_path / "o" / "error.npy")
    assert phase.dtype == np.float32 and phase.shape == (b, n, n)
    assert err.dtype == np.float64 and err.shape == (b, iters)
    assert out["outputs"] == {"phase": {"shape": [b, n, n], "dtype": "float32"},
                              "error": {"shape": [b, iters], "dtype": "float64"}}
    with gpu.Plan(gpu.ALGO_GS, b, n, n, gpu.TGT_F32, False, iters) as p:
        p.set_target(bench.targets(0, b, n))
        p.run(iters)
        ref_phase, _, ref_stats, _ = p.read(expected=False, iters=False)
    np.testing.assert_array_equal(phase, ref_phase)
    np.testing.assert_array_equal(err, ref_stats[:, :iters, 3])
    assert np.ptp(phase) > 1 and (err[:, -1] < err[:, 0]).all()
