"""The contract of `python bench.py` at N = 1 (the command the driver runs): ONE JSON line with the metric and the whole-job value;
with `--full` also the `roofline` object of the dominant kernel class and the `cpu_baseline` object -- checked on short runs (few
steps, small CPU budget; the numbers are not asserted, their consistency is)."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_single_gpu_bench_line_contract():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "4", "--warmup", "2", "--full", "--no-train", "--cpu-budget-s", "3"],
                       capture_output=True, text=True, timeout=900, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["unit"] == "steps/s" and d["dtype"] == "bf16" and d["data"] == "synthetic" and d["scaling"] == "weak"
    assert d["vs_baseline"] is None                                   # BASELINE.md publishes no number for this metric
    assert abs(d["value"] * d["ms_per_step"] - 1e3) < 1.0             # one sample: steps/s = 1000 / ms per step
    assert "workload" in d["config"] and "model" not in d["config"]
    rf = d["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and rf["peak"] == 2500.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and 0.05 < rf["frac"] < 1.0
    assert abs(rf["achieved"] - rf["algorithmic_gflop_per_launch"] / rf["avg_launch_us"] * 1e3) < 0.02 * rf["achieved"]
    # traffic: the PMC figure of THIS build (profiles/r03_pmc_traffic.json carries the library digest) or null with the reason
    assert ("traffic" in rf) and (rf["traffic"] is None and "traffic_note" in rf or rf["traffic"] > rf["algorithmic_bytes_per_launch"] * 0.5)
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "steps/s" and cb["cores"] >= 1 and 0 < cb["value"] < d["value"] and cb["sample"]


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """a plain run (no --full) times exactly --steps steps and prints the headline only (the extras' keys are null);
    --dump-outputs writes the last timed step's x_prev / pred_x0 as float32 .npy files, and the same arguments give the same arrays (to reduction order)"""
    import numpy as np
    dumps = []
    for run in range(2):
        out = tmp_path / f"run{run}"
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs",
                            str(out)], capture_output=True, text=True, timeout=900, cwd=str(ROOT))
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, lines
        d = json.loads(lines[0])
        assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["dtype"] == "bf16" and d["unit"] == "steps/s"
        assert d["higher_is_better"] is True and abs(d["value"] * d["ms_per_step"] - 1e3) < 1.0
        assert d["roofline"] is None and d["cpu_baseline"] is None and d["end_to_end"] is None and d["train_step"] is None
        got = {n: np.load(out / f"{n}.npy") for n in ("x_prev", "pred_x0")}
        for a in got.values():
            assert a.dtype == np.float32 and a.shape == (1, 4, 10, 32, 32) and np.isfinite(a).all()
        dumps.append(got)
    for n in dumps[0]:          # same seeded inputs and weights: the same result up to the order of floating-point reductions
        a, b = dumps[0][n].astype(np.float64), dumps[1][n].astype(np.float64)
        assert np.linalg.norm(a - b) <= 1e-3 * np.linalg.norm(a), n
