"""bench.py at N = 1 in its two forms: a plain run does only what the headline figure needs (set-up, warm-up, the timed steps,
--dump-outputs, the line); `--full` adds the other arithmetic, parity_in_run and the rocm-smi samples (and, not exercised here, the
CPU baseline and the `configs` block)."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "roofline", "config")
FULL_ONLY_KEYS = ("cpu_baseline", "configs", "parity_in_run", "value_fp32", "ms_per_step_fp32", "roofline_fp32", "device_sample",
                  "device_sample_under_load", "kernel_breakdown")


def _line(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--clips", "8", *args],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_carries_the_headline_and_nothing_else():
    with tempfile.TemporaryDirectory() as tmp:
        out = _line(["--dump-outputs", tmp])
        mask = np.load(os.path.join(tmp, "peak_mask.npy"))
        npeaks = np.load(os.path.join(tmp, "npeaks.npy"))
    assert all(k in out for k in HEADLINE_KEYS), sorted(set(HEADLINE_KEYS) - set(out))
    assert not any(k in out for k in FULL_ONLY_KEYS), sorted(set(FULL_ONLY_KEYS) & set(out))
    assert out["n_gpus"] == 1 and out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0 and out["higher_is_better"]
    assert out["metric"] == "8s/8kHz clips/sec (STFT+UNet+peak-pick)" and out["unit"] == "clips/s" and out["dtype"].startswith("bf16x3")
    assert abs(out["value"] - 8 * 1e3 / out["ms_per_step"]) < 0.01 * out["value"]
    assert out["roofline"]["launches"] > 0 and out["roofline"]["kernel_ms_per_step"] > 0
    assert mask.shape == (8, 256, 251) and npeaks.shape == (8,)
    assert int(out["config"]["peaks_last_step_rank0"]) == int(npeaks.sum()) == int(mask.sum())


def test_full_run_adds_the_extras():
    out = _line(["--full", "--cpu-seconds", "0", "--no-configs"])
    assert all(k in out for k in HEADLINE_KEYS), sorted(set(HEADLINE_KEYS) - set(out))
    assert out["parity_in_run"]["rel_l1_bf16x3_vs_fp32"] <= 1e-4
    assert out["value_fp32"] > 0 and out["ms_per_step_fp32"] > 0 and out["roofline_fp32"]["launches"] > 0
    assert "device_sample" in out and "cpu_baseline" not in out and "configs" not in out
