"""bench.py's command line: a plain run prints the headline line only, --dump-outputs writes the
last timed step's results, --full adds the side measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"}
FULL_ONLY_KEYS = {"roofline", "probed_ms_per_step", "fwd_embeddings_per_sec", "bf16", "f32_bf16x6", "roofline_gemm",
                  "hbm_kernels", "dvector_inference", "vendor_baseline", "dropin_loop", "cpu_baseline"}


def test_dump_sample_is_fixed_and_bounded():
    import bench
    small = torch.arange(10, dtype=torch.float64)
    assert bench._dump_sample(small).dtype == np.float32 and bench._dump_sample(small).tolist() == list(range(10))
    n = bench.DUMP_MAX_ELEMS + 1000
    big = torch.arange(n, dtype=torch.int32)
    a, b = bench._dump_sample(big), bench._dump_sample(big)
    assert a.shape == (bench.DUMP_MAX_ELEMS,) and a.dtype == np.float32
    assert np.array_equal(a, b) and np.all(np.diff(a) > 0) and a[-1] < n
    # the two arrays that can reach the cap (params, grads) stay well under the 64 MB a dump may take
    assert 2 * bench.DUMP_MAX_ELEMS * 4 <= 48e6


@pytest.mark.gpu
def test_plain_run_prints_headline_only_and_dumps_outputs(tmp_path):
    steps, warmup = 2, 1
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--N", "4", "--M", "5", "--T", "24", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert HEADLINE_KEYS <= set(res) and not FULL_ONLY_KEYS & set(res), sorted(res)
    assert res["steps"] == steps and res["warmup"] == warmup and res["dtype"] == "f32" and res["higher_is_better"] is True
    assert res["ms_per_step"] > 0
    assert abs(res["value"] - 20 / (res["ms_per_step"] * 1e-3)) <= 1e-3 * res["value"]
    # exactly one run of warmup + steps steps was logged: no probed or side runs
    assert r.stderr.count("] run N=") == 1 and f"steps={steps} warmup={warmup}" in r.stderr, r.stderr[-2000:]
    arrays = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(arrays) == {"loss", "params", "grads", "ge2e_wb", "ge2e_wb_grads"}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64e6
    assert abs(float(arrays["loss"][0]) - res["loss"]) <= 1e-5 * abs(res["loss"]) + 1e-5
    assert arrays["params"].shape == arrays["grads"].shape and arrays["params"].size > 1 << 20
    assert np.abs(arrays["grads"]).max() > 0 and arrays["ge2e_wb"].shape == (2,)
    # (w, b) moved from their initial (10, -5) by at most lr * clip per step
    assert 0 < np.abs(arrays["ge2e_wb"] - np.array([10.0, -5.0])).max() <= 0.01 * 1.0 * (steps + warmup) * 1.001
