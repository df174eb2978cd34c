"""GPU test of bench.py's plain run and its --dump-outputs contract: one JSON result line with the headline fields,
--steps timed steps, and the outputs of the last timed step written as float32 .npy files that do not change from run
to run for the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps):
    # --nbuf 8 --streams 4: eight rotating batches, so that step 0 and step 8 use the same inputs and output buffers
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--nbuf", "8", "--streams", "4", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    return d, {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    d1, o1 = _bench(tmp_path / "a", 1)
    d9, o9 = _bench(tmp_path / "b", 9)
    for d, steps in ((d1, 1), (d9, 9)):
        assert d["steps"] == steps and d["warmup"] == 1 and d["n_gpus"] == 1
        assert d["unit"] == "snapshots/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["value"] > 0 and d["ms_per_step"] > 0
        assert abs(d["value"] * d["ms_per_step"] * 1e-3 - d["config"]["batch"]) <= 1e-6 * d["config"]["batch"]
        assert "roofline" not in d and "cpu_baseline" not in d and "other_configs" not in d   # --full only
    B, N, P, M = d1["config"]["batch"], d1["config"]["inputs"], d1["config"]["pspectrum_len"], d1["config"]["num_targets"]
    shapes = {"covariance": (B, N * N, 2), "spectrum": (B, P), "peak_values": (B, M), "peak_angles": (B, M)}
    assert {k: v.shape for k, v in o1.items()} == shapes
    assert all(v.dtype == np.float32 and np.all(np.isfinite(v)) for v in o1.values())
    assert sum(v.nbytes for v in o1.values()) <= 64 << 20
    assert np.all(o1["spectrum"].max(axis=1) == 0.0)              # the spectrum is normalised to its peak, in dB
    # step 0 of the 1-step run and step 8 of the 9-step run: the same seeded inputs, so the same outputs bit for bit
    for k in shapes:
        assert np.array_equal(o1[k], o9[k]), k
