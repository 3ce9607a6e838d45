"""GPU: a plain `bench.py` run (no --full) measures the headline and nothing else: one JSON line with the headline fields,
exactly --steps timed steps, the last step's outputs under --dump-outputs, and none of the figures that --full adds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("roofline_builder", "h2d_overlapped", "config2_bf16_input_gemm", "p1_single_call", "p2_bigru", "hipgraph",
             "hp_builder", "file_path", "cpu_baseline")


@pytest.mark.timeout(600)
def test_plain_run_is_headline_only(tmp_path):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "GROUP_RANK", "LOCAL_WORLD_SIZE")}
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "16", "--warmup", "0", "--dump-outputs", str(dump)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=580)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["unit"] == "windows/s" and out["higher_is_better"] is True and out["dtype"] == "f32" and out["metric"]
    assert out["steps"] == out["timed_steps"] == 16 and out["warmup"] == 0 and out["full"] is False
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["ms_per_step"] * 16 - out["timed_seconds"] * 1e3) < 1e-6 * out["timed_seconds"] * 1e3
    assert abs(out["value"] - 16 * 512 / out["timed_seconds"]) < 1e-6 * out["value"]
    assert not [k for k in FULL_ONLY if k in out], sorted(out)
    assert sorted(out["kernel_ms"]) == ["k_lstm_layer_dec"]
    images, probs = np.load(str(dump / "images.npy")), np.load(str(dump / "probs.npy"))
    assert images.shape == (512, 33, 26) and probs.shape == (512, 3)
    assert np.allclose(probs.sum(axis=1), 1.0, atol=1e-4)
    for name in ("region", "position", "depth", "cand_freq"):
        assert np.load(str(dump / (name + ".npy"))).shape[0] == 512, name
