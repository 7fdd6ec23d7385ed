"""The plain benchmark run and --dump-outputs: the line holds the headline figure alone (what rides
along needs --full), --steps sets the number of timed steps, and the dumped verdicts of the last
timed step are the expected pattern of the seeded workload."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_float32_and_seeded_sample_past_the_budget(tmp_path, monkeypatch):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4096)
    small = np.arange(100, dtype=np.uint8) & 1
    big = np.arange(10000, dtype=np.uint8)
    for d in ("a", "b"):
        bench._dump_outputs(str(tmp_path / d), {"small": small, "big": big})
    a, b = tmp_path / "a", tmp_path / "b"
    assert sorted(os.listdir(a)) == ["big.npy", "big_index.npy", "small.npy"]
    s = np.load(a / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small.astype(np.float32))
    idx, v = np.load(a / "big_index.npy"), np.load(a / "big.npy")
    assert idx.dtype == np.float64 and v.dtype == np.float32 and v.nbytes + idx.nbytes <= 4096 // 2
    assert np.all(np.diff(idx) > 0) and np.array_equal(v, big[idx.astype(np.int64)].astype(np.float32))
    assert all(np.array_equal(np.load(a / f), np.load(b / f)) for f in os.listdir(a))   # the same sample each run


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    n, steps = 1 << 14, 3
    out_dir = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--log2-batch", "14", "--dump-outputs", str(out_dir)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.strip().splitlines() if l.strip()]
    assert lines and lines[-1].startswith("{") and sum(l.startswith("{") for l in lines) == 1, lines[-3:]
    d = json.loads(lines[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["unit"] == "verifies/s" and d["higher_is_better"] is True and d["steps"] == steps
    assert abs(d["value"] - n / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    for k in ("roofline", "double", "vargen", "rlc", "mixed", "cpu_baseline", "small_batch", "verify_batch_e2e"):
        assert k not in d, k
    assert sorted(os.listdir(out_dir)) == ["verdicts.npy"]
    v = np.load(out_dir / "verdicts.npy")
    assert v.dtype == np.float32 and v.shape == (n,)
    assert np.array_equal(v, (np.arange(n) % 16 != 0).astype(np.float32))   # every 16th item corrupted
