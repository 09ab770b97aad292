"""bench.py's driver options on the CPU path: --steps sets the timed step
count, ms_per_step is reported, --full is accepted, and --dump-outputs writes
the last timed step's arrays as float32 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DUMP_BYTES = 64 * 1000 * 1000


def check_dump(dst, batch_size):
    names = sorted(os.listdir(dst))
    assert {"loss.npy", "logits.npy", "dense_params.npy"} <= set(names), names
    total = 0
    for n in names:
        assert n.endswith(".npy"), n
        a = np.load(os.path.join(dst, n))
        assert a.dtype in (np.float32, np.float64), (n, a.dtype)
        assert a.size > 0 and np.isfinite(a).all(), n
        total += a.nbytes
    assert total <= MAX_DUMP_BYTES, total
    assert np.load(os.path.join(dst, "loss.npy")).size == 1
    assert np.load(os.path.join(dst, "logits.npy")).size == batch_size


def test_bench_full_and_dump_outputs_cpu(tmp_path):
    dst = tmp_path / "out"
    out = subprocess.run(
        [
            sys.executable, os.path.join(REPO, "bench.py"),
            "--gpus", "1", "--steps", "4", "--warmup", "1",
            "--batch-size", "64", "--rows", "1e4", "--num-sparse", "4",
            "--dim", "16", "--device", "cpu", "--graph", "0",
            "--full", "--dump-outputs", str(dst),
        ],
        capture_output=True, text=True, timeout=600, cwd=REPO,
    )
    assert out.returncode == 0, (out.stderr[-3000:], out.stdout[-500:])
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    res = json.loads(lines[0])
    assert res["steps"] == 4
    assert res["ms_per_step"] > 0
    assert abs(res["value"] * res["ms_per_step"] / 1000.0 - 64) < 1e-6 * 64
    for key in ("metric", "value", "unit", "higher_is_better", "dtype"):
        assert key in res
    check_dump(str(dst), batch_size=64)
