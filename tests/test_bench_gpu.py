"""bench.py's contract: one JSON result line whose ``steps`` / ``ms_per_step`` describe the timed updates, and
``--dump-outputs DIR`` leaving what the last timed update produced as float32 ``.npy`` files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_result_line_and_dumped_outputs(cuda, tmp_path):
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(d)], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert res["unit"] == "env-steps/s" and res["higher_is_better"] is True and res["dtype"] == "bf16"
    assert res["config"]["engine"] == "native"
    # value and ms_per_step are the same measurement: 32 envs x 5 rollout steps per update
    assert abs(res["value"] - 160 * 1000.0 / res["ms_per_step"]) <= 1e-3 * res["value"]
    got = {f[:-4]: np.load(str(d / f)) for f in sorted(os.listdir(str(d)))}
    assert set(got) == {"params", "stats", "actions", "rewards", "dones", "values"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got["actions"].shape == (5, 32) and got["values"].shape == (6, 32)
    assert got["params"].size > 1_600_000 and np.abs(got["params"]).max() > 0
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
