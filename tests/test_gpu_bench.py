"""GPU test (-m gpu) of bench.py's plain run: the headline line without the --full sections, and --dump-outputs, whose arrays are the
same from run to run (seeded inputs).  bench.py runs as a fresh CHILD process (subprocess)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def _plain(dump, steps):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", "1024", "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_run_and_dumped_outputs(tmp_path):
    a = _plain(tmp_path / "a", 3)
    b = _plain(tmp_path / "b", 5)
    for line, steps in ((a, 3), (b, 5)):
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "evals/s" and line["dtype"] == "f64"
        assert "cpu_baseline" not in line and "secondary" not in line and line["roofline"]["measured_fma_ceiling_tflops"] is None
    la, lb = np.load(tmp_path / "a" / "logl.npy"), np.load(tmp_path / "b" / "logl.npy")
    sa, sb = np.load(tmp_path / "a" / "status.npy"), np.load(tmp_path / "b" / "status.npy")
    assert la.shape == (1024,) and la.dtype == np.float64 and sa.shape == (1024,) and sa.dtype == np.float64
    assert np.array_equal(la, lb, equal_nan=True) and np.array_equal(sa, sb)
    ok = sa == 0
    assert ok.mean() == a["status_ok_frac"] and np.isfinite(la[ok]).all()
