"""GPU suite: a plain bench.py run - exactly --steps timed steps, the headline fields only, and --dump-outputs writing the
whole solve of its last step (checked against the oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
from gato_python_amd import synth                                   # noqa: E402
from oracle import gato_oracle as o                                 # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_times_its_steps_and_dumps_its_outputs(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["metric"] == "PCG iterations/s" and d["unit"] == "iterations/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 7 and d["timed_steps"] == 7 and d["warmup"] == 2
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 100) < 0.01             # 100 PCG iterations per step (6 digits each)
    assert "roofline" not in d and "cpu_baseline" not in d and "sweep" not in d
    lam, dz = np.load(out / "lambda.npy"), np.load(out / "dz.npy")
    s = synth.make_system(14, 7, 50, seed=0)
    lam_o, dz_o, _ = o.linsys_solve(*s.csr_args(), 14, 7, 50, 0.0, 100, s.rho, dtype=np.float64)
    assert lam.dtype == np.float64 and lam.shape == lam_o.shape and dz.shape == dz_o.shape
    assert np.abs(lam - lam_o).max() / np.abs(lam_o).max() < 1e-9
    assert np.abs(dz - dz_o).max() < 1e-8
