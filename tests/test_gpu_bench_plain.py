"""bench.py without --full: the record of the timed steps and nothing else measured; --dump-outputs writes what the last
timed step computed, the same from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _bench(args, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, "stdout must carry exactly one line, the record"
    return json.loads(lines[0])


def test_plain_solve_run_records_its_steps_and_dumps_the_last_solution(tmp_path):
    recs, xs = [], []
    for k in range(2):
        out = tmp_path / ("run%d" % k)
        rec = _bench(["--gpus", "1", "--ncell", "20", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in rec, key
        assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["higher_is_better"] is True and rec["dtype"] == "f64"
        assert abs(rec["value"] * rec["ms_per_step"] - 1e3) < 1e-6 * 1e3     # one timed step = one solve
        for key in ("roofline", "cpu_baseline", "alt", "dropin", "extra", "multi_gpu"):
            assert key not in rec, key                                        # measured with --full only
        x = np.load(out / "x.npy")
        info = np.load(out / "solve_info.npy")
        assert x.dtype == np.float64 and x.shape == (20 ** 3,) and np.all(np.isfinite(x)) and np.abs(x).max() > 0
        assert info.dtype == np.float64 and info.shape == (4,)
        assert info[0] == rec["config"]["iterations"] and info[2] == 1 == rec["config"]["converged"] and info[3] < 1e-8
        recs.append(rec)
        xs.append(x)
    assert recs[0]["config"]["iterations"] == recs[1]["config"]["iterations"]
    assert np.linalg.norm(xs[0] - xs[1]) <= 1e-8 * np.linalg.norm(xs[0])


def test_step_workload_dumps_the_particle_state(tmp_path):
    out = tmp_path / "step"
    rec = _bench(["--workload", "step", "--ncell", "20", "--kernel", "wendland", "--steps", "1", "--warmup", "0",
                  "--dump-outputs", str(out)])
    assert rec["unit"] == "steps/s" and rec["steps"] == 1
    x, v, p = (np.load(out / (k + ".npy")) for k in ("x", "v", "p"))
    assert x.shape == (20 ** 3, 3) and v.shape == (20 ** 3, 3) and p.shape == (20 ** 3,)
    assert all(a.dtype == np.float64 and np.all(np.isfinite(a)) for a in (x, v, p))
    ke = 0.5 * float((v * v).sum())
    assert abs(ke - rec["config"]["kinetic_energy_sum_end"]) <= 1e-12 * ke
