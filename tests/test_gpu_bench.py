"""bench.py as the driver runs it (one GPU): the plain run's line and --dump-outputs.

A plain run (`--gpus 1 --steps K --warmup W`) prints one line with the headline fields and none of the
`--full` extras; `--dump-outputs DIR` writes what the last timed step returned, and two runs with the same
arguments see the same inputs, so they write the same arrays: the simulator's per-particle outputs are a pure
function of (z0, seed, counter, particle id) and must agree bit for bit; the moment sums and what the residual
forms from them are reduced in a fixed order, so they agree bit for bit too.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NSTEPS, K, W = 8192, 10, 3, 1


def _bench(extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup",
                        str(W), "--particles", str(N), "--n-steps", str(NSTEPS)] + extra,
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_line_and_dump_outputs(native, tmp_path):
    outs = []
    for k in ("a", "b"):
        line = _bench(["--dump-outputs", str(tmp_path / k)])
        outs.append({f[:-4]: np.load(tmp_path / k / f) for f in sorted(os.listdir(tmp_path / k))})
    assert line["steps"] == K and line["warmup"] == W and line["n_gpus"] == 1
    assert line["unit"] == "particle-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] / 1e3 - N * (NSTEPS + 1)) < 1e-6 * line["value"]
    assert line["roofline"]["kernel_launches_timed"] == K
    for key in ("cpu_baseline", "cpu_baseline_1core", "cpu_baseline_c1", "gpu_over_cpu", "drift_err"):
        assert key not in line, key  # --full only
    assert "box_write_ceiling_GBps" not in line["roofline"]
    a, b = outs
    assert sorted(a) == ["last", "moments", "moments_local", "particle_ids", "residual_grad", "residual_out", "tau",
                         "traj"]
    assert a["traj"].shape == (NSTEPS, 4096, 8) and a["tau"].shape == (NSTEPS, 4096) and a["last"].shape == (4096, 8)
    assert a["residual_grad"].shape == (20,) and a["moments"].shape == (3, 45)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for name, v in a.items():
        assert v.dtype in (np.float32, np.float64) and np.isfinite(v).all(), name
        assert np.array_equal(v, b[name]), name
    # the dump is the last timed step's output: its loss is the line's loss
    assert float(a["residual_out"].ravel()[0]) == pytest.approx(line["loss"], rel=1e-6)
