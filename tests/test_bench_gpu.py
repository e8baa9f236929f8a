"""bench.py as a command: a plain run (no --full) times exactly --steps steps, prints one line with ms_per_step and
none of the --full legs, and --dump-outputs writes the last step's arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_dumps_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--batch", "2", "--dump-outputs", str(tmp_path / "dump")], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert out.returncode == 0, out.stderr.decode()
    lines = [json.loads(ln) for ln in out.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "images/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["ms_per_step"] > 0
    # value = images per second of the timed steps: batch / (one step's seconds), up to the rounding of both fields
    np.testing.assert_allclose(line["value"], 2 * 1e3 / line["ms_per_step"], rtol=1e-2)
    for key in ("cpu_baseline", "peak_achievable", "class_rooflines", "exchange"):
        assert key not in line
    got = {f[:-4]: np.load(str(tmp_path / "dump" / f)) for f in os.listdir(str(tmp_path / "dump"))}
    assert {"loss", "grad", "param", "out0_heatmap", "out0_regr", "out0_offset"} <= set(got)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["out0_heatmap"].shape == (2, 1, 128, 128)
    assert got["param"].shape == got["grad"].shape and np.abs(got["grad"]).sum() > 0
    assert abs(float(got["loss"]) - line["final_loss"]) <= 1e-5 * max(1.0, abs(line["final_loss"]))
