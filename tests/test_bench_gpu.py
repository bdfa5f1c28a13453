"""A plain ``bench.py`` run on the GPU (small shape): it times exactly ``--steps`` graph replays, reports
only the headline figure's fields, and ``--dump-outputs`` writes the last step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(180)
def test_plain_run_is_lean_and_dumps_its_outputs(dev, tmp_path):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "2", "--seq-len", "256", "--dump-outputs", str(out)],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=170)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["n_gpus"] == 1 and res["dtype"] == "bf16" and res["higher_is_better"] is True
    assert res["unit"] == "feature-timesteps/sec" and res["ms_per_step"] > 0
    # value is the timed steps' throughput: B * T timesteps per ms_per_step
    assert abs(res["value"] - 2 * 256 / (res["ms_per_step"] * 1e-3)) <= 1e-6 * res["value"]
    assert res["execution"].startswith("hip-graph replay") and res["full"] is False
    for k in ("roofline", "cpu_baseline", "parity_mode", "fresh_batch", "param_checksums", "comm"):
        assert k not in res, k
    assert sorted(os.listdir(out)) == ["grads.npy", "loss.npy", "params.npy"]
    a = {k: np.load(out / (k + ".npy")) for k in ("loss", "params", "grads")}
    assert res["outputs"] == {k: list(v.shape) for k, v in a.items()}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert a["loss"][0] == np.float32(res["loss"]) and a["params"].shape == a["grads"].shape
    assert np.count_nonzero(a["grads"]) > 0 and np.count_nonzero(a["params"]) > 0
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 * 2 ** 20
