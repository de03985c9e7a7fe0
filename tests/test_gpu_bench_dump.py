"""GPU: a plain `bench.py` run -- the headline leg alone -- and its --dump-outputs: the last timed step's outputs as float32 .npy files,
identical whatever the number of steps (the inputs depend on the arguments that shape them only)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(steps, out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--frames", "1",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_run_dumps_the_last_step(tmp_path):
    a, b = _run(2, tmp_path / "a"), _run(5, tmp_path / "b")
    for d, steps in ((a, 2), (b, 5)):
        assert d["steps"] == steps and d["ms_per_step"] > 0 and d["value"] > 0 and d["full"] is False
        for k in ("metric", "unit", "higher_is_better", "dtype"):
            assert k in d
        for leg in ("cpu_baseline", "shard_4k", "reference_workload", "encoder"):
            assert leg not in d, leg
    shapes = {"sad_8x8": (32400,), "satd_8x8": (32400,), "dct_32x32": (1980, 32, 32)}      # one 1080p frame
    for name, shape in shapes.items():
        x, y = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert x.dtype == np.float32 and x.shape == shape, (name, x.dtype, x.shape)
        np.testing.assert_array_equal(x, y, err_msg=name)
    sad, satd = np.load(tmp_path / "a" / "sad_8x8.npy"), np.load(tmp_path / "a" / "satd_8x8.npy")
    # ref = cur + noise in [-8, 8]: every 8x8 SAD lies in [0, 512], and the blocks differ
    assert sad.min() >= 0 and sad.max() <= 512 and sad.mean() > 64
    assert (satd > 0).mean() > 0.99
    assert np.abs(np.load(tmp_path / "a" / "dct_32x32.npy")).sum() > 0
