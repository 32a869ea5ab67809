"""GPU: bench.py's contract -- a plain run times exactly --steps steps and reports ms_per_step, and --dump-outputs writes
the last timed step's outputs as float .npy files that are identical from run to run (the inputs are seeded).  It runs
from a working directory it may not write to: the benchmark writes only where it is told to."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import helpers as H


def _bench(out_dir, cwd):
    r = subprocess.run([sys.executable, "-s", os.path.join(H.ROOT, "bench.py"), "--gpus", "1", "--steps", "7",
                        "--warmup", "3", "--dump-outputs", str(out_dir)],
                       cwd=str(cwd), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_bench_times_its_steps_and_dumps_the_same_outputs_twice(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ro = tmp_path / "read_only"
    ro.mkdir()
    ro.chmod(0o555)
    try:
        a, b = _bench(tmp_path / "a", ro), _bench(tmp_path / "b", ro)
        assert os.listdir(ro) == []
    finally:
        ro.chmod(0o755)
    for line in (a, b):
        assert line["steps"] == 7 and line["repeats"] == 1 and not line["full"]
        assert line["ms_per_step"] > 0 and line["unit"] == "steps/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f32" and "roofline" not in line and "cpu_baseline" not in line
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"td_error.npy", "params.npy", "priority.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), n
        assert np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
