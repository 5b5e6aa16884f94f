"""bench.py on the GPU at a small shape: a plain run times exactly --steps steps, prints the headline fields, and
--dump-outputs writes the last timed step's outputs, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--size", "128"]


def _bench(dump):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + ["--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return lines[0]


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_same_outputs_twice(gpu_device, tmp_path):
    line = _bench(tmp_path / "a")
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "images/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["ms_per_step"] > 0
    assert abs(line["value"] - 2 * 1e3 / line["ms_per_step"]) <= 0.01 * line["value"]
    assert line["roofline"] is None and line["cpu_baseline"] is None
    assert not {"sustained", "other_configs", "roofline_ops", "math_accuracy_check"} & set(line)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(n + ".npy" for n in ("cls_prob", "loc_loss", "cls_target", "det_out", "seg_out", "weights_sample"))
    total = 0
    for n in names:
        a = np.load(tmp_path / "a" / n)
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), n
        total += a.nbytes
    assert total <= 64 << 20
    _bench(tmp_path / "b")
    for n in names:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n), err_msg=n)
