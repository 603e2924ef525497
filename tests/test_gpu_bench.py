"""bench.py's plain run: the headline line and the dumped outputs, nothing that takes time of its own (the CPU-oracle baseline
is behind --full).  Runs the benchmark as a child process at T = 2.  Needs a MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_prints_the_headline_line_and_dumps_without_the_cpu_baseline(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--T", "2", "--steps", "1", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline", "hbm"):
        assert k in d, k
    assert d["unit"] == "audio-sec/s" and d["dtype"] == "f32" and d["higher_is_better"] is True and d["value"] > 0
    assert d["steps"] == 1 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["output_finite"] is True
    assert "cpu_baseline" not in d
    arrays = d["dumped_outputs"]["arrays"]
    assert sorted(arrays) == ["filter_params", "restored_audio"]
    a = np.load(tmp_path / "restored_audio.npy")
    assert list(a.shape) == arrays["restored_audio"]["shape"] and np.isfinite(a).all()
