"""bench.py's command line: a plain run prints the headline line only (no
roofline, extras or CPU baseline: those are behind --full), --steps sets the
number of timed steps, and --dump-outputs writes the loss triple the last
timed step returned."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent


def test_plain_run_line_and_dump(device, tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1
    assert d["unit"] == "pairs/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: pairs per step over the step time
    pairs = 1024 * 1024 + 1024 * 16
    assert d["value"] == pytest.approx(pairs / (d["ms_per_step"] * 1e-3), rel=1e-9)
    for moved in ("roofline", "extras", "cpu_baseline", "vs_cpu_baseline_same_box"):
        assert moved not in d, moved
    assert sorted(p.name for p in out.iterdir()) == ["loss.npy"]
    loss = np.load(out / "loss.npy")
    assert loss.dtype == np.float64 and loss.shape == (3,)
    assert np.all(np.isfinite(loss)) and np.all(loss > 0)
    assert loss[0] == d["config"]["final_loss"]
    # the mixed loss is 0.7 explicit + 0.3 in-batch, fp64 sums; the two weights reach
    # the kernel as fp32 (6e-8 relative rounding each), hence 1e-6
    assert loss[0] == pytest.approx(0.7 * loss[1] + 0.3 * loss[2], rel=1e-6)
