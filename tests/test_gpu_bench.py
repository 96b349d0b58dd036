"""bench.py end to end on a small cloud: a plain run is the timed steps and its line, nothing else; --full adds what it
names (box record, stage times, roofline, CPU baseline, end-to-end leg) on the same timed steps."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--points", "3000000", "--full-line", *extra]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_is_lean_and_full_adds_the_rest():
    plain = _record()
    for k, v in (("metric", "octree-build Mpoints/sec"), ("unit", "Mpoints/s"), ("higher_is_better", True), ("dtype", "f64"),
                 ("steps", 2), ("warmup", 1)):
        assert plain[k] == v, k
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["config"]["nodes"] > 0
    assert len(plain["wall_ms_each_step"]) == 2 and plain["kernel_ms_per_step"]
    for k in ("roofline", "encode_sort", "cpu_baseline", "parity", "end_to_end", "stage_ms", "query", "config5", "sharded",
              "intensity", "config1"):
        assert plain[k] is None, k
    assert plain["config"]["box"] is None

    full = _record("--full", "--cpu-sample", "1000000")
    assert full["value"] > 0 and full["config"]["nodes"] == plain["config"]["nodes"]
    assert set(full["config"]["box"]) == {"idle_before_warmup", "right_after_timed_region"}
    assert full["stage_ms"] and full["roofline"]["kernel"] and full["encode_sort"]["ms"] > 0
    assert full["cpu_baseline"]["value"] > 0 and full["end_to_end"]["files"] > 0
