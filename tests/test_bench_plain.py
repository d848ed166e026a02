"""A plain `bench.py --gpus 1 --steps N --warmup W` does what its headline figure needs and nothing else: set-up,
warm-up, the timed steps, one JSON line.  `--full` adds the kernel timing pass with its roofline, the CPU baseline
and the legs beside the headline."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
LEGS = ("mid_density", "open_space", "laserscan_room", "extras", "fresh_inputs", "mapper_cfg4")
FULL_ONLY = ("kernels_ms", "host_phases_ms", "roofline", "cpu_baseline") + LEGS


def _bench(*extra):
    e = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "KC_BENCH_FORCE_DIST"):
        e.pop(k, None)
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "2", *extra],
                       capture_output=True, text=True, timeout=280, env=e)
    assert p.returncode == 0, p.stderr[-800:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_plain_run_is_the_headline_alone():
    out = _bench()
    assert set(HEADLINE) <= set(out)
    assert (out["metric"], out["unit"], out["higher_is_better"]) == ("trajectory-steps/s", "trajectory-steps/s", True)
    assert out["steps"] == 20 and out["warmup"] == 2
    cfg = out["config"]
    assert out["value"] == pytest.approx(cfg["global_samples"] * cfg["points"] / (out["ms_per_step"] * 1e-3), rel=1e-9)
    assert [k for k in FULL_ONLY if k in out] == []


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_full_run_adds_the_timing_pass_and_every_leg():
    out = _bench("--full", "--no-cpu")
    assert set(HEADLINE) <= set(out)
    assert out["kernels_ms"] and out["roofline"]["kernel"] in out["kernels_ms"]
    assert out["config"]["launches_per_cycle"] == len(out["kernels_ms"])
    assert set(LEGS) <= set(out) and "cpu_baseline" not in out
    assert out["mid_density"]["config"]["scene"] == "mid" and out["open_space"]["config"]["scene"] == "open"
