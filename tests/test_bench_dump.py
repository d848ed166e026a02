"""`bench.py --dump-outputs DIR`: what the timed controller cycle returned in its last step, as DIR/<name>.npy
(float32 / float64), identical from run to run with the same arguments; `--steps` is the number of timed steps."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
RECORD = ("found", "cost", "index", "raw_index", "n_admissible", "n_samples")
BEST = ("best_path_x", "best_path_y", "best_vx", "best_vy", "best_omega")


def _bench(*extra):
    e = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "KC_BENCH_FORCE_DIST"):
        e.pop(k, None)
    return subprocess.run([sys.executable, str(ROOT / "bench.py"), *extra], capture_output=True, text=True,
                          timeout=280, env=e)


@pytest.mark.parametrize("extra", [["--steps", "0"], ["--mapper", "--dump-outputs", "unused"],
                                   ["--ref", "cost5k", "--dump-outputs", "unused"]])
def test_arguments_the_dump_cannot_serve_are_refused(extra, tmp_path):
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), *extra], capture_output=True, text=True,
                       timeout=120, cwd=tmp_path)
    assert p.returncode == 2 and "error:" in p.stderr, p.stderr[-400:]
    assert not (tmp_path / "unused").exists()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_dump_is_the_last_timed_cycle_and_repeats(tmp_path):
    runs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        p = _bench("--gpus", "1", "--steps", "7", "--warmup", "2", "--only-headline", "--no-cpu", "--dump-outputs", str(d))
        assert p.returncode == 0, p.stderr[-800:]
        out = json.loads([ln for ln in p.stdout.splitlines() if ln.strip()][-1])
        assert out["steps"] == 7 and out["warmup"] == 2
        runs.append((out, {f.stem: np.load(f) for f in sorted(d.glob("*.npy"))}))
    (out, a), (_, b) = runs
    assert sorted(a) == sorted(b)
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    assert set(RECORD) <= set(a)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    w = out["winner"]
    assert bool(a["found"]) == w["found"] and int(a["raw_index"]) == w["raw_index"]
    assert a["cost"].dtype == np.float32 and a["cost"] == np.float32(w["cost"])
    assert int(a["n_samples"]) == out["config"]["samples_per_gpu"]
    if w["found"]:
        P = out["config"]["points"]
        assert [a[n].shape for n in BEST] == [(P,), (P,), (P - 1,), (P - 1,), (P - 1,)]
        assert np.all(np.isfinite(a["best_path_x"])) and np.all(np.isfinite(a["best_path_y"]))
