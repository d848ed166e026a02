"""CPU: the launch plans of the DWA host path (csrc/kc_launch_plan.h: samples per workgroup, tile and LDS bytes of the
roll-out, the dropped cycle, the sensor build's bands, sphere layers and bucket grid, the cost kernel choice, the yaw
range rule) against hand-derived expectations (tests/native/launch_plan.cpp).  The header has no HIP include."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "launch_plan.cpp"
INC = ROOT / "kompass-core_amd" / "csrc"


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_launch_plans_match_the_stated_rules(tmp_path):
    exe = tmp_path / "launch_plan"
    p = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", f"-I{INC}", str(SRC), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 bad" in r.stdout
