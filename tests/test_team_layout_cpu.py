"""CPU: the team layout of the cycle kernel's cost phase (csrc/kc_team_layout.h: wavefronts per team and lanes per
trajectory point from the survivors of a workgroup and the trajectory length) against the stated rule, exhaustively
over R = 1..4 and P = 2..64 (tests/native/team_layout.cpp).  The header has no HIP include."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "team_layout.cpp"
INC = ROOT / "kompass-core_amd" / "csrc"


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_team_layout_matches_the_stated_rule(tmp_path):
    exe = tmp_path / "team_layout"
    p = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{INC}", str(SRC), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 bad" in r.stdout
