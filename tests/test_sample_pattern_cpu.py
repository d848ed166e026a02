"""CPU: the sample-pattern rule of the DWA host path (csrc/kc_sample_pattern.h: which pattern's tables are active, which
are kept, which slot a pattern is put away into) and the two walking orders (counting sort by trig row, rectangular and
ragged deal) against sequences and lists worked out by hand (tests/native/sample_pattern.cpp).  The header has no HIP
include."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "sample_pattern.cpp"
INC = ROOT / "kompass-core_amd" / "csrc"


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pattern_rule_and_walking_orders(tmp_path):
    exe = tmp_path / "sample_pattern"
    p = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{INC}", str(SRC), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 bad" in r.stdout
