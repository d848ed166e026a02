"""CPU: the Q16 pose arithmetic of the world map's ray walks, the localiser and the MPPI controller (csrc/kc_q16.h: the
clamp, mix64, the step key, the draw, the noise, the motion step, the beam direction, the weight table's entry) against
the Python statements of the rules, tests/worldmap_mcl_ref.py and tests/mppi_ref.py.  tests/native/q16.cpp prints the
header's results for a fixed list of cases, a line a case with its inputs; every expected value here is formed from the
inputs by the Python statements, none by the header.  The header has no HIP include."""
import shutil
import subprocess
from pathlib import Path

import pytest

import mppi_ref
import worldmap_mcl_ref as mref
from worldmap_ref import MAX_OFFSET

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "q16.cpp"
INC = ROOT / "kompass-core_amd" / "csrc"
B = 1 << 36
M64 = (1 << 64) - 1


def rule22(cq, sq, ac, as_):
    """DESIGN.md 4.11 rule 22 as tests/worldmap_scan_ref.py has it inside its walk"""
    return (cq * ac - sq * as_ + (1 << 15)) >> 16, (sq * ac + cq * as_ + (1 << 15)) >> 16


def expected(name, a):
    """The results of case `name` with the integer inputs a, as a list"""
    if name == "bound":
        return [MAX_OFFSET]
    if name == "mix64":
        return [mref.mix64(a[0])]
    if name == "draw":
        return [mref.draw(*a)]
    if name == "mppi_draw":   # rule 3 as mppi_ref.sample has it
        seed, step, k, t, c = a
        return [mref.mix64(mppi_ref.sample_key(seed, step) ^ ((k << 8) | (3 * t + c)))]
    if name == "noise":
        return [mref.noise(*a)]
    if name == "clamp":
        return [mref.clamp(a[0])]
    if name == "move":        # 4.12 rule 4, which is 4.11 rule 31's: (C, S) must be the table's entry h
        h, C, S, tx, ty, F, L = a
        assert mref.headings()[h] == (C, S)
        x, y, h1 = mppi_ref.advance(tx, ty, h, F, L, 0)
        assert h1 == h
        return [x, y]
    if name == "turn":
        cq, sq, ac, as_ = a
        dx, dy = rule22(cq, sq, ac, as_)
        if (cq, sq) in AXES:  # the same rotation through the motion step of a pose at the origin: far inside the clamp
            assert mppi_ref.advance(0, 0, AXES[(cq, sq)], ac, as_, 0)[:2] == (dx, dy)
        return [dx, dy]
    if name == "weight_bin":  # rule 36 through record_of: a table that holds its own index
        v, vmin, w_shift, EW = a
        return [mref.record_of([0, 0], [0, 0], [0, 0], [vmin, v], range(EW), w_shift, 0)[1][1]]
    raise AssertionError(f"unknown case {name}")


AXES = {(65536, 0): 0, (0, 65536): 16384, (-65536, 0): 32768, (0, -65536): 49152}
N_IN = {"bound": 0, "mix64": 1, "draw": 4, "mppi_draw": 5, "noise": 2, "clamp": 1, "move": 7, "turn": 4, "weight_bin": 4}

# the cases that must be among the printed ones, by name and inputs
REQUIRED = [
    ("bound", ()), ("mix64", (0,)), ("draw", (5, 3, 7, 2)),
    ("noise", (0, 1000)), ("noise", (M64, 1000)),                   # the two extremes of g
    ("noise", (0, 0)), ("noise", (M64, 0)), ("noise", (0, 2 ** 31 - 1)), ("noise", (M64, 2 ** 31 - 1)),
    ("noise", (1, 3)),                                              # g = -131069: -393207 is no multiple of 65536
    ("clamp", (B,)), ("clamp", (-B,)), ("clamp", (B + 1,)), ("clamp", (-B - 1,)),
    ("move", (40000, -50404, -41886, 123456789, -987654321, 70000, -30000)),  # C and S negative
    ("move", (0, 65536, 0, 1000, -1000, 12345, -54321)),
    ("move", (0, 65536, 0, B - 100, -B + 50, 100, -50)),            # lands exactly on the bound
    ("move", (0, 65536, 0, B - 100, -B + 50, 101, -51)),            # would pass it
    ("turn", (65536, 0, 759250125, 759250125)), ("turn", (-65536, 0, 759250125, 759250125)),
    ("turn", (0, 65536, 759250125, 759250125)), ("turn", (0, -65536, 759250125, 759250125)),
    ("turn", (32768, 0, 3, -3)),                                    # both products round at exactly half
    ("mppi_draw", (0x0123456789ABCDEF, 77, 65535, 63, 2)),
]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = tmp_path_factory.mktemp("q16") / "q16"
    p = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{INC}", str(SRC), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert p.stderr == "", p.stderr   # -Wall stays quiet
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = []
    for line in r.stdout.splitlines():
        name, *nums = line.split()
        nums = [int(v) for v in nums]
        out.append((name, tuple(nums[:N_IN[name]]), nums[N_IN[name]:]))
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_q16_header_matches_the_python_statements(lines):
    assert len(lines) > len(REQUIRED)
    for name, a, got in lines:
        assert got == expected(name, a), (name, a)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_q16_cases_cover_the_edges(lines):
    printed = {(name, a) for name, a, _ in lines}
    for case in REQUIRED:
        assert case in printed, case
    got = {(name, a): r for name, a, r in lines}
    # known answers, so that the two sides cannot agree on a wrong rule
    assert got[("mix64", (0,))] == [0xE220A8397B1DCDAF]
    assert got[("draw", (5, 3, 7, 2))] == [mref.mix64(mref.mix64(5 ^ (3 << 32)) ^ ((7 << 8) | 2))]
    assert got[("noise", (0, 1000))] == [-2000] and got[("noise", (M64, 1000))] == [2000]
    assert got[("noise", (1, 3))] == [-6]                          # floor(-393207 / 65536 + 1 / 2)
    assert got[("clamp", (B + 1,))] == [B] and got[("clamp", (-B - 1,))] == [-B]
    assert got[("move", (0, 65536, 0, B - 100, -B + 50, 100, -50))] == [B, -B]
    assert got[("move", (0, 65536, 0, B - 100, -B + 50, 101, -51))] == [B, -B]
    assert got[("turn", (32768, 0, 3, -3))] == [2, -1]             # 1.5 -> 2, -1.5 -> -1: half goes up
