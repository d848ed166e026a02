"""Scenes, fills, poses and checks shared by tests/test_bayes_edges_cpu.py and tests/test_bayes_edges_gpu.py.  Not
collected by pytest.

The Bayesian update (LocalMapper::updateGridCellProbability, local_mapper.cpp:106-125) fed back scan after scan
leaves the interior of (0, 1) quickly: with the benchmark's sensor model the cells reach exactly 1.0f and 0.0f, with
the defaults they settle at nextafter(1, 0) and float(2^-52).  The scenes here drive the update and the warp
(getPreviousGridInCurrentPose, :17-78) there, and under previous values a caller can hand over: +-0, 1, the
neighbours of 1, subnormals, values outside [0, 1], +-inf and NaN.

Every oracle sequence is computed once per process (functools.lru_cache) and handed out read-only."""
from __future__ import annotations

import functools
import json
from pathlib import Path

import numpy as np

import mapper_ref as mr
from oracle import ko

F = np.float32
KEYS = ("p_prior", "p_occupied", "p_empty", "range_sure", "range_max", "wall_size")
# LocalMapper Bayesian ctor arguments of the reference benchmark (benchmark_runner.cpp:207-212) and the first
# ctor's defaults (local_mapper.h:22-24)
BENCH = dict(zip(KEYS, (0.6, 0.9, 0.1, 0.1, 20.0, 0.2)))
DEFAULT = dict(zip(KEYS, (0.5, 0.6, 0.4, 1.0, 20.0, 0.2)))
PARAM_SETS = {
    "bench": BENCH,
    "default": DEFAULT,
    "certain": dict(zip(KEYS, (0.5, 1.0, 0.0, 0.5, 2.0, 0.1))),
    "prior0": dict(zip(KEYS, (0.0, 0.7, 0.3, 0.3, 5.0, 0.0))),
    "prior1": dict(zip(KEYS, (1.0, 0.7, 0.3, 0.3, 5.0, 0.0))),
    "rangemax0": dict(zip(KEYS, (0.4, 0.7, 0.3, 0.3, 0.0, 0.2))),
    "negwall": dict(zip(KEYS, (0.4, 0.7, 0.3, 30.0, 1.0, -0.5))),
    "widewall": dict(zip(KEYS, (0.4, 0.8, 0.2, 0.05, 0.3, 5.0))),
}

ONE_BELOW = np.nextafter(F(1), F(0))             # 1 - 2^-24
TWO_M52 = F(2.0 ** -52)
SPECIAL = np.array([0.0, -0.0, 1.0, np.nextafter(F(1), F(0)), np.nextafter(F(1), F(2)), 1.4e-45, 1.1754942e-38,
                    1.1754944e-38, 2.220446e-16, 1e-30, 0.5, 0.6, 2.0, -0.25, 3.4e38, -3.4e38, np.inf, -np.inf,
                    np.nan, 0.99999], F)
GOLD = Path(__file__).parent / "golden"


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_prob(got, want, what=""):
    """The comparison of the new tests: where `want` is NaN, `got` must be NaN (the oracle's own NaNs come out with
    both signs on x86, the device gives the positive quiet NaN: any sign and payload pass); everywhere else the
    uint32 patterns must be identical, the sign of zero and subnormals included."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    bad = np.where(nan, ~np.isnan(got), bits(got) != bits(want))
    if bad.any():
        idx = np.argwhere(bad)
        first = [(tuple(int(v) for v in k), hex(int(bits(got)[tuple(k)])), hex(int(bits(want)[tuple(k)])))
                 for k in idx[:6]]
        raise AssertionError(f"{what}: {len(idx)} of {want.size} cells differ; (cell, got, want) {first}")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def caching_walker():
    """walker(s, ends, H, W) for mapper_ref.emissions that walks a set of lines once: the scans of a feedback loop
    repeat the same beams, only the previous grid changes."""
    memo = {}

    def run(s, ends, H, W):
        key = (tuple(int(v) for v in s), np.asarray(ends, np.int64).tobytes(), H, W)
        if key not in memo:
            memo[key] = mr.walk(s, ends, H, W)
        return memo[key]
    return run


def literal_scan(scene, prev, params, walker=None):
    """mapper_ref.scan_to_grid_baysian; the inputs here divide by zero and multiply inf by 0 on purpose."""
    H, W, res, pos, orient, ang, rng = scene
    with np.errstate(all="ignore"):
        return mr.scan_to_grid_baysian(H, W, res, pos, orient, ang, rng, prev, params, walker)


def literal_warp(prev, inv, prior):
    with np.errstate(all="ignore"):
        return mr.warp_previous(prev, inv, prior)


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------
def scene_a():
    a = np.linspace(-np.pi, np.pi, 360, endpoint=False)
    return 70, 66, 0.05, (0.1, -0.05, 0.0), 0.3, a, 1.0 + 0.3 * np.sin(3 * a)


def scene_b():
    a = np.linspace(-np.pi, np.pi, 300, endpoint=False)
    return 67, 45, 0.05, (0.1, -0.05, 0.0), 0.3, a, 0.9 + 0.5 * np.sin(5 * a) ** 2


SMALL_GRIDS = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 64), (65, 5)]


def small_scene(H, W):
    """64 beams of 0.3 m from the central cell: the cell pass's 64 x 4 workgroup is partly empty in both directions
    on these grids."""
    a = np.linspace(-np.pi, np.pi, 64, endpoint=False)
    return H, W, 0.05, (0.0, 0.0, 0.0), 0.0, a, np.full(64, 0.3)


def class_scene():
    """The 120 x 160 grid, fixture scan and sensor model of test_local_mapper_frontend_baysian's kompass_cpp part."""
    d = json.loads((GOLD / "laserscan_data.json").read_text())
    ang = d["angle_min"] + np.arange(len(d["ranges"])) * d["angle_increment"]
    rng = np.clip(np.nan_to_num(np.array(d["ranges"], float), posinf=d["range_max"]), 0, 20.0)
    return (120, 160, 0.05, (0.0, 0.0, 0.0), 0.0, ang, rng), dict(BENCH, wall_size=0.1)


def special_grid(H, W, count=len(SPECIAL)):
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return SPECIAL[(7 * i + 3 * j) % count].copy()


def seed_run2(H, W):
    vals = np.array([1e-12, 1e-14, 1e-15, 5e-16, 1 - 1e-5, 1 - 1e-6, 1 - 3e-7, 1 - 1.2e-7], F)
    return np.random.default_rng(1).choice(vals, (H, W))


def finite_fill(H, W):
    """uniform(0, 1), 20 % of the cells subnormal (1e-40), then 10 % at nextafter(1, 0)."""
    r = np.random.default_rng(100 * H + W)
    g = r.uniform(0, 1, (H, W)).astype(F)
    g[r.random((H, W)) < 0.2] = F(1e-40)
    g[r.random((H, W)) < 0.1] = ONE_BELOW
    return g


def oracle(scene, params):
    H, W, res, pos, orient, _, _ = scene
    return ko.BayesMapper(H, W, res, pos, orient, **params)


# ---------------------------------------------------------------------------
# 1. feedback loops on the oracle (computed once)
# ---------------------------------------------------------------------------
def _feedback(scene, params, steps, seed=None):
    o = oracle(scene, params)
    if seed is not None:
        o.set_previous(seed)
    out = []
    for _ in range(steps):
        g, p = o.scan_to_grid_baysian(scene[5], scene[6])
        out.append(_frozen(g, p))
        o.set_previous(p)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def run1():
    """Scene A, benchmark parameters, 20 scans fed back from the prior: ((grid, prob), ...)."""
    return _feedback(scene_a(), BENCH, 20)


def check_run1(steps):
    g, p = steps[-1]
    touched = g != -1
    zeros, ones = int((p[touched] == 0.0).sum()), int((p[touched] == 1.0).sum())
    assert zeros >= 400 and ones >= 200, (zeros, ones)
    assert np.array_equal(bits(steps[-2][1]), bits(p)), "cells still move between scans 19 and 20"
    assert not np.isnan(p).any()


@functools.lru_cache(maxsize=None)
def run2():
    """Scene A, default parameters, 12 scans fed back from seed_run2: (seed, ((grid, prob), ...))."""
    s = scene_a()
    seed = _frozen(seed_run2(s[0], s[1]))
    return seed, _feedback(s, DEFAULT, 12, seed)


def check_run2(steps):
    g, p = steps[-1]
    touched = g != -1
    hi, lo = int((p[touched] == ONE_BELOW).sum()), int((p[touched] == TWO_M52).sum())
    assert hi >= 100 and lo >= 150, (hi, lo)
    assert (bits(steps[-2][1]) != bits(p)).any(), "no cell changes in the last step"


@functools.lru_cache(maxsize=None)
def run3():
    """The class scene, 16 scans fed back from the prior."""
    scene, params = class_scene()
    return _feedback(scene, params, 16)


def check_run3(steps):
    g, p = steps[-1]
    touched = g != -1
    assert (p[touched] == 0.0).any() and (p[touched] == 1.0).any()


# ---------------------------------------------------------------------------
# 2. special previous values
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def special_scan(name):
    """Scene B over the special previous grid with one parameter set: (prev, grid, prob) of the oracle."""
    s = scene_b()
    prev = special_grid(s[0], s[1])
    o = oracle(s, PARAM_SETS[name])
    o.set_previous(prev)
    g, p = o.scan_to_grid_baysian(s[5], s[6])
    return _frozen(prev, g, p)


def check_special_scan(name, prev, g, p):
    touched = g != -1
    assert int(touched.sum()) == 1645
    H, W = g.shape
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    under = np.bincount(((7 * i + 3 * j) % len(SPECIAL))[touched], minlength=len(SPECIAL))
    assert under.min() >= 3, under
    nan = int(np.isnan(p[touched]).sum())
    assert 247 <= nan <= 1645, nan
    if name == "rangemax0":
        assert nan == 1645
    assert all(special_classes().values()), special_classes()


@functools.lru_cache(maxsize=None)
def special_classes():
    """Which kinds of value the oracle's touched cells hold over the eight parameter sets together."""
    seen = dict(nan=False, zero=False, one=False, negative=False, above_one=False)
    for name in PARAM_SETS:
        _, g, p = special_scan(name)
        v = p[g != -1]
        with np.errstate(invalid="ignore"):
            for key, hit in (("nan", np.isnan(v)), ("zero", v == 0), ("one", v == 1), ("negative", v < 0),
                             ("above_one", v > 1)):
                seen[key] |= bool(hit.any())
    return seen


@functools.lru_cache(maxsize=None)
def small_scan(H, W, name):
    s = small_scene(H, W)
    prev = special_grid(H, W, 10)
    o = oracle(s, PARAM_SETS[name])
    o.set_previous(prev)
    g, p = o.scan_to_grid_baysian(s[5], s[6])
    return _frozen(prev, g, p)


# ---------------------------------------------------------------------------
# 3. the warp
# ---------------------------------------------------------------------------
WARP_GRIDS = [(1, 1), (1, 9), (9, 1), (2, 2), (2, 7), (63, 65), (64, 64), (257, 3), (70, 66)]
WARP_RES = 0.05
FILLS = {"special": special_grid, "finite": finite_fill}


def warp_poses(r=WARP_RES):
    return [((0.0, 0.0), 0.0), ((3 * r, -2 * r), 0.0), ((-r, 4 * r), 0.0), ((0.0, 0.0), np.pi / 2),
            ((0.0, 0.0), -np.pi / 2), ((0.0, 0.0), np.pi), ((2 * r, r), np.pi / 2), ((0.0125, -0.0375), 0.0),
            ((0.31, -0.17), 0.4), ((0.0, 0.0), 1e-8), ((0.0, 0.0), np.nan), ((0.0, 0.0), np.inf),
            ((1e6, 0.0), 0.2), ((0.0, -5e7), 0.0),
            # two more whole-cell shifts (the offset is truncated: half a cell keeps it away from a rounding edge).
            # With theta = 0 the sources are x + 2 (c1 + k1) - H / 2 and y + 2 (c0 + k0) - W / 2 for a shift of
            # (k0, k1) cells: on 64 x 64 and 70 x 66 the poses above leave source 0 out on both axes, (-18, -16)
            # brings it in; on 2 x 2 the sources are odd offsets and only k = 1 makes W - 1 = H - 1 = 1 one of them
            ((-18.5 * r, -16.5 * r), 0.0), ((1.5 * r, 1.5 * r), 0.0)]


WHOLE_SHIFTS = (0, 1, 2, 14, 15)  # the poses with theta = 0 and whole-cell shifts
PRIOR_ONLY = (10, 11, 12, 13)     # non-finite angles, poses far away: nothing of the previous grid is inside


def warp_oracle(H, W):
    return ko.BayesMapper(H, W, WARP_RES, (0, 0, 0), 0.0, **BENCH)


@functools.lru_cache(maxsize=None)
def warp_single(H, W, fill):
    """Every pose on a fresh previous grid: (prev, ((inv, warped), ...)) of the oracle."""
    prev = _frozen(FILLS[fill](H, W))
    o = warp_oracle(H, W)
    out = []
    for pos, th in warp_poses():
        o.set_previous(prev)
        inv = o.warp_matrix(pos, th)
        out.append(_frozen(inv, o.get_previous_grid_in_current_pose(pos, th)))
    return prev, tuple(out)


@functools.lru_cache(maxsize=None)
def warp_chain(fill):
    """All poses applied in place, one after the other, on (70, 66): (prev, ((inv, warped), ...))."""
    H, W = 70, 66
    prev = _frozen(FILLS[fill](H, W))
    o = warp_oracle(H, W)
    o.set_previous(prev)
    out = []
    for pos, th in warp_poses():
        inv = o.warp_matrix(pos, th)
        out.append(_frozen(inv, o.get_previous_grid_in_current_pose(pos, th)))
    return prev, tuple(out)


LIMIT_POSE = ((2.0 ** 30 - 128, 0.0), 0.0)   # the float below 2^30 is 2^30 - 64
REFUSED_POSES = [(2.0 ** 30, 0.0), (0.0, -(2.0 ** 30)), (np.inf, 0.0), (np.nan, 0.0)]


@functools.lru_cache(maxsize=None)
def warp_below_limit():
    """LIMIT_POSE on a 10 x 10 grid at 1 m: (prev, inv, warped) of the oracle."""
    prev = _frozen(finite_fill(10, 10))
    o = ko.BayesMapper(10, 10, 1.0, (0, 0, 0), 0.0, **BENCH)
    o.set_previous(prev)
    inv = o.warp_matrix(*LIMIT_POSE)
    return prev, *_frozen(inv, o.get_previous_grid_in_current_pose(*LIMIT_POSE))


def check_warp_single(H, W, fill, prev, results):
    """The conditions on the oracle's warps of one grid (mapper_ref.warp gives the source coordinates)."""
    prior = F(BENCH["p_prior"])
    # the translation of the matrix holds 0.5 H and 0.5 W: whole-cell shifts give whole-number sources on the grids
    # with an even height and width, and there the bounds are met at equality (>= 0 holds, < W - 1 does not)
    if H % 2 == 0 and W % 2 == 0:
        xs, ys = set(), set()
        for k in WHOLE_SHIFTS:
            with np.errstate(all="ignore"):
                ok, _ = mr.warp(prev, results[k][0])
            sx, sy = mr.warp_sources(H, W, results[k][0])
            assert (sx == np.round(sx)).all() and (sy == np.round(sy)).all()
            xs |= set(sx.ravel().tolist())
            ys |= set(sy.ravel().tolist())
            assert not ok[(sx == W - 1) | (sy == H - 1)].any()
            assert ok[(sx >= 0) & (sx <= W - 2) & (sy >= 0) & (sy <= H - 2)].all()
        assert {0.0, W - 2.0, W - 1.0} <= xs and {0.0, H - 2.0, H - 1.0} <= ys, (xs, ys)
    for k in PRIOR_ONLY:
        assert (results[k][1] == prior).all(), k
    if min(H, W) <= 2:
        inside = [int((bits(w) != bits(prior)).sum()) for _, w in results]
        if (H, W) == (2, 2):
            assert max(inside) == 1 and sum(inside) >= 1, inside
        else:
            assert max(inside) == 0, inside
    if (H, W, fill) == (64, 64, "finite"):
        w = results[0][1]
        sub = int(((np.abs(w) > 0) & (np.abs(w) < np.finfo(F).tiny)).sum())
        assert sub >= 100, sub
