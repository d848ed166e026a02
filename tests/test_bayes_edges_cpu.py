"""CPU: the yardstick of tests/test_bayes_edges_gpu.py.  On every input of those tests the C oracle
(ko.BayesMapper) must equal the literal restatement in tests/mapper_ref.py (scan_to_grid_baysian, cell_probability,
warp_previous) under same_prob: NaN as a class, every other value bit for bit (signed zeros and subnormals
included).  The conditions that make the inputs worth running (saturation at exactly 0 and 1, the two rounding
fixed points, NaN / negative / above-one outputs, whole-number source coordinates at the bounds of the warp,
subnormal blends) are asserted on the oracle here and again in front of every device comparison."""
import numpy as np
import pytest

import bayes_edges as be
from bayes_edges import F, same_prob


def _literal_feedback(scene, params, steps, seed=None):
    """The oracle's feedback sequence against the restatement fed with its own output, step by step."""
    H, W = scene[0], scene[1]
    prev = np.full((H, W), F(params["p_prior"]), F) if seed is None else seed
    walker = be.caching_walker()
    for k, (g, p) in enumerate(steps):
        lg, lp = be.literal_scan(scene, prev, params, walker)
        np.testing.assert_array_equal(g, lg)
        same_prob(p, lp, f"scan {k + 1}")
        prev = lp


# ---------------------------------------------------------------------------
# the comparison rule itself
# ---------------------------------------------------------------------------
def test_same_prob_is_bitwise_except_for_nan():
    nan_pos, nan_neg = np.array([0x7fc00000, 0xffc00000], np.uint32).view(F)
    payload = np.array([0x7f800001], np.uint32).view(F)[0]
    want = np.array([nan_neg, nan_pos, 0.0, 1e-40, 1.0], F)
    same_prob(np.array([nan_pos, payload, 0.0, 1e-40, 1.0], F), want)
    for k, v in [(0, 1.0), (2, -0.0), (3, 0.0), (3, np.nextafter(F(1e-40), F(1))), (4, be.ONE_BELOW), (4, np.nan)]:
        got = want.copy()
        got[k] = v
        with pytest.raises(AssertionError):
            same_prob(got, want)


# ---------------------------------------------------------------------------
# 1. feedback until saturation
# ---------------------------------------------------------------------------
def test_run1_bench_feedback_saturates_at_exact_zero_and_one():
    steps = be.run1()
    be.check_run1(steps)
    _literal_feedback(be.scene_a(), be.BENCH, steps)
    # p / (1 - p) at the two ends: +inf and 0, the cells never move again
    one, zero = F(1), F(0)
    with np.errstate(all="ignore"):
        assert np.isinf(one / (F(1) - one)) and zero / (F(1) - zero) == 0


def test_run2_default_feedback_settles_at_the_rounding_fixed_points():
    seed, steps = be.run2()
    be.check_run2(steps)
    _literal_feedback(be.scene_a(), be.DEFAULT, steps, seed)


def test_run3_class_scene_feedback():
    scene, params = be.class_scene()
    steps = be.run3()
    be.check_run3(steps)
    _literal_feedback(scene, params, steps)


# ---------------------------------------------------------------------------
# 2. special previous values under every kind of cell
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(be.PARAM_SETS))
def test_special_previous_values(name):
    prev, g, p = be.special_scan(name)
    be.check_special_scan(name, prev, g, p)
    lg, lp = be.literal_scan(be.scene_b(), prev, be.PARAM_SETS[name])
    np.testing.assert_array_equal(g, lg)
    same_prob(p, lp, name)


@pytest.mark.parametrize("H,W", be.SMALL_GRIDS)
def test_special_previous_values_on_small_grids(H, W):
    for name in be.PARAM_SETS:
        prev, g, p = be.small_scan(H, W, name)
        assert (g != -1).any()
        lg, lp = be.literal_scan(be.small_scene(H, W), prev, be.PARAM_SETS[name])
        np.testing.assert_array_equal(g, lg)
        same_prob(p, lp, f"{H}x{W} {name}")


# ---------------------------------------------------------------------------
# 3. the warp
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fill", list(be.FILLS))
@pytest.mark.parametrize("H,W", be.WARP_GRIDS)
def test_warp_single_poses(H, W, fill):
    prev, results = be.warp_single(H, W, fill)
    be.check_warp_single(H, W, fill, prev, results)
    for (pos, th), (inv, w) in zip(be.warp_poses(), results):
        same_prob(w, be.literal_warp(prev, inv, be.BENCH["p_prior"]), f"{H}x{W} {fill} pose {pos} {th}")


@pytest.mark.parametrize("fill", list(be.FILLS))
def test_warp_chain_in_place(fill):
    prev, results = be.warp_chain(fill)
    for (pos, th), (inv, w) in zip(be.warp_poses(), results):
        prev = be.literal_warp(prev, inv, be.BENCH["p_prior"])
        same_prob(w, prev, f"{fill} chain pose {pos} {th}")


# ---------------------------------------------------------------------------
# 4. the largest accepted pose
# ---------------------------------------------------------------------------
def test_warp_pose_just_below_2_30_cells_gives_the_prior():
    """(2^30 - 128, 0) on a 10 x 10 grid at 1 m is the largest pose the device accepts on that axis;
    poses from 2^30 cells on are never handed to the oracle, whose int conversion is the reference's."""
    prev, inv, w = be.warp_below_limit()
    assert (w == F(be.BENCH["p_prior"])).all()
    same_prob(w, be.literal_warp(prev, inv, be.BENCH["p_prior"]))
