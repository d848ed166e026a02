"""GPU: bayes_cells_kernel, warp_kernel and the host side of kc_mapper_warp_previous (kh.MapperContext, and the
kompass_cpp.mapping.LocalMapper class surface) against the oracle where the feedback loop takes them: cells
saturated at exactly 0 and 1, the rounding fixed points of the default sensor model, previous values no scan
produces (+-0, subnormals, beyond [0, 1], +-inf, NaN), grids smaller than a workgroup, warps whose source
coordinates sit on the bounds, subnormal blends, and poses at the 2^30-cell rule.

tests/test_bayes_edges_cpu.py pins the oracle to the literal restatement on the same inputs.  The comparison is
bayes_edges.same_prob: NaN as a class, every other value bit for bit.  The conditions on each input are asserted on
the oracle before the device is compared."""
import numpy as np
import pytest

import bayes_edges as be
from bayes_edges import F, bits, same_prob

pytestmark = pytest.mark.gpu


def _device_feedback(scene, params, steps, seed=None):
    """scan -> set_previous_prob(None) on one context, against the oracle's sequence at every step."""
    import kompass_hip as kh
    H, W, res, pos, orient, ang, rng = scene
    m = kh.MapperContext(H, W, res, pos, orient, len(ang))
    m.enable_bayes(**params)
    if seed is not None:
        m.set_previous_prob(seed)
    for k, (want_g, want_p) in enumerate(steps):
        got_g, got_p = m.scan_to_grid_baysian(ang, rng)
        np.testing.assert_array_equal(got_g, want_g)
        same_prob(got_p, want_p, f"scan {k + 1}")
        m.set_previous_prob(None)
    same_prob(m.previous_prob(), steps[-1][1], "previous grid after the last feedback")
    m.close()


# ---------------------------------------------------------------------------
# 1. feedback until saturation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", ["1", "0", "3"])
def test_bench_feedback_until_cells_saturate(tiles, monkeypatch):
    """Benchmark sensor model: exact 1.0f after 10 scans, exact 0.0f after 15; from then on the previous odds are
    1 / 0 = +inf or 0 and the cells stay."""
    monkeypatch.setenv("KC_MAPPER_TILES", tiles)
    steps = be.run1()
    be.check_run1(steps)
    _device_feedback(be.scene_a(), be.BENCH, steps)


def test_default_feedback_at_the_rounding_fixed_points():
    """Default sensor model from a seed next to 0 and 1: the cells settle at nextafter(1, 0) and float(2^-52), where
    the correctly rounded float divide of p / (1 - p) and the narrowing of 1 - 1 / (1 + odds) decide every bit."""
    seed, steps = be.run2()
    be.check_run2(steps)
    _device_feedback(be.scene_a(), be.DEFAULT, steps, seed)


def test_class_surface_feedback_loop():
    """kompass_cpp.mapping.LocalMapper: scan_to_grid_baysian + set_previous_grid(None), 16 scans."""
    import kompass_cpp
    (H, W, res, pos, orient, ang, rng), params = be.class_scene()
    steps = be.run3()
    be.check_run3(steps)
    cm = kompass_cpp.mapping.LocalMapper(grid_height=H, grid_width=W, resolution=res,
                                         laserscan_position=list(pos), laserscan_orientation=orient,
                                         is_pointcloud=False, scan_size=len(ang), angle_step=0.01, max_height=10.0,
                                         min_height=-10.0, max_points_per_line=600, **params)
    for k, (want_g, want_p) in enumerate(steps):
        g, p = cm.scan_to_grid_baysian(angles=list(ang), ranges=list(rng))
        np.testing.assert_array_equal(np.asarray(g), want_g)
        same_prob(np.asarray(p).copy(), want_p, f"scan {k + 1}")
        cm.set_previous_grid(None)


# ---------------------------------------------------------------------------
# 2. special previous values under every kind of cell
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(be.PARAM_SETS))
def test_special_previous_values(name):
    import kompass_hip as kh
    prev, want_g, want_p = be.special_scan(name)
    be.check_special_scan(name, prev, want_g, want_p)
    H, W, res, pos, orient, ang, rng = be.scene_b()
    m = kh.MapperContext(H, W, res, pos, orient, len(ang))
    m.enable_bayes(**be.PARAM_SETS[name])
    m.set_previous_prob(prev)
    np.testing.assert_array_equal(bits(m.previous_prob()), bits(prev))      # the upload keeps every bit, NaN too
    got_g, got_p = m.scan_to_grid_baysian(ang, rng)
    np.testing.assert_array_equal(got_g, want_g)
    same_prob(got_p, want_p, name)
    m.close()


@pytest.mark.parametrize("H,W", be.SMALL_GRIDS)
def test_special_previous_values_on_small_grids(H, W):
    import kompass_hip as kh
    _, _, res, pos, orient, ang, rng = be.small_scene(H, W)
    for name, params in be.PARAM_SETS.items():
        prev, want_g, want_p = be.small_scan(H, W, name)
        assert (want_g != -1).any()
        m = kh.MapperContext(H, W, res, pos, orient, len(ang))
        m.enable_bayes(**params)
        m.set_previous_prob(prev)
        got_g, got_p = m.scan_to_grid_baysian(ang, rng)
        np.testing.assert_array_equal(got_g, want_g)
        same_prob(got_p, want_p, f"{H}x{W} {name}")
        m.close()


# ---------------------------------------------------------------------------
# 3. the warp
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fill", list(be.FILLS))
@pytest.mark.parametrize("H,W", be.WARP_GRIDS)
def test_warp_single_poses(H, W, fill):
    import kompass_hip as kh
    prev, results = be.warp_single(H, W, fill)
    be.check_warp_single(H, W, fill, prev, results)
    m = kh.MapperContext(H, W, be.WARP_RES, (0, 0, 0), 0.0, 16)
    m.enable_bayes(**be.BENCH)
    for (pos, th), (_, want) in zip(be.warp_poses(), results):
        m.set_previous_prob(prev)
        m.get_previous_grid_in_current_pose(pos, th)
        same_prob(m.previous_prob(), want, f"{H}x{W} {fill} pose {pos} {th}")
    m.close()


@pytest.mark.parametrize("fill", list(be.FILLS))
def test_warp_chain_in_place(fill):
    import kompass_hip as kh
    prev, results = be.warp_chain(fill)
    m = kh.MapperContext(70, 66, be.WARP_RES, (0, 0, 0), 0.0, 16)
    m.enable_bayes(**be.BENCH)
    m.set_previous_prob(prev)
    for (pos, th), (_, want) in zip(be.warp_poses(), results):
        m.get_previous_grid_in_current_pose(pos, th)
        same_prob(m.previous_prob(), want, f"{fill} chain pose {pos} {th}")
    m.close()


# ---------------------------------------------------------------------------
# 4. the warp's pose under the 2^30 rule
# ---------------------------------------------------------------------------
def test_warp_pose_at_2_30_cells_is_refused_and_leaves_the_previous_grid():
    import kompass_hip as kh
    prev, _, want = be.warp_below_limit()
    assert (want == F(be.BENCH["p_prior"])).all()
    m = kh.MapperContext(10, 10, 1.0, (0, 0, 0), 0.0, 16)
    m.enable_bayes(**be.BENCH)
    m.set_previous_prob(prev)
    for pos in be.REFUSED_POSES:
        with pytest.raises(IndexError, match="2\\^30"):
            m.get_previous_grid_in_current_pose(pos, 0.0)
        np.testing.assert_array_equal(bits(m.previous_prob()), bits(prev))
    # a non-finite orientation stays accepted, as the reference has it: no source lies inside
    for th in (np.nan, np.inf):
        m.get_previous_grid_in_current_pose((0.0, 0.0), th)
        assert (m.previous_prob() == F(be.BENCH["p_prior"])).all()
        m.set_previous_prob(prev)
    m.get_previous_grid_in_current_pose(*be.LIMIT_POSE)
    same_prob(m.previous_prob(), want, "pose just below 2^30 cells")
    m.close()


def test_class_surface_refuses_the_pose_too():
    import kompass_cpp
    (H, W, res, pos, orient, ang, _), params = be.class_scene()
    cm = kompass_cpp.mapping.LocalMapper(grid_height=H, grid_width=W, resolution=res,
                                         laserscan_position=list(pos), laserscan_orientation=orient,
                                         is_pointcloud=False, scan_size=len(ang), angle_step=0.01, max_height=10.0,
                                         min_height=-10.0, max_points_per_line=600, **params)
    for p in ([res * 2.0 ** 30, 0.0], [0.0, float("nan")]):
        with pytest.raises(IndexError):
            cm.get_previous_grid_in_current_pose(p, 0.0)
