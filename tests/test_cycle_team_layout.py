"""GPU: the team layout of the cycle kernel's cost phase (csrc/kc_team_layout.h, cycle_costs) -- a workgroup with R
survivors costs them by R teams of floor(16 / R) wavefronts, eight, four or two lanes per trajectory point.  One workgroup
(a lattice of 32 samples, fused_cycle=2, cycle_samples=32), scenes built with the oracle so that exactly R samples stay
admissible, every edge of the rule at the R where it bites: every cost, the admissible set, the winner and its row bit for
bit against the oracle, and the same record through the halves only (team_max 2) and a wavefront a sample (team_max 0).
At the headline horizon three and four survivors also run a box robot, LaserScan input (the near-table branch of the
obstacle wavefront), drop_samples = 0, weights that switch a term off, and the lattice as two workgroups of sixteen."""
import math

import numpy as np
import pytest

import kompass_hip as kh
import synthetic as syn
from helpers import hip_context, hip_cycle, oracle_cycle
from oracle import ko

BASE_OPTS = dict(fused_cycle=2, cycle_samples=32)
_SCENES = {}


def _inputs(P, robot=None, weights=None):
    """32 samples (4 vx x 8 omega) over a sparse cloud; the step is stretched for short horizons so that the paths stay
    5 s long and their end points apart (an obstacle on one of them leaves its neighbours admissible).  Two points: only
    the speed moves the end point -- 32 speeds, one step of 5 s, a thin robot."""
    inp = syn.make_controller_inputs("cfg2", seed=1, scale=0.1)
    vx, vy, om = syn.lattice_nonholonomic(4, 8) if P > 2 else syn.lattice_nonholonomic(32, 1)
    pts = syn.costmap_points(syn.CONFIGS["cfg2"]["map_side"], 0.05, 7, p_occ=0.0003, free_radius=1.0)
    inp = dict(inp, vx=vx, vy=vy, omega=om, P=P, points=pts, dt=0.1 if P >= 50 else round(5.0 / (P - 1), 3))
    if P == 2:
        inp["robot"] = dict(shape=syn.CYLINDER, dims=[0.01, 0.4])
    if robot is not None:
        inp["robot"] = robot
    if weights is not None:
        inp["weights"] = weights
    return inp


KEEP_CTRL = 30  # drop_samples = 0: a collision up to control point 30 drops the sample, a later one freezes it
KEEP_AT = (25, 28, 22, 18)  # the control point the obstacles go on: the first of these that ends on exactly R survivors


def _oracle(inp, sc, mode):
    if mode != "keep":
        return oracle_cycle(inp, scan=sc)
    rb, st = inp["robot"], inp["state"]
    coll = ko.Collision(rb["shape"], rb["dims"], (0, 0, 0), (0, 0, 0, 1), inp["octree_res"])
    coll.update_state(st[0], st[1], st[2])
    coll.update_points(inp["points"], True)
    ox, oy = ko.obstacles_from_points((0, 0, 0), (0, 0, 0, 1), st, inp["points"])
    ci = ko.CostInputs(inp["seg_xyz"], 0, inp["acc_at_seg"], inp["ref_len"], np.stack([ox, oy], axis=1),
                       np.float32(inp["max_range"]) / np.float32(3.0), inp["acc_limits"], ko.make_weights(*inp["weights"]))
    o = ko.full_cycle_mode(coll, ci, st, inp["dt"], inp["P"], inp["vx"], inp["vy"], inp["omega"], False, KEEP_CTRL, None)
    o["keep"] = (coll, ci)
    return o


def _scene(P, R, robot=None, weights=None, mode="points"):
    """The inputs and the oracle's cycle with exactly R admissible samples (cached: the tests share them unchanged).
    mode "scan": LaserScan input, a beam of its own ends on the end point of every sample taken out; "keep":
    drop_samples = 0, the obstacle goes on a control point (one on the end point would only freeze the sample)."""
    key = (P, R, None if robot is None else robot["shape"], weights, mode)
    if key in _SCENES:
        return _SCENES[key]
    for at in KEEP_AT if mode == "keep" else (-1,):
        _SCENES[key] = _build(P, R, robot, weights, mode, at)
        if len(_SCENES[key][2]["raw"]) == R:
            break
    return _SCENES[key]


def _build(P, R, robot, weights, mode, at):
    inp = _inputs(P, robot, weights)
    sc, used = None, set()
    if mode == "scan":
        ang, rng = syn.dense_scan(720, scale=1.6)
        sc = (np.array(rng), np.array(ang))
    for _ in range(64):
        o = _oracle(inp, sc, mode)
        if len(o["raw"]) <= R:
            break
        ex, ey = float(o["px"][-1][at]), float(o["py"][-1][at])  # a point of the last admissible sample's path
        if mode == "scan":  # (samples of one bearing: a beam each, or the nearer one's beam would free the farther)
            k = int(round((math.atan2(ey, ex) + math.pi) / (2 * math.pi / 720)))
            j = next(k + d for d in (0, 1, -1, 2, -2, 3, -3) if (k + d) % 720 not in used) % 720
            used.add(j)
            sc[0][j] = math.hypot(ex, ey)
        else:
            inp = dict(inp, points=np.ascontiguousarray(np.vstack([inp["points"], [[ex, ey, 0.0]]]), np.float32))
    return inp, sc, o


def _check(P, R, opts=None, **kw):
    inp, sc, o = _scene(P, R, **kw)
    assert len(o["raw"]) == R, (len(o["raw"]), R)
    ctx = hip_context(kh, inp)
    if kw.get("mode") == "keep":
        opts = dict(opts or {}, drop_samples=0, num_ctrl_points=KEEP_CTRL)
    for k, v in dict(BASE_OPTS, **(opts or {})).items():
        ctx.set_option(k, v)
    records = []
    for tm in (4, 2, 0):
        ctx.set_option("team_max", tm)
        h = hip_cycle(kh, inp, scan=sc, ctx=ctx)
        assert ctx.get_option("last_cycle_single_launch") == 1.0
        assert h["res"]["n_admissible"] == R
        np.testing.assert_array_equal(h["raw"], o["raw"])
        np.testing.assert_array_equal(h["costs"].view(np.uint32), o["costs"].view(np.uint32))
        assert h["res"]["found"] == (o["index"] >= 0)
        if o["index"] >= 0:
            assert h["res"]["index"] == o["index"] and h["res"]["raw_index"] == int(o["raw"][o["index"]])
            assert np.float32(h["res"]["cost"]) == np.float32(o["cost"])
            np.testing.assert_array_equal(h["best"][0].view(np.uint32), o["px"][o["index"]].view(np.uint32))
            np.testing.assert_array_equal(h["best"][1].view(np.uint32), o["py"][o["index"]].view(np.uint32))
        records.append((h["res"]["found"], h["res"]["index"], h["res"]["raw_index"], np.float32(h["res"]["cost"]).tobytes()))
    assert records[0] == records[1] == records[2]
    ctx.close()


# P: 2 smallest; 33: two lanes a point spill into a second wavefront; 48 | 49: four | two lanes at R = 4; 50: the headline;
# 56 | 57: eight | four lanes at R <= 2; 24 | 25: eight | four at R = 4; 32 | 33: eight | four at R = 3 (five wavefronts);
# 64: full; 65: no obstacle wavefront
CASES = [(50, R) for R in (0, 1, 2, 3, 4, 5)] + [
    (2, 0), (2, 1), (2, 2), (2, 3), (2, 4), (2, 5), (20, 3), (32, 3), (33, 3), (40, 3), (33, 4), (48, 4), (49, 4), (24, 4),
    (25, 4), (56, 1), (56, 2), (57, 1), (57, 2),
    (57, 4), (64, 1), (64, 2), (64, 3), (64, 4), (64, 5), (65, 2), (65, 3), (65, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("P,R", CASES)
def test_every_edge_of_the_layout_against_the_oracle(P, R):
    _check(P, R)


BOX = dict(shape=syn.BOX, dims=[0.3, 0.2, 0.4])


@pytest.mark.gpu
@pytest.mark.parametrize("R", [3, 4])
@pytest.mark.parametrize("what", ["box", "scan", "no_obstacle_weight", "obstacle_weight_only", "keep_samples", "two_by_16"])
def test_three_and_four_survivors_at_the_headline_horizon(R, what):
    if what == "box":
        _check(50, R, robot=BOX)
    elif what == "scan":  # LaserScan input: the near-table branch of the obstacle wavefront
        _check(50, R, mode="scan")
    elif what == "keep_samples":  # drop_samples = 0: frozen samples stay admissible
        _check(50, R, mode="keep")
    elif what == "no_obstacle_weight":
        _check(50, R, weights=(1.0, 1.0, 0.0, 0.0, 0.0))
    elif what == "obstacle_weight_only":
        _check(50, R, weights=(0.0, 0.0, 1.0, 0.0, 0.0))
    else:  # the same lattice as two workgroups of sixteen, reduced on the device
        _check(50, R, opts=dict(cycle_samples=16, host_reduce=0))
