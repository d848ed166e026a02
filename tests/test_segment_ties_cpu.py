"""The tie scenes of segment_ties.py, without a GPU: the oracle's full scan against the plain numpy statement, bit
for bit, and the conditions that make the GPU tests of the same scenes mean something -- the ties are real
(float32 minima == integer-arithmetic minima), they lie in different chunks and super-chunks of the kernels' tables,
and picking the other one changes the goal cost visibly."""
import numpy as np
import pytest

import segment_ties as st
from helpers import oracle_cycle
from oracle import ko

ALL = dict(st.SCENES, **st.DEGENERATE)


def _oracle(scene, px, py, w_path, w_goal):
    ci = ko.CostInputs(scene.seg, 0, scene.acc, scene.ref_len, None, np.float32(10.0) / np.float32(3.0), (2.0, 0.0, 3.0),
                       ko.make_weights(w_path, w_goal, 0.0, 0.0, 0.0))
    return ko.min_trajectory_cost(ci, px, py, None)


@pytest.mark.parametrize("name", sorted(ALL))
def test_oracle_equals_the_plain_statement(name):
    scene = ALL[name]
    stacks = scene.stacks()
    assert stacks and sum(len(px) for px, _ in stacks) == 3 * len(scene.ends)
    for px, py in stacks:
        path, goal, _, _ = st.path_goal_np(scene.seg, scene.acc, scene.ref_len, px, py)
        for w_path, w_goal in st.WEIGHTINGS:
            want = st.totals_np(path, goal, w_path, w_goal, scene.ref_len)
            idx, cost, costs = _oracle(scene, px, py, w_path, w_goal)
            np.testing.assert_array_equal(st.bits(costs), st.bits(want), err_msg=f"P={px.shape[1]} w=({w_path}, {w_goal})")
            widx, wcost = st.select_np(want)
            assert idx == widx
            if idx >= 0:
                assert np.float32(cost) == wcost
        if scene.kind != "degenerate":
            assert st.select_np(st.totals_np(path, goal, 0.7, 1.3, scene.ref_len))[0] > 0   # never the first of its stack


def test_degenerate_scenes_have_no_length():
    """seg_len == 0: the end-point term of the path cost is x / 0 -- inf beside the point, NaN on it -- and no such
    cost is ever selected (strict `<` against FLT_MAX)."""
    for scene in st.DEGENERATE.values():
        assert st.segment_length_np(scene.seg) == 0.0
        for px, py in scene.stacks():
            path, goal, arg, _ = st.path_goal_np(scene.seg, scene.acc, scene.ref_len, px, py)
            assert not np.isfinite(path).any() and np.isfinite(goal).all() and (arg == 0).all()
            assert st.select_np(st.totals_np(path, goal, 1.0, 0.0, scene.ref_len))[0] == -1
            assert st.select_np(st.totals_np(path, goal, 0.0, 1.0, scene.ref_len))[0] >= 0
    for s in st.DEGENERATE.values():
        path = np.concatenate([st.path_goal_np(s.seg, s.acc, s.ref_len, px, py)[0] for px, py in s.stacks()])
        assert np.isnan(path).any() and np.isinf(path).any()


def _tied_ends(scene):
    out = []
    for x, y, _ in scene.ends:
        m = sorted(st.minima_np(scene.seg, x, y))
        if len(m) >= 2:
            out.append((x, y, m))
    return out


@pytest.mark.parametrize("name", st.TIE_SCENES)
def test_tie_scenes_have_real_and_visible_ties(name):
    scene = st.SCENES[name]
    chunk, sup = st.chunk_of(scene.S), st.super_of(scene.S)
    assert chunk == 16 and scene.S <= 1025
    for x, y, _ in scene.ends:          # a float tie is a real tie, a float minimum the real minimum
        assert st.minima_np(scene.seg, x, y) == st.exact_ties(scene.seg, x, y), (x, y)
    tied = _tied_ends(scene)
    assert len(tied) >= 3
    if "hairpin" not in name:           # (every query on the bisector ties) and a control
        assert any(len(st.minima_np(scene.seg, x, y)) == 1 for x, y, _ in scene.ends)
    L = np.float32(scene.ref_len)
    for x, y, m in tied:
        lo, hi = m[0], m[-1]
        assert scene.acc[lo] != scene.acc[hi]
        d = np.sqrt(st._d2(scene.seg, np.float32(x), np.float32(y))[lo])
        g_lo = (L - scene.acc[lo]) / L + d / L
        g_hi = (L - scene.acc[hi]) / L + d / L
        assert abs(float(g_lo) - float(g_hi)) > 1e-3, (x, y, m)
    assert any(m[0] // chunk != m[-1] // chunk for _, _, m in tied)
    if scene.far_super:
        assert any(m[0] // sup != m[-1] // sup for _, _, m in tied)
    # the statement's own end-point columns say the same for the stacked trajectories
    for px, py in scene.stacks():
        _, _, arg, cnt = st.path_goal_np(scene.seg, scene.acc, scene.ref_len, px, py)
        for n in range(len(px)):
            m = st.minima_np(scene.seg, px[n, -1], py[n, -1])
            assert arg[n] == min(m) and cnt[n] == len(m)


def test_named_scenes_have_the_ties_their_comments_name():
    sq = st.SCENES["closed_square"]
    assert sq.S == 513 and (sq.seg[0] == sq.seg[512]).all() and sq.ref_len == 32.0
    assert sorted(st.minima_np(sq.seg, 0.0, 0.0)) == [0, 512]                   # chunks 0 and 32, super-chunks 0 and 4
    assert len(st.minima_np(sq.seg, 1.0 / 32.0, 0.0)) == 3 and len(st.minima_np(sq.seg, 0.0, 1.0 / 32.0)) == 3
    assert sorted(st.minima_np(sq.seg, 4.0, 4.0)) == [64, 192, 320, 448]
    assert sorted(st.minima_np(sq.seg, 8.0, 8.0)) == [256]
    assert (st.SCENES["closed_small17"].S, st.SCENES["closed_small33"].S) == (17, 33)
    hp = st.SCENES["hairpin_bisector"]
    assert hp.S == 800
    for x, y, _ in hp.ends:
        m = sorted(st.minima_np(hp.seg, x, y))
        assert len(m) == 2 and m[0] < 400 <= m[1]                               # one on each leg, at every query
    assert any(m % 16 == 0 for x, y, _ in hp.ends for m in st.minima_np(hp.seg, x, y))
    lift = st.SCENES["hairpin_lifted"]
    assert (lift.seg[:400, 2] == 0.5).all() and (lift.seg[400:, 2] == 0.0).all()
    assert all(y == 0.0 and len(st.minima_np(lift.seg, x, y)) == 2 for x, y, _ in lift.ends)
    zz = st.SCENES["lattice_zigzag"]
    assert zz.S == 257 and sorted(len(st.minima_np(zz.seg, x, y)) for x, y, _ in zz.ends) == [1, 2, 2, 3, 3]
    for name, s in st.SCENES.items():
        if name.endswith("-negzero"):
            assert np.signbit(s.seg[:, 2]).all() and (s.seg[:, 2] == 0).all()
            base = st.SCENES[name[:-len("-negzero")]]
            for x, y, _ in s.ends:
                assert st.minima_np(s.seg, x, y) == st.minima_np(base.seg, x, y)
        if s.kind != "circle" and (name.endswith("-east") or name.endswith("-west")):   # (a shifted circle is rounded anew)
            base = st.SCENES[name[:-5]]
            for (x, y, _), (bx, by, _) in zip(s.ends, base.ends):                # shifted: the same ties
                assert st.minima_np(s.seg, x, y) == st.minima_np(base.seg, bx, by)


@pytest.mark.parametrize("name", ["circle_centre", "circle_centre-negzero"])
def test_circle_centre_ties_are_many_and_everywhere(name):
    """(The variants with z = 0.5 and the shifted ones round every distance anew: other float ties, fewer of them;
    they are compared with the oracle like every scene and carry no condition of their own.)"""
    c = st.SCENES[name]
    (x0, y0, _), (x1, y1, _), (x2, y2, _) = c.ends
    m = sorted(st.minima_np(c.seg, x0, y0))
    chunk, sup = st.chunk_of(c.S), st.super_of(c.S)
    assert chunk == 16
    assert len(m) >= 50 and len({j // chunk for j in m}) >= 20 and len({j // sup for j in m}) >= 2
    assert len(set(c.acc[m].tolist())) == len(m)
    assert len(st.minima_np(c.seg, x1, y1)) == 1 and len(st.minima_np(c.seg, x2, y2)) == 1


@pytest.mark.parametrize("name", [n for n in sorted(st.SCENES) if st.SCENES[n].kind == "zero"])
def test_stationary_runs_have_zero_chords(name):
    s = st.SCENES[name]
    chunk = st.chunk_of(s.S)
    span = 8 * chunk if "128" in name else chunk
    whole = [c for c in range(s.S // span) if (s.seg[c * span:(c + 1) * span] == s.seg[c * span]).all()]
    assert whole, "no whole chunk / super-chunk is a single point"
    x, y, _ = s.ends[0]
    m = st.minima_np(s.seg, x, y)
    assert len(m) >= 40 and m == st.exact_ties(s.seg, x, y)


def test_large_segments_need_all_sixteen_seed_bits():
    for S in (65535, 65536):
        s = st.straight_large(S)
        (px, py), = s.stacks()
        assert px.shape == (8, 5)
        _, _, arg, cnt = st.path_goal_np(s.seg, s.acc, s.ref_len, px, py)
        chunk = st.chunk_of(S)
        assert (arg[:3] == S - 1).all() and (arg[3:5] == 0).all() and (arg[5:] // chunk == (S - 1) // chunk).all()
        assert cnt[7] == 2 and S - 1 >= 0x8000


def _one_lane_tie(m):
    """Both minima at even indices, no chunk head, in the same residue modulo 16: one lane of eight meets both."""
    m = sorted(m)
    return len(m) == 2 and m[0] % 2 == 0 and m[0] % 16 != 0 and (m[1] - m[0]) % 16 == 0


def test_hairpin_even_has_ties_that_one_lane_decides():
    s = st.SCENES["hairpin_even"]
    assert _one_lane_tie(st.minima_np(s.seg, *s.ends[0][:2])) and _one_lane_tie(st.minima_np(s.seg, *s.ends[2][:2]))
    m = sorted(st.minima_np(s.seg, *s.ends[1][:2]))
    assert len(m) == 2 and m[0] % 8 == 4 and m[1] % 8 == 4                      # one lane of four
    for name in ("hairpin_bisector", "closed_square", "lattice_zigzag"):         # (no other scene has one)
        assert not any(_one_lane_tie(st.minima_np(st.SCENES[name].seg, x, y)) for x, y, _ in st.SCENES[name].ends)
    hits = 0
    for scene, state in st.CYCLES:
        if scene != "hairpin_even":
            continue
        for P in st.CYCLE_PS:
            o = oracle_cycle(st.cycle_inputs(scene, state, P))
            assert (o["py"] == np.float32(0.25)).all() and len(o["raw"]) == 12
            hits += sum(_one_lane_tie(st.exact_ties(s.seg, x, y)) for x, y in zip(o["px"][:, -1], o["py"][:, -1]))
    assert hits >= 4


def test_team_cycles_end_on_ties_of_one_lane():
    s = st.SCENES["hairpin_even"]
    for ks in st.TEAM_KS:
        o = oracle_cycle(st.cycle_inputs("hairpin_even", (0.0, 0.25, 0.0, 0.0), 31, ks))
        assert len(o["raw"]) == len(ks) <= 4
        for x, y in zip(o["px"][:, -1], o["py"][:, -1]):
            m = sorted(st.exact_ties(s.seg, x, y))
            lanes = 8 if len(ks) <= 2 else 4
            assert len(m) == 2 and m[0] % 2 == 0 and m[0] % 16 != 0 and (m[0] // 2) % lanes == (m[1] // 2) % lanes


@pytest.mark.parametrize("P", st.CYCLE_PS)
def test_rollout_scene_stays_on_the_bisector(P):
    for scene, state in st.CYCLES[:2]:
        assert scene == "hairpin_bisector"
        inp = st.cycle_inputs(scene, state, P)
        o = oracle_cycle(inp)
        assert len(o["raw"]) == len(inp["vx"])                     # no obstacles: everything admissible
        assert (o["py"] == np.float32(0.25)).all()
        assert (o["px"] * 64 == np.round(o["px"] * 64)).all()
        s = st.SCENES[scene]
        two = sum(len(st.exact_ties(s.seg, x, y)) == 2 for x, y in zip(o["px"][:, -1], o["py"][:, -1]))
        assert 2 * two >= len(o["raw"])
