"""The pruned searches of the tracked segment on inputs where their tie handling decides the result: exact ties
between segment points (closed loops, a hairpin's bisector, a lattice, a circle's centre), chunks and super-chunks
whose chord has no length, z = -0.0, large coordinates, segments of no length, and the near table's size guard.
Every search -- the eight-lane scan of the workgroup-per-sample kernel, wave_sample_total with and without the near
table (wavefront per sample), batch_totals (batched kernel), and in the single-launch cycle wave_sample_total again
or, for workgroups of up to four survivors, group_segment_search -- must give the bits of the oracle's full scan
(cost_evaluator.cpp:111-177) and the same lowest index: the goal cost reads acc[argmin].
The scenes and what makes them decisive are in segment_ties.py and test_segment_ties_cpu.py."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import synthetic as syn  # noqa: E402
from oracle import ko  # noqa: E402

import segment_ties as st  # noqa: E402
from helpers import assert_cycle_equal, hip_context, hip_cycle, oracle_cycle  # noqa: E402

ALL = dict(st.SCENES, **st.DEGENERATE)
ACC_LIMITS = (2.0, 0.0, 3.0)

CONFIGS = [dict(cost_kernel=1),
           dict(cost_kernel=2, near_table=0), dict(cost_kernel=2, near_table=16),
           dict(cost_kernel=2, near_table=128), dict(cost_kernel=2, near_table=500),
           dict(cost_kernel=2, cost_batch=2),
           dict(cost_kernel=0)]
WINDOW_CONFIGS = [dict(cost_kernel=1), dict(cost_kernel=2), dict(cost_kernel=2, near_table=0),
                  dict(cost_kernel=2, cost_batch=2)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert kh.device_count() >= 1, "no HIP device visible: the -m gpu tests need an MI355X"


def _oracle_eval(seg, acc, ref_len, px, py, w):
    ci = ko.CostInputs(seg, 0, acc, ref_len, None, np.float32(10.0) / np.float32(3.0), ACC_LIMITS,
                       ko.make_weights(w[0], w[1], 0.0, 0.0, 0.0))
    return ko.min_trajectory_cost(ci, px, py, None)


@functools.lru_cache(maxsize=None)
def _expected(name):
    """The oracle's answers for a scene, computed once: {(stack, weighting): (index, cost, costs)}."""
    s = ALL[name]
    return {(i, w): _oracle_eval(s.seg, s.acc, s.ref_len, px, py, w)
            for i, (px, py) in enumerate(s.stacks()) for w in st.WEIGHTINGS}


def _context(S, opts):
    ctx = kh.DwaContext(syn.CYLINDER, [0.1, 0.4], max_samples=64, max_points=max(st.PS), max_segment=max(S, 16),
                        max_obstacles=16, acc_limits=ACC_LIMITS)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


def _same(got, want, what):
    """(Result, costs) of the library against (index, cost, costs) of the oracle: bits, a NaN for a NaN."""
    r, costs = got
    oi, oc, ocosts = want
    np.testing.assert_array_equal(st.bits(costs), st.bits(ocosts), err_msg=what)
    if oi < 0:       # nothing below FLT_MAX (every cost NaN or inf): the oracle's strict `<` selects nothing
        assert not r.found and r.index == -1, what
    else:
        assert r.found and r.index == oi and np.float32(r.cost) == np.float32(oc), what


def _evaluate_all(ctx, name, what):
    s = ALL[name]
    want = _expected(name)
    for w in st.WEIGHTINGS:
        ctx.set_weights(kh.make_weights(w[0], w[1], 0.0, 0.0, 0.0))
        for i, (px, py) in enumerate(s.stacks()):
            tag = f"{name} {what} w={w} P={px.shape[1]}"
            _same(ctx.cost_evaluate(px, py, None), want[i, w], tag)
            ctx.cost_upload(px, py, None)      # and resident, twice: the near table is kept on the second call
            _same(ctx.cost_evaluate_resident(), want[i, w], tag + " resident")
            _same(ctx.cost_evaluate_resident(), want[i, w], tag + " resident again")


@pytest.mark.parametrize("name", sorted(ALL))
def test_caller_paths_on_tie_scenes(name):
    """kc_cost_evaluate over every scene, one fresh context per kernel configuration.  (The C ABI takes segments of
    one, two and three points: the degenerate scenes run like the others and give the oracle's inf / NaN.)"""
    s = ALL[name]
    for opts in CONFIGS:
        ctx = _context(s.S, opts)
        ctx.set_tracked_segment(s.seg, s.acc, s.ref_len)
        _evaluate_all(ctx, name, str(opts))
        ctx.close()


@pytest.mark.parametrize("name", sorted(ALL))
def test_resident_path_window_on_tie_scenes(name):
    """The same scenes as a window of a device-resident path (segment_window_kernel builds the tables on the
    device), the window the whole scene: against the oracle, and against a context fed by set_tracked_segment."""
    s = ALL[name]
    for opts in WINDOW_CONFIGS:
        a, b = _context(s.S, opts), _context(s.S, opts)
        a.set_path(s.seg, s.acc, s.ref_len)
        a.set_tracked_window(0, s.S)
        b.set_tracked_segment(s.seg, s.acc, s.ref_len)
        _evaluate_all(a, name, f"window {opts}")
        w = st.WEIGHTINGS[2]
        for c in (a, b):
            c.set_weights(kh.make_weights(w[0], w[1], 0.0, 0.0, 0.0))
        for px, py in s.stacks():
            (ra, ca), (rb, cb) = a.cost_evaluate(px, py, None), b.cost_evaluate(px, py, None)
            np.testing.assert_array_equal(st.bits(ca), st.bits(cb))
            assert (ra.found, ra.index) == (rb.found, rb.index)
        a.close(); b.close()


@pytest.mark.parametrize("start", [512, 0, 256])
def test_window_between_the_coincident_pair_of_a_two_lap_path(start):
    """Two laps of closed_square as the resident path; the window [512, 1025) begins and ends on the coincident
    pair (so does [0, 513)), [256, 769) has the pair in its middle: acc of the tied points differs by a lap."""
    sq = st.SCENES["closed_square"]
    seg = np.concatenate([sq.seg, sq.seg[1:]])
    acc = np.concatenate([sq.acc, sq.acc[1:] + sq.acc[-1]]).astype(np.float32)
    ref_len = float(acc[-1])
    S = sq.S
    wseg, wacc = seg[start:start + S], acc[start:start + S]
    assert (wseg[0] == wseg[-1]).all() and wacc[-1] - wacc[0] == 32.0
    for opts in WINDOW_CONFIGS:
        a, b = _context(len(seg), opts), _context(len(seg), opts)
        a.set_path(seg, acc, ref_len)
        a.set_tracked_window(start, S)
        b.set_tracked_segment(wseg, wacc, ref_len)
        for w in st.WEIGHTINGS:
            for c in (a, b):
                c.set_weights(kh.make_weights(w[0], w[1], 0.0, 0.0, 0.0))
            for px, py in sq.stacks():
                want = _oracle_eval(wseg, wacc, ref_len, px, py, w)
                _same(a.cost_evaluate(px, py, None), want, f"window {start} {opts} w={w}")
                _same(b.cost_evaluate(px, py, None), want, f"segment {start} {opts} w={w}")
        a.close(); b.close()


@pytest.mark.parametrize("P", st.CYCLE_PS)
@pytest.mark.parametrize("case", range(len(st.CYCLES)))
def test_full_cycles_on_the_bisector_and_the_loop(case, P):
    """Whole controller cycles whose roll-outs run along the hairpin's bisector (every point ties between the legs)
    and along the first side of the closed loop from its start corner; no obstacles."""
    scene, state = st.CYCLES[case]
    inp = st.cycle_inputs(scene, state, P)
    o = oracle_cycle(inp)
    assert len(o["raw"]) == len(inp["vx"])
    for opts in (dict(fused_cycle=0), dict(fused_cycle=2), dict(fused_cycle=0, cost_kernel=2, force_split=1)):
        ctx = hip_context(kh, inp)
        for k, v in opts.items():
            ctx.set_option(k, v)
        assert_cycle_equal(o, hip_cycle(kh, inp, ctx=ctx))
        ctx.close()


@pytest.mark.parametrize("ks", st.TEAM_KS, ids=lambda ks: f"{len(ks)}samples")
def test_cycles_of_few_samples_costed_by_teams(ks):
    """One to four survivors in a workgroup of the single-launch cycle: group_segment_search, eight or four lanes
    a point, on end points whose two tied indices fall to the same lane."""
    inp = st.cycle_inputs("hairpin_even", (0.0, 0.25, 0.0, 0.0), 31, ks)
    o = oracle_cycle(inp)
    assert len(o["raw"]) == len(ks)
    for opts in (dict(fused_cycle=2), dict(fused_cycle=2, near_table=0), dict(fused_cycle=0)):
        ctx = hip_context(kh, inp)
        for k, v in opts.items():
            ctx.set_option(k, v)
        assert ctx.get_option("team_max") == 4
        assert_cycle_equal(o, hip_cycle(kh, inp, ctx=ctx))
        ctx.close()


@pytest.mark.parametrize("near_table", [128, 0])
@pytest.mark.parametrize("S", [65535, 65536])
def test_near_table_size_guard(S, near_table):
    """The near table packs clo | chi << 8 | seed << 16: a seed needs all 16 bits at S = 65535, and from
    S = 65536 on the table is left out.  End points nearest to the last point, to index 0 and inside the last chunk."""
    s = st.straight_large(S)
    (px, py), = s.stacks()
    ctx = kh.DwaContext(syn.CYLINDER, [0.1, 0.4], max_samples=8, max_points=5, max_segment=S, max_obstacles=16,
                        acc_limits=ACC_LIMITS)
    ctx.set_option("cost_kernel", 2)
    ctx.set_option("near_table", near_table)
    ctx.set_tracked_segment(s.seg, s.acc, s.ref_len)
    for w in st.WEIGHTINGS:
        ctx.set_weights(kh.make_weights(w[0], w[1], 0.0, 0.0, 0.0))
        want = _oracle_eval(s.seg, s.acc, s.ref_len, px, py, w)
        _same(ctx.cost_evaluate(px, py, None), want, f"S={S} near_table={near_table} w={w}")
        _same(ctx.cost_evaluate(px, py, None), want, f"S={S} near_table={near_table} w={w} again")
    ctx.close()
