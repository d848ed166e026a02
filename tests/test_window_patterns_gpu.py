"""The velocity window's pattern store on the MI355X (the rule and the orders: csrc/kc_sample_pattern.h, natively in
tests/native/sample_pattern.cpp; the uploads: upload_samples / build_perm, csrc/kc_dwa.hip; DESIGN.md 0.4, point 11):
the device tables a cycle reads after a window came back from the store, was replaced in it, was overwritten by an explicit list, met other options or another share than it was built for, or does not fit the
kernels' LDS tables.  A stale table raises no error, it gives other samples, so every step runs three ways
(tests/window_patterns.py: the context under test, a context that only ever sees explicit lists, the oracle) and
everything a cycle leaves is compared as bits; the counters pattern_hits / pattern_builds follow a plain model of the
rule step by step.

Every test runs under a time limit: a cycle whose workgroups wait for a record that never comes would not return,
and a Python-level limit cannot interrupt a native call; the thread method ends the process instead."""
import numpy as np
import pytest

TIME_LIMIT_S = 120   # the slowest test takes a few seconds on an MI355X box; a loaded box gets many times that

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(TIME_LIMIT_S, method="thread")]

import kompass_hip as kh  # noqa: E402
import sharding  # noqa: E402
import synthetic as syn  # noqa: E402
import window_patterns as wp  # noqa: E402
from helpers import oracle_cycle  # noqa: E402
from oracle import ko  # noqa: E402

ACK, DIFF, OMNI = syn.ACKERMANN, syn.DIFFERENTIAL_DRIVE, syn.OMNI


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert kh.device_count() >= 1, "no HIP device visible: the -m gpu tests need an MI355X"


@pytest.fixture(scope="module")
def scene():
    return wp.make_scene()


def test_eviction_and_return(scene):
    """272 windows of distinct pattern (odd L in 3..35 x odd A in 1..31 around 0.5 m/s: no small value, the pattern is
    the two axis lengths) against 256 slots: swept once (the first 15 are replaced), again in the same order (every
    one was replaced before its turn and is built again, replacing the oldest), then in reverse (the last one is still
    active, the 256 put away most recently come back by a swap, the oldest 15 are built)."""
    lims = wp.limits_pair()
    cur = (0.5, 0.0, 0.1)
    windows = [(L, A) for L in range(3, 36, 2) for A in range(1, 32, 2)]
    assert len(windows) == 272
    run = wp.ThreeWays(scene)
    for L, A in windows + windows + windows[::-1]:
        run.window(DIFF, lims, cur, L, A)
    assert len(set(run.keys[:272])) == 272, "the windows were meant to differ in pattern, by the oracle's axes"
    count = run.model.count
    print(f"eviction_and_return: {run.steps} steps, same {count['same']}, hit {count['hit']}, build {count['build']}, "
          f"least-recently-used slot taken {count['lru']} times, {run.oracle_steps} oracle cycles, {run.mixed} steps with "
          f"0 < admissible < n")
    assert run.classes[:544] == ["build"] * 544 and run.classes[544:] == ["same"] + ["hit"] * 256 + ["build"] * 15
    assert count["lru"] >= 16
    assert run.counters() == (count["hit"], count["build"])
    assert run.mixed >= run.steps // 2, "the scene was meant to leave 0 < admissible < n"
    run.finish()


def test_lists_between_windows(scene):
    """Explicit lists have no signature: they overwrite the active tables and are never kept, a window after one finds
    nothing worth keeping (on a hit the slot empties), an equal list stays active by vector equality, the empty list
    uploads nothing."""
    lims = wp.limits_pair()
    X, Y = ((0.5, 0.0, 0.1), 9, 7), ((0.3, 0.0, -0.2), 7, 5)
    E = ko.sample_velocities(DIFF, lims[1], (0.6, 0.0, 0.0), scene["dt"], 5, 9)
    by_omega = np.argsort(E[2], kind="stable")
    E2 = tuple(a[by_omega] for a in E)                 # the same count, other rows
    E3 = tuple(a[::-1].copy() for a in E)              # other values in the same pattern: equal index vectors
    assert wp.list_labels(*E2) != wp.list_labels(*E) and wp.list_labels(*E3) == wp.list_labels(*E)
    none = (np.zeros(0),) * 3
    run = wp.ThreeWays(scene)
    win = lambda w, how=None: run.window(DIFF, lims, w[0], w[1], w[2], how)
    win(X)
    run.explicit(*E)      # overwrites X
    win(X)                # X was not kept: built again
    win(Y)                # X is put away
    run.explicit(*E)      # overwrites Y
    run.explicit(*E)      # the same list: stays active
    run.explicit(*E3)     # equal index vectors, other values: stays active, value tables rewritten
    run.explicit(*E2)     # other rows
    run.explicit(*none)
    run.explicit(*E2)     # the tables of E2 are still there, its orders are not
    run.explicit(*none)
    win(X)                # a hit with nothing worth keeping: the slot empties
    win(Y)                # Y was overwritten: built, X goes into the emptied slot
    run.explicit(*none)
    win(Y, "find")        # still active
    win(X)
    assert run.classes == ["build", "build", "build", "hit", "build", "same", "hit"]
    assert run.model.slots == 1
    assert run.counters() == (2, 4 + 3 + 2)   # builds: X, X, Y, Y; E, E, E2; the orders of E2 and of Y after an empty list
    run.finish()


def test_options_between_reuses(scene):
    """A pattern comes back from the store under other options than its walking orders were built for: samples per
    workgroup (a rectangular window, whose dealt order depends on them), the single launch on or off (the dealt and
    the plain order each go to the device after the other was valid), the device trig."""
    lims = wp.limits_pair()
    A, B = ((0.5, 0.0, 0.1), 8, 24), ((0.5, 0.0, 0.1), 11, 5)
    xs, _, oms = wp.window_axes(DIFF, lims[1], A[0], scene["dt"], A[1], A[2])
    assert len(xs) % 4 == 0 and len(oms) % 8 == 0, "A was meant to take the rectangular deal"
    run = wp.ThreeWays(scene)
    win = lambda w: run.window(DIFF, lims, w[0], w[1], w[2])

    def round_(first=(), second=()):
        run.option("cycle_samples", 32)
        for k, v in first:
            run.option(k, v)
        win(A)
        win(B)
        run.option("cycle_samples", 16)
        for k, v in second:
            run.option(k, v)
        win(A)   # a hit on a slot built for 32
        win(B)   # ... and one whose context has just built for 16

    round_()
    round_()
    for f_a, f_b in [(2, 0), (0, 1), (1, 2)]:
        round_([("fused_cycle", f_a)], [("fused_cycle", f_b)])
    for t_a, t_b in [(0, 1), (1, 0)]:
        round_([("device_trig", t_a)], [("device_trig", t_b)])
    run.option("device_trig", 1)
    # every step but the very first brings its tables back by a swap and builds its orders again for the other size
    assert run.classes == ["build", "build"] + ["hit"] * (4 * 7 - 2)
    assert run.counters() == (4 * 7 - 2, 4 * 7)
    assert run.mixed >= run.steps // 2
    run.finish()


def test_three_robot_types(scene):
    """Ackermann, differential drive and omni on one context, 80 steps of a random velocity walk around zero each: values
    cross |v| = kMinVel all the time, the omni rows are ragged and take the non-rectangular deal."""
    lims = wp.limits_pair(vx=(1.0, 1.0, 1.0), vy=(1.0, 1.0, 1.0), omega=(2.0, 2.0, 3.0, 3.0))   # windows of +-0.1 m/s
    run = wp.ThreeWays(scene, max_samples=4096)
    rng = np.random.default_rng(17)
    for ctr, L, A in ((ACK, 13, 5), (DIFF, 13, 5), (OMNI, 44, 3)):   # omni: 33 x 11, steps of 0.006 and 0.02 m/s
        first = len(run.keys)
        v = np.array([0.05, 0.0, 0.0])
        both_small = 0
        for _ in range(80):
            v += rng.normal(0.0, (0.012, 0.012 if ctr == OMNI else 0.0, 0.05))
            v = np.clip(v, (-0.06, -0.06, -0.5), (0.12, 0.06, 0.5))
            cur = (float(v[0]), float(v[1]), float(v[2]))
            run.window(ctr, lims, cur, L, A)
            xs, ys, _ = wp.window_axes(ctr, lims[1], cur, scene["dt"], L, A)
            both_small += any(abs(a) < wp.K_MIN_VEL for a in xs) and any(abs(a) < wp.K_MIN_VEL for a in ys)
        patterns = len(set(run.keys[first:]))
        print(f"three_robot_types: control type {ctr}: {patterns} patterns in 80 steps, {both_small} with small values on both axes")
        assert patterns >= 8
        assert ctr != OMNI or both_small >= 40
    count = run.model.count
    print(f"three_robot_types: same {count['same']}, hit {count['hit']}, build {count['build']}")
    assert count["hit"] >= 40 and run.counters() == (count["hit"], count["build"])
    run.finish()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("mode", [kh.SHARD_BLOCKS, kh.SHARD_ROWS])
def test_windows_under_shard_rules(scene, world, mode):
    """One context plays every rank in turn while the window alternates A, B, A, C, B: every share's tables come back
    from the store (by rows: a pattern of its own per rank; by blocks: one pattern whose orders belong to another
    rank's block).  The shares together are the oracle's cycle."""
    lim, ko_lim = wp.limits_pair()
    A, B, C = ((0.5, 0.0, 0.1), 9, 7), ((0.3, 0.0, -0.2), 11, 5), ((0.005, 0.0, 0.3), 9, 9)
    ctx = wp.make_context(scene)
    st, P = scene["state"], scene["P"]
    hits = 0
    for step, (cur, L, A_) in enumerate((A, B, A, C, B)):
        vx, vy, om = ko.sample_velocities(DIFF, ko_lim, cur, scene["dt"], L, A_)
        o = oracle_cycle(dict(scene, vx=vx, vy=vy, omega=om))
        assert 0 < len(o["raw"]) < len(vx)
        _, rows = np.unique(om + 0.0, return_inverse=True)
        owner = kh.shard_plan(rows, world, mode)
        raws, costs, keys = [], [], []
        for r in range(world):
            ctx.set_shard_rule(r, world, mode)
            if (step + r) % 2:
                res = ctx.find_best_path(st, P, window=(DIFF, lim, cur, L, A_))
            else:
                assert ctx.sample_window(DIFF, lim, cur, L, A_, want_list=False) == len(vx)   # the FULL window's count
                res = ctx.cycle(st, P)
            mine = np.nonzero(owner == r)[0]
            assert int(ctx.get_option("shard_samples")) == len(mine) == res.n_samples
            _, _, raw, c = ctx.get_samples(with_costs=True, with_paths=False)
            assert len(raw) == res.n_admissible and np.isin(raw, mine).all()
            raws.append(raw.copy())
            costs.append(c.copy())
            if res.found:
                keys.append(sharding.key_pack(res.cost, res.raw_index))
                k = int(np.nonzero(o["raw"] == res.raw_index)[0][0])
                bx, by, _ = ctx.get_best()
                np.testing.assert_array_equal(wp.bits(bx), wp.bits(o["px"][k]))
                np.testing.assert_array_equal(wp.bits(by), wp.bits(o["py"][k]))
        raw_all = np.concatenate(raws)
        order = np.argsort(raw_all, kind="stable")
        np.testing.assert_array_equal(raw_all[order], o["raw"])
        np.testing.assert_array_equal(wp.bits(np.concatenate(costs)[order]), wp.bits(o["costs"]))
        found, cost, raw_win = sharding.key_unpack(min(keys)) if keys else (False, 0.0, -1)
        assert found == (o["index"] >= 0)
        if found:
            assert raw_win == int(o["raw"][o["index"]]) and wp.bits(np.float32(cost)) == wp.bits(np.float32(o["cost"]))
            before = 0
            for r in range(world):
                ctx.set_shard_rule(r, world, mode)   # (the share of the window at hand, back from the store)
                ctx.rollout(st, P)
                before += ctx.count_admissible_before(raw_win)
            assert before == o["index"]
        hits, was = int(ctx.get_option("pattern_hits")), hits
        if step >= 2 and mode == kh.SHARD_ROWS:
            assert hits - was >= world, "every rank's share was meant to come back from the store"
    assert hits >= 1
    ctx.close()


def test_windows_past_the_lds_tables():
    """Windows with more axis values than the kernels keep in LDS (128 vx values, 64 vy values, 384 trig rows), each
    through the store twice with another window in between."""
    clipped = dict(vx=(130 / 256, 100.0, 100.0), omega=(2.0, 192 / 128, 100.0, 100.0))   # both limits cut the window: steps of 2^-7
    wide_x, wide_om = wp.limits_pair(vx=clipped["vx"]), wp.limits_pair(omega=clipped["omega"])
    plain = wp.limits_pair()
    other = (DIFF, plain, (0.5, 0.0, 0.1), 9, 7)
    dt = 0.1
    cases = [
        (wp.make_scene(), 2048, (DIFF, wide_x, (0.1, 0.0, 0.1), 131, 3), lambda xs, ys, oms: len(xs) == 131),
        (wp.make_scene(), 2048, (DIFF, wide_om, (0.5, 0.0, 0.1), 3, 385), lambda xs, ys, oms: len(oms) == 385),
        (wp.make_scene(P=4, state=(1.8, 0.4, -1.0, 0.0)), 16384, (OMNI, plain, (0.4, 0.1, 0.1), 261, 1), lambda xs, ys, oms: len(xs) > 128 and len(ys) + 1 > 64),
    ]
    for inp, max_samples, big, past in cases:
        assert past(*wp.window_axes(big[0], big[1][1], big[2], dt, big[3], big[4])), "the window was meant to pass a table bound"
        run = wp.ThreeWays(inp, max_samples=max_samples)
        for w in (big, other, big, other, big):
            a, _ = run.window(*w)
            assert 0 < a["n_admissible"] < a["n_samples"]
        assert run.classes == ["build", "build", "hit", "hit", "hit"]
        run.finish()
