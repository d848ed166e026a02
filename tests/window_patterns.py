"""Drivers of tests/test_window_patterns_gpu.py: one small scene, a plain model of the kept-pattern rule, and a
runner that takes every step three ways.

The scene.  cfg2's "mid" costmap cut to the points within 4 m of a robot that stands at the edge of the clutter, the
straight tracked segment, P = 10 poses: a horizon of one second, in which the faster samples of a window reach the
clutter and the slower ones do not (0 < admissible < n for the windows the tests draw).

The model (point 11; csrc/kc_sample_pattern.h find_pattern, carried out by upload_samples / build_perm in
csrc/kc_dwa.hip).  A context holds one
ACTIVE set of index tables and walking orders and keeps those of up to pattern_slots(n) earlier window patterns, a
pattern being (signature, sample count).  A window whose pattern is the active one changes nothing ("same").  One
found among the kept patterns changes places with the active one ("hit", counter pattern_hits).  Any other one
("miss") moves the active pattern into an empty slot, a new slot or, when there is neither, the slot that was put
away longest ago, and builds its tables anew.  Explicit lists have no signature: they are never kept, they overwrite
the active tables, and a window after one finds nothing active worth keeping -- on a hit the slot then empties.  The
walking orders belong to (first sample, sample count, samples per workgroup) of the share that was rolled out: a
cycle that finds other ones builds them again (counter pattern_builds), whatever brought the tables back."""
from __future__ import annotations

import numpy as np

import kompass_hip as kh
import synthetic as syn
from helpers import oracle_cycle
from oracle import ko

P_SMALL = 10
STATE = (1.9, 0.8, 0.3, 0.0)


def make_scene(P=P_SMALL, state=STATE, radius=4.0):
    inp = syn.make_controller_inputs("cfg2", seed=2, scale=0.2, scene="mid")
    pts = np.asarray(inp["points"], np.float32)
    near = np.hypot(pts[:, 0] - np.float32(state[0]), pts[:, 1] - np.float32(state[1])) < radius
    inp.update(P=P, state=state, points=np.ascontiguousarray(pts[near]),
               seg_xyz=np.ascontiguousarray(inp["seg_xyz"], np.float32),
               acc_at_seg=np.ascontiguousarray(inp["acc_at_seg"], np.float32))
    return inp


def limits_pair(vx=syn.LIMITS["vx"], vy=syn.LIMITS["vy"], omega=syn.LIMITS["omega"]):
    """The same limits for the library and for the oracle."""
    return kh.make_limits(vx, vy, omega), ko.make_limits(vx, vy, omega)


def pattern_slots(n):
    """128 MB over 40 bytes a sample and pattern, held between 16 and 256 (tests/native/launch_plan.cpp pins the rule)."""
    return min(256, max(16, (128 << 20) // (40 * max(n, 1))))


K_MIN_VEL = 0.01


def window_axes(ctr, lim, cur, dt, max_lin, max_ang):
    """The three axes of a window by the sampler's plain rules (counts by the split and odd rules, limits clipped to the
    reachable range, a step of range / (count - 1) held above 0.001, values by repeated addition) -> (xs, ys, oms)
    with ys empty unless omni.  `lim` is either Limits structure.  expand_axes() of them is checked against the oracle's
    list wherever the tests use them, so an error here cannot hide one of the library."""
    odd = lambda k: k + 1 if k % 2 == 0 else k
    lo = lambda a, b: b if b < a else a
    hi = lambda a, b: b if a < b else a
    omni = int(ctr) == ko.OMNI
    nx = odd(max(3, max_lin * 3 // 4)) if omni else odd(max(3, max_lin))
    ny = odd(max(3, max_lin // 4)) if omni else 1
    na = max_ang + 1 - (max_ang % 2)

    def axis(vmax, acc, dec, c, count):
        top, bottom = lo(vmax, c + acc * dt), hi(-vmax, c - dec * dt)
        if count > 1:
            step = hi((top - bottom) / (count - 1), 0.001)
        else:  # x / 0 in IEEE arithmetic: inf, or NaN from 0 / 0 -- one value either way
            step = float("nan") if top == bottom else float("inf")
        out, v = [], bottom
        while v <= top:
            out.append(v)
            v += step
        return out

    xs = axis(lim.vx_max, lim.vx_acc, lim.vx_dec, cur[0], nx)
    ys = axis(lim.vy_max, lim.vy_acc, lim.vy_dec, cur[1], ny) if omni else []
    oms = axis(lim.omega_max, lim.omega_acc, lim.omega_dec, cur[2], na)
    return xs, ys, oms


def expand_axes(ctr, xs, ys, oms):
    """The sample list of the axes in generation order: per vx the (vx, vy, 0) samples of an omni robot, then the
    (vx, 0, omega) samples unless vx is small; a sample of three small values is never made."""
    small = lambda v: abs(v) < K_MIN_VEL
    out = []
    for v in xs:
        for w in ys:
            if not (small(v) and small(w)):
                out.append((v, w, 0.0))
        if not small(v):
            out.extend((v, 0.0, o) for o in oms)
    return np.array(out, np.float64).reshape(-1, 3)


def pattern_key(ctr, xs, ys, oms):
    """What decides a window's index pattern: omni or not, the length of each axis, and which axis values are small."""
    small = lambda a: tuple(i for i, v in enumerate(a) if abs(v) < K_MIN_VEL)
    return (int(ctr) == ko.OMNI, len(xs), len(ys), len(oms), small(xs), small(ys))


def list_labels(vx, vy, om):
    """What decides whether an explicit list equals the active one: per sample, which distinct value of each axis it
    takes, in order of first appearance (bit patterns; -0.0 and +0.0 of an omega are one row)."""
    def ranks(a):
        seen = {}
        return tuple(seen.setdefault(v, len(seen)) for v in np.ascontiguousarray(a, np.float64).view(np.uint64).tolist())
    return (ranks(vx), ranks(vy), ranks(np.asarray(om, np.float64) + 0.0))


class PatternModel:
    """The kept-pattern rule, restated plainly (module docstring).  `kept` is ordered by when a pattern was put away."""

    def __init__(self):
        self.active = None      # key of the active window pattern; None: nothing, or an explicit list
        self.orders = {}        # key -> (first, count, samples per workgroup) its walking orders were built for
        self.list_orders = None  # the same for an active explicit list
        self.list_labels = None  # list_labels of the explicit list whose tables are active
        self.kept = []          # keys, oldest first
        self.slots = 0          # slots ever made (an emptied one is used again before a new one is made)
        self.count = dict(same=0, hit=0, build=0, lru=0)

    def window(self, key, n):
        """A window of pattern `key` with n > 0 samples arrives -> 'same' | 'hit' | 'build' (= miss)."""
        self.list_orders = self.list_labels = None
        if key == self.active:
            what = "same"
        elif key in self.kept:
            self.kept.remove(key)
            if self.active is not None:
                self.kept.append(self.active)
            what = "hit"
        else:
            if self.active is not None:
                if len(self.kept) < self.slots:
                    pass                                   # an empty slot
                elif self.slots < pattern_slots(n):
                    self.slots += 1
                else:
                    self.orders.pop(self.kept.pop(0), None)  # the one put away longest ago
                    self.count["lru"] += 1
                self.kept.append(self.active)
            self.orders.pop(key, None)
            what = "build"
        self.active = key
        self.count[what] += 1
        return what

    def explicit_list(self, labels, n):
        """An explicit list of n samples arrives (labels: list_labels of it)."""
        if n == 0:   # nothing is uploaded; whatever is active stays, but its walking orders are built again
            if self.active is not None:
                self.orders.pop(self.active, None)
            self.list_orders = None
            return
        if self.active is None and labels == self.list_labels:
            return   # the active list, vector by vector: only the value tables are rewritten
        if self.active is not None:   # the window's tables are overwritten, not kept
            self.orders.pop(self.active, None)
            self.active = None
        self.list_labels = labels
        self.list_orders = None

    def cycle(self, first, count, cs):
        """A cycle rolls out `count` > 0 samples from `first` in workgroups of cs -> 1 when it has to build the orders."""
        want = (first, count, cs)
        have = self.orders.get(self.active) if self.active is not None else self.list_orders
        if have == want:
            return 0
        if self.active is not None:
            self.orders[self.active] = want
        else:
            self.list_orders = want
        return 1


def make_context(inp, max_samples=2048, **options):
    rb = inp["robot"]
    c = kh.DwaContext(rb["shape"], rb["dims"], (0, 0, 0), (0, 0, 0, 1), inp["octree_res"], inp["dt"], max_samples=max_samples,
                      max_points=inp["P"], max_segment=len(inp["seg_xyz"]), max_obstacles=max(len(inp["points"]), 16),
                      acc_limits=inp["acc_limits"])
    for k, v in options.items():
        c.set_option(k, v)
    c.set_weights(kh.make_weights(*inp["weights"]))
    c.set_points(inp["state"], inp["points"], inp["max_range"])
    c.set_tracked_segment(inp["seg_xyz"], inp["acc_at_seg"], inp["ref_len"])
    return c


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def read_cycle(ctx, res):
    """Everything a cycle left: the record, the winner's row, the admissible ids and every cost."""
    best = ctx.get_best() if res.found else None
    _, _, raw, costs = ctx.get_samples(with_costs=True, with_paths=False)
    return dict(n_samples=int(res.n_samples), n_admissible=int(res.n_admissible), found=bool(res.found), index=int(res.index),
                raw_index=int(res.raw_index), cost=np.float32(res.cost), raw=raw.copy(), costs=costs.copy(),
                bx=None if best is None else best[0].copy(), by=None if best is None else best[1].copy())


def assert_same_cycle(a, b, what):
    assert (a["n_samples"], a["n_admissible"], a["found"]) == (b["n_samples"], b["n_admissible"], b["found"]), what
    np.testing.assert_array_equal(a["raw"], b["raw"], err_msg=what)
    np.testing.assert_array_equal(bits(a["costs"]), bits(b["costs"]), err_msg=what)
    if a["found"]:
        assert (a["index"], a["raw_index"]) == (b["index"], b["raw_index"]), what
        assert bits(a["cost"]) == bits(b["cost"]), what
        np.testing.assert_array_equal(bits(a["bx"]), bits(b["bx"]), err_msg=what)
        np.testing.assert_array_equal(bits(a["by"]), bits(b["by"]), err_msg=what)


def assert_oracle_cycle(o, a, what):
    assert a["n_admissible"] == len(o["raw"]), what
    np.testing.assert_array_equal(a["raw"], o["raw"], err_msg=what)
    np.testing.assert_array_equal(bits(a["costs"]), bits(o["costs"]), err_msg=what)
    assert a["found"] == (o["index"] >= 0), what
    if a["found"]:
        assert (a["index"], a["raw_index"]) == (o["index"], int(o["raw"][o["index"]])), what
        assert bits(a["cost"]) == bits(np.float32(o["cost"])), what
        np.testing.assert_array_equal(bits(a["bx"]), bits(o["px"][o["index"]]), err_msg=what)
        np.testing.assert_array_equal(bits(a["by"]), bits(o["py"][o["index"]]), err_msg=what)


class ThreeWays:
    """Every step on (1) `win`, the long-lived context under test, which gets windows; (2) `lst`, a long-lived context
    that only ever gets the oracle's list of the same window (no signature, never kept: it cannot share an error of the
    pattern store); (3) on the first step, every 16th and -- finish() -- the last, through oracle_cycle on that list.
    After every step the two counters of `win` must have moved as the model says."""

    def __init__(self, inp, max_samples=2048, **options):
        self.inp = inp
        self.win = make_context(inp, max_samples, **options)
        self.lst = make_context(inp, max_samples, **options)
        self.model = PatternModel()
        self.steps = 0
        self.mixed = 0          # steps with 0 < admissible < n
        self.oracle_steps = 0
        self.keys = []          # pattern key of every window step
        self.classes = []       # 'same' | 'hit' | 'build' of every window step
        self._last = None
        self._counters = self.counters()

    def option(self, name, value):
        self.win.set_option(name, value)
        self.lst.set_option(name, value)

    def counters(self):
        return int(self.win.get_option("pattern_hits")), int(self.win.get_option("pattern_builds"))

    def _oracle(self, lists, got, what):
        vx, vy, om = lists
        o = oracle_cycle(dict(self.inp, vx=vx, vy=vy, omega=om))
        assert_oracle_cycle(o, got, what + " (oracle)")
        self.oracle_steps += 1

    def _finish_step(self, lists, res, hit, what):
        st, P = self.inp["state"], self.inp["P"]
        n = len(lists[0])
        a = read_cycle(self.win, res)
        # the counters against the model: a hit is counted when the tables change places, a build when the cycle
        # finds no walking orders for (first sample, count, samples per workgroup)
        builds = self.model.cycle(0, n, int(self.win.get_option("last_cycle_samples"))) if n else 0
        now = self.counters()
        moved = (now[0] - self._counters[0], now[1] - self._counters[1])
        self._counters = now
        assert moved == (int(hit), builds), f"{what}: pattern_hits / pattern_builds moved by {moved}, the model says {(int(hit), builds)}"
        self.lst.set_samples(*lists)
        b = read_cycle(self.lst, self.lst.cycle(st, P))
        assert a["n_samples"] == n, what
        assert_same_cycle(a, b, what)
        self.mixed += 0 < a["n_admissible"] < a["n_samples"]
        if self.steps % 16 == 0:
            self._oracle(lists, a, what)
            self._last = None
        else:
            self._last = (lists, a, what)
        self.steps += 1
        return a

    def window(self, ctr, lims, cur, L, A, how=None):
        """One window through `win`: how = 'find' (kc_dwa_find_best_path), 'list' / 'count' (kc_dwa_sample_window with or
        without the list coming back, then kc_dwa_cycle); None: by turns.  -> (what the cycle left, the oracle's list)"""
        lim, ko_lim = lims
        how = how or ("find", "list", "count")[self.steps % 3]
        st, P = self.inp["state"], self.inp["P"]
        what = f"step {self.steps}: window {ctr} {tuple(cur)} {L} x {A} by {how}"
        lists = ko.sample_velocities(ctr, ko_lim, cur, self.inp["dt"], L, A)
        axes = window_axes(ctr, ko_lim, cur, self.inp["dt"], L, A)
        mine = expand_axes(ctr, *axes)
        for k in range(3):   # the axes the pattern key is read from are the oracle's
            np.testing.assert_array_equal(np.ascontiguousarray(mine[:, k]).view(np.uint64), lists[k].view(np.uint64), err_msg=what)
        n = len(lists[0])
        assert n > 0, what
        key = pattern_key(ctr, *axes)
        klass = self.model.window(key, n)
        self.keys.append(key)
        self.classes.append(klass)
        if how == "find":
            res = self.win.find_best_path(st, P, window=(ctr, lim, cur, L, A))
        else:
            if how == "list":
                got = self.win.sample_window(ctr, lim, cur, L, A)
                for g, o in zip(got, lists):
                    np.testing.assert_array_equal(g.view(np.uint64), o.view(np.uint64), err_msg=what)
            else:
                assert self.win.sample_window(ctr, lim, cur, L, A, want_list=False) == n, what
            res = self.win.cycle(st, P)
        return self._finish_step(lists, res, klass == "hit", what + " (" + klass + ")"), lists

    def explicit(self, vx, vy, om):
        """An explicit list through `win` as well (between windows)."""
        st, P = self.inp["state"], self.inp["P"]
        lists = tuple(np.ascontiguousarray(a, np.float64) for a in (vx, vy, om))
        self.model.explicit_list(list_labels(*lists), len(lists[0]))
        self.win.set_samples(*lists)
        res = self.win.cycle(st, P)
        return self._finish_step(lists, res, False, f"step {self.steps}: explicit list of {len(lists[0])}")

    def finish(self):
        if self._last is not None:
            self._oracle(*self._last)
        self.win.close()
        self.lst.close()
