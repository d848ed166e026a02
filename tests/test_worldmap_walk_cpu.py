"""The walk model and the walk generator on their own, without a device (tests/worldmap_walk_model.py):

  the model is consistent: along every default walk DistRef's lazily refreshed plane equals dist2_plane of the whole map at
  every call that reads it, and a replayed list gives the same results;

  the generator meets the coverage conditions for the default seeds: every kind at least three times a seed, refusals at
  most 15 %, trivial answers at most 25 % a reading kind, and the sequences (a) to (j) each somewhere in the default seeds;

  the walks tell a wrong implementation apart: six deliberately wrong variants of the model each give a differing result on
  at least two of the default seeds, which is what the device test would see of a host with that fault.

`python tests/test_worldmap_walk_cpu.py` prints each seed's histogram, refusals, sequences and model-only time."""
import collections
import time

import numpy as np
import pytest

import worldmap_walk_model as wk
from worldmap_walk_model import Refused, WalkModel, freeze, walk_config, walk_ops

SEEDS = wk.DEFAULT_SEEDS
READING = ("points", "scan", "movers", "mppi_step", "mcl_step")          # the kinds with a trivial answer
SEQUENCES = ("a", "b", "c", "d", "e", "f", "g:mcl_step", "g:mcl_resample", "g:mcl_resample_inject", "g:mcl_particles", "h", "i", "j")
MARK_ALL = ("set_prior", "clear", "set_model", "set_distance")


class _Checked(WalkModel):
    """WalkModel that compares the two planes at every read."""
    reads = 0

    def read_plane(self):
        out = super().read_plane()
        lazy, full = self.last_planes
        assert lazy.dtype == full.dtype == np.uint16 and lazy.tobytes() == full.tobytes(), (len(self.log), self._note["kind"])
        type(self).reads += 1
        return out


@pytest.fixture(scope="module")
def walks():
    """seed -> (ops, the model after them, the results, the model-only seconds): made once, left unchanged."""
    out = {}
    for seed in SEEDS:
        ops = walk_ops(seed)
        t = time.perf_counter()
        model, results = _Checked.replay(ops, walk_config(seed))
        out[seed] = (ops, model, results, time.perf_counter() - t)
    return out


def test_lazy_plane_is_the_whole_maps_plane_at_every_read(walks):
    assert _Checked.reads >= 6 * len(SEEDS)
    for seed, (ops, model, _, _) in walks.items():
        assert len(ops) == wk.DEFAULT_OPS == len(model.log)
        if model.dist is not None:                                        # and once more at the end
            model._note = {}
            model.read_plane()


def test_walks_are_functions_of_the_seed(walks):
    for seed, (ops, _, results, _) in walks.items():
        assert walk_ops(seed) == ops
        assert eval(repr(ops)) == ops                                     # the failure message's literal is the list
        _, again = WalkModel.replay(ops, walk_config(seed))
        assert freeze(again) == freeze(results), seed


def test_a_refused_operation_leaves_the_model_as_it_was(walks):
    """Each default walk with every refused operation taken out gives the same results for the rest."""
    n = 0
    for seed, (ops, _, results, _) in walks.items():
        kept = [i for i, r in enumerate(results) if not isinstance(r, Refused)]
        n += len(ops) - len(kept)
        _, again = WalkModel.replay([ops[i] for i in kept], walk_config(seed))
        assert freeze(again) == freeze([results[i] for i in kept]), seed
    assert n >= len(SEEDS)


def test_a_longer_walk_goes_on_freely():
    """Past its quotas a walk draws any kind that is ready, with the unhinted arguments; the model stays consistent."""
    ops = walk_ops(21, 240)
    assert ops[:wk.DEFAULT_OPS] == walk_ops(21)
    model, _ = _Checked.replay(ops, walk_config(21))
    tail = collections.Counter(op[0] for op in ops[wk.DEFAULT_OPS:])
    assert len(tail) >= 20 and tail["clear"] + tail["set_model"] >= 1 and tail["shift"] >= 3 and tail["set_distance"] >= 1
    assert sum(n["refused"] for n in model.log) <= 0.15 * len(ops)


# ---- the coverage conditions ----
def test_every_kind_three_times_a_seed(walks):
    for seed, (ops, _, _, _) in walks.items():
        hist = collections.Counter(op[0] for op in ops)
        assert set(hist) == set(wk.KINDS)
        assert min(hist.values()) >= 3, (seed, {k: v for k, v in hist.items() if v < 3})


def test_refusals_are_few_and_of_every_cause(walks):
    why = collections.Counter()
    for seed, (ops, model, results, _) in walks.items():
        refused = [i for i, r in enumerate(results) if isinstance(r, Refused)]
        assert len(refused) <= 0.15 * len(ops), (seed, len(refused))
        for i in refused:
            assert model.log[i]["refused"]
            why[(ops[i][0], results[i].error, model.log[i]["why"])] += 1

    def seen(kind, error, text):
        return any((kind is None or k == kind) and e == error and text in w for k, e, w in why)

    assert seen(None, "StateError", "distance plane is off"), why
    assert seen("mppi_step", "StateError", "c2 above the plane's reach^2"), why
    assert seen("movers", "StateError", "m2 above the plane's reach^2"), why
    assert seen("mcl_step", "StateError", "c2 above the plane's reach^2"), why           # the field model's reach
    assert seen("shift", "IndexError", "offset above 2^30 cells"), why
    assert seen(None, "IndexError", "2^20 cells"), why
    assert seen("mcl_step", "StateError", "init"), why


def trivial_share(model):
    """kind -> (trivial answers, answered calls): a refused call gives no answer and counts on neither side."""
    calls, trivial = collections.Counter(), collections.Counter()
    for n in model.log:
        if n["kind"] in READING and not n["refused"]:
            calls[n["kind"]] += 1
            trivial[n["kind"]] += int(bool(n.get("trivial")))
    return {k: (trivial[k], calls[k]) for k in READING}


def test_trivial_answers_are_rare(walks):
    for seed, (_, model, _, _) in walks.items():
        for kind, (t, c) in trivial_share(model).items():
            assert c >= 1 and t <= 0.25 * c, (seed, kind, t, c)


def argument_cases(ops, log):
    """The argument cases of the issue's list that a walk's answered calls contain: the histogram counts kinds alone."""
    found = set()
    n = len(ops)
    for i, (op, note) in enumerate(zip(ops, log)):
        if note["refused"]:
            continue
        kind = op[0]
        if kind == "shift":
            di, dj = op[1], op[2]
            found.add("shift (0, 0)" if (di, dj) == (0, 0) else "shift clearing" if abs(di) >= wk.W or abs(dj) >= wk.H
                      else "shift beyond 3 cells" if max(abs(di), abs(dj)) > 3 else "shift within 3 cells")
        if kind == "set_distance" and op[1] > 0:                          # a plane counts once it is read
            for k in range(i + 1, n):
                if log[k]["plane_read"]:
                    found.add(f"plane read at reach {op[1]}")
                    found.add(f"plane read with flags {op[2]}")
                    break
                if ops[k][0] == "set_distance" and not log[k]["refused"]:
                    break
        if kind == "points":
            found.add(f"points count_only {op[4]}")
        if kind == "scan":
            found.add(f"scan flags {op[3]}")
            found.add("scan of 65 beams" if op[2] == 65 else "scan of one beam" if op[2] == 1 else "scan")
            found.add(f"scan of {len(op[1])} poses")
        if kind == "integrate":
            found.add(f"integrate flags {op[4]}")
            if note.get("masked", 0) > 0:
                found.add("integrate with a skip mask")
        if kind == "update" and note.get("changed") == 0:
            found.add("update that changes nothing")
        if kind == "mcl_step":
            found.add("field step" if note["field"] else "beam step")
        if kind == "mcl_resample_inject":
            found.add("inject some" if op[1] > 0 else "inject none")
        if kind == "mppi_set_movers":
            found.add("movers set" if op[1] else "movers cleared")
        if kind == "mppi_set_costs":
            found.add(f"c2 {op[1]}")
        if kind == "mppi_set_team":
            found.add(f"team {op[1]}")
    return found


EVERY_WALK = ("plane read at reach 70", "plane read at reach 9", "plane read with flags 0", "plane read with flags 1", "field step",
              "beam step", "shift beyond 3 cells", "c2 16")
SOME_WALK = ("shift (0, 0)", "shift clearing", "shift within 3 cells", "plane read at reach 4", "points count_only 0", "points count_only 1",
             "scan flags 0", "scan flags 1", "scan of 65 beams", "scan of one beam", "scan of 1 poses", "scan of 3 poses", "integrate flags 0",
             "integrate flags 1", "integrate with a skip mask", "update that changes nothing", "inject some", "inject none",
             "movers set", "movers cleared", "c2 81", "team 1", "team 4", "team 8")


def test_argument_cases_occur(walks):
    found = {seed: argument_cases(ops, model.log) for seed, (ops, model, _, _) in walks.items()}
    for seed, f in found.items():
        assert not set(EVERY_WALK) - f, (seed, sorted(set(EVERY_WALK) - f))
    count = collections.Counter(c for f in found.values() for c in f)
    assert not [c for c in SOME_WALK if count[c] == 0], {c: count[c] for c in SOME_WALK}
    assert {walk_config(s)["N"] for s in SEEDS} == {65, 300} and {walk_config(s)["K"] for s in SEEDS} == {65, 257}


def overlap(a, b):
    return a[0] <= b[2] and b[0] <= a[2] and a[1] <= b[3] and b[1] <= a[3]


def sequences(ops, log):
    """The names of SEQUENCES a walk contains."""
    found = set()
    n = len(log)
    ok = [not x["refused"] for x in log]
    reads = [bool(x["plane_read"]) for x in log]
    moved = [ok[i] and log[i]["kind"] in ("shift", "recentre") and log[i].get("shift", (0, 0)) != (0, 0) for i in range(n)]
    clearing = [moved[i] and (abs(log[i]["shift"][0]) >= wk.W or abs(log[i]["shift"][1]) >= wk.H) for i in range(n)]
    changed = [ok[i] and log[i].get("changed", 0) > 0 for i in range(n)]

    def next_read(i, stop=()):
        """The first plane read after i, None when a kind of `stop` comes first."""
        for k in range(i + 1, n):
            if reads[k]:
                return k
            if ok[k] and log[k]["kind"] in stop:
                return None
        return None

    for i in range(n):
        kind = log[i]["kind"]
        if changed[i] and kind == "update":                               # (a)
            k = next_read(i, MARK_ALL)                                    # the shift alone marks the whole map
            if k is not None and any(moved[j] and not clearing[j] for j in range(i + 1, k)):
                found.add("a")
        if changed[i] and kind in ("update", "integrate"):                # (b): nothing in between marks the whole map
            k = next_read(i, MARK_ALL + ("shift", "recentre"))
            if k is not None:
                other = "integrate" if kind == "update" else "update"
                if any(changed[j] and log[j]["kind"] == other and not overlap(log[i]["box"], log[j]["box"]) for j in range(i + 1, k)):
                    found.add("b")
        if ok[i] and kind == "set_distance" and log[i]["reach"] == 0:    # (c)
            on = next((j for j in range(i + 1, n) if ok[j] and log[j]["kind"] == "set_distance"), None)
            if on is not None and log[on]["reach"] > 0 and next_read(on) is not None \
                    and any(ok[j] and log[j]["kind"] in wk.MUTATING for j in range(i + 1, on)):
                found.add("c")
        if clearing[i] and next_read(i, MARK_ALL + ("shift", "recentre")) is not None:   # (e): the clearing shift alone
            found.add("e")
        if i and reads[i] and reads[i - 1] and log[i]["refreshed"] is None:   # (f)
            found.add("f")
        if ok[i] and kind == "integrate" and log[i].get("masked", 0) > 0 and i and log[i - 1]["kind"] == "movers" and ok[i - 1]:
            found.add("j")
    up = any(ok[i] and log[i]["kind"] == "set_distance" and 0 < log[i]["reach_before"] <= 63 < log[i]["reach"] and log[i]["dirty_before"]
             for i in range(n))
    down = any(ok[i] and log[i]["kind"] == "set_distance" and 0 < log[i]["reach"] <= 63 < log[i]["reach_before"] and log[i]["dirty_before"]
               for i in range(n))
    if up and down:
        found.add("d")
    shifts, inited = 0, None                                              # (g) and (h)
    for i in range(n):
        kind = log[i]["kind"]
        if moved[i]:
            shifts += 1
        if ok[i] and kind in ("mcl_init_pose", "mcl_init_global"):
            shifts, inited = 0, i
        if ok[i] and kind in wk.MCL_ENTRIES:
            if shifts >= 2 and log[i]["followed"] != (0, 0):
                found.add("g:" + kind)
            shifts = 0
            if kind == "mcl_step":
                if inited is not None and any(ok[j] and log[j]["kind"] in ("set_prior", "clear") for j in range(inited + 1, i)):
                    found.add("h")
                inited = None
    sets = [i for i in range(n) if ok[i] and log[i]["kind"] == "set_distance"] + [n]      # (i)
    for a, b, c in zip(sets, sets[1:], sets[2:]):
        def both(lo, hi, refused):
            got = set()
            for j in range(lo + 1, hi):
                if log[j]["kind"] == "mppi_step" and log[j]["refused"] == refused and (not refused or ops[j][1][0] < 1 << 36):
                    got.add("mppi")
                if log[j]["kind"] == "mcl_step" and log[j].get("field") and log[j]["refused"] == refused:
                    got.add("mcl")
            return len(got) == 2
        if both(a, b, True) and both(b, c, False):
            found.add("i")
    return found


def test_named_sequences_occur(walks):
    found = {seed: sequences(ops, model.log) for seed, (ops, model, _, _) in walks.items()}
    missing = set(SEQUENCES) - set().union(*found.values())
    assert not missing, (sorted(missing), {s: sorted(f) for s, f in found.items()})


# ---- the wrong variants: what a faulty host would compute ----
class Replaces(WalkModel):
    """(1) the dirty box is replaced where it must be merged"""
    read_lazy = True

    def _mark(self, changed, box):
        if self.dist is not None and changed:
            self.dist.dirty = None
        super()._mark(changed, box)


class ShiftForgets(WalkModel):
    """(2) a shift does not mark the plane"""
    read_lazy = True

    def _mark_shift(self, di, dj):
        pass


class ClearingShiftForgets(WalkModel):
    """(2b) a shift that clears the whole window, which the host does on a path of its own, does not mark the plane"""
    read_lazy = True

    def _mark_shift(self, di, dj):
        if abs(di) < wk.W and abs(dj) < wk.H:
            super()._mark_shift(di, dj)


class KeepsBox(WalkModel):
    """(3) set_distance on, off, on keeps the box (and the plane) it had"""
    read_lazy = True

    def _new_dist(self, reach, flags):
        new, old = super()._new_dist(reach, flags), getattr(self, "kept", None)
        if new is not None and self.dist is None and old is not None:
            new.dirty, new.plane = old.dirty, old.plane.copy()
        self.kept = new or old
        return new


class LastShiftOnly(WalkModel):
    """(4) only the last pending shift reaches the particles"""

    def _pend(self, di, dj):
        self.pending = (di, dj)


class LeavesMarks(WalkModel):
    """(5) a refused integrate leaves its marks behind, for the next one to apply"""
    left = None

    def _refused_integrate(self, a):
        if a["flags"] & ~1:
            self.left = self.map.marks(a["pose"], a["angles"], a["zq"], a["range_max"], 0)[0]

    def _marks(self, marks):
        marks, self.left = (marks if self.left is None else marks | self.left), None
        return marks


class OldReach(WalkModel):
    """(6) the plane is refreshed with the reach it had before set_distance"""
    read_lazy = True

    def _new_dist(self, reach, flags):
        self.before = self.dist.reach if self.dist is not None else reach
        return super()._new_dist(reach, flags)

    def _refresh(self):
        now, self.dist.reach = self.dist.reach, self.before or self.dist.reach
        try:
            return super()._refresh()
        finally:
            self.dist.reach = now


VARIANTS = (Replaces, ShiftForgets, ClearingShiftForgets, KeepsBox, LastShiftOnly, LeavesMarks, OldReach)


def first_difference(a, b):
    fa, fb = freeze(a), freeze(b)
    return next((i for i in range(len(fa)) if fa[i] != fb[i]), None)


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: v.__name__)
def test_a_wrong_variant_is_told_apart_on_two_seeds(walks, variant):
    told = {}
    for seed, (ops, _, results, _) in walks.items():
        _, got = variant.replay(ops, walk_config(seed))
        at = first_difference(results, got)
        if at is not None:
            told[seed] = (at, ops[at][0])
    assert len(told) >= 2, told
    if variant.read_lazy:                                                 # distance-plane state alone: a plane reader's result differs
        assert all(kind in ("distance", "movers", "mppi_step", "mcl_step") for _, kind in told.values()), told


def test_the_lazy_model_itself_gives_the_same_results(walks):
    """read_lazy alone changes nothing: the variants above differ by their fault, not by which plane they read."""
    class Lazy(WalkModel):
        read_lazy = True
    for seed, (ops, _, results, _) in walks.items():
        assert first_difference(results, Lazy.replay(ops, walk_config(seed))[1]) is None


def report():
    for seed in SEEDS:
        ops = walk_ops(seed)
        t = time.perf_counter()
        model, results = WalkModel.replay(ops, walk_config(seed))
        dt = time.perf_counter() - t
        hist = collections.Counter(op[0] for op in ops)
        refused = collections.Counter((ops[i][0], r.error) for i, r in enumerate(results) if isinstance(r, Refused))
        print(f"seed {seed}: {walk_config(seed)}  model-only {dt:.2f} s  refusals {sum(refused.values())}")
        print("  histogram", " ".join(f"{k}:{hist[k]}" for k in wk.KINDS))
        print("  refused", dict(refused))
        print("  trivial", trivial_share(model))
        print("  sequences", " ".join(sorted(sequences(ops, model.log))))
        print("  cases", "; ".join(sorted(argument_cases(ops, model.log))))
        told = [v.__name__ for v in VARIANTS if first_difference(results, v.replay(ops, walk_config(seed))[1]) is not None]
        print("  variants told apart", " ".join(told))


if __name__ == "__main__":
    report()
