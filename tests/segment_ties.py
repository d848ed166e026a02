"""Scenes on which the search of the tracked segment has to DECIDE something, and a plain statement of what it
must find (not collected: the CPU and GPU tests of the same name import it).

The cost kernels replace the reference's full scan of the tracked segment (pathCostFunc / goalCostFunc,
cost_evaluator.cpp:111-177) with pruned searches whose contract is "the same minimum and the same LOWEST index as
the full scan": the goal cost reads acc[argmin], and two segment points at the same squared distance can be a whole
path length apart in acc.  Here every scene is built from dyadic rationals, so float32 holds every coordinate and
every difference exactly and equal distances are equal bits:

  tie scenes       closed_square, closed_small17 / 33, hairpin_bisector, hairpin_even, lattice_zigzag: end points with
                   2 to 4 exact minima whose acc values differ (a wrong pick changes the goal cost by more than 1e-3);
  circle_centre    float32 of (2 cos, 2 sin): the centre has many FLOAT minima scattered through every chunk (the one
                   scene whose ties are rounding accidents; its two controls have one minimum each);
  zero chords      stationary_run40 / 128 (a whole chunk / a whole super-chunk is one point: both table builders
                   store inv = 0 for its chord; the tied points share one acc value, so these are not tie scenes in
                   the sense above) and `degenerate` (S = 1, 2, 3 of one point: the segment's length is 0).

Variants: z = -0.0 everywhere (not "flat" for the kernels, every distance unchanged), z = 0.5 everywhere, the
hairpin with one leg lifted so that z makes the tie, and the flat scenes shifted by (4096, -2048) and
(-12288, 8192): coordinates and ties stay exact, the pruning slacks and the near table's cell arithmetic see large
magnitudes.  (Not so the circle: shifted, or with z = 0.5, its distances round anew and other, fewer points tie.)

path_goal_np is written from cost_evaluator.cpp's arithmetic in numpy float32 and shares nothing with
oracle/kompass_oracle.c; exact_ties counts the true geometric minima in integer arithmetic.
"""
from __future__ import annotations

import numpy as np

F = np.float32
PS = (2, 5, 64, 65, 130)          # trajectory lengths, cycled over the end points of a scene
WEIGHTINGS = ((1.0, 0.0), (0.0, 1.0), (0.7, 1.3))   # (path, goal); every other weight 0
OFFSETS = ((4096.0, -2048.0), (-12288.0, 8192.0))
STEP = 1.0 / 64.0


# ---------------------------------------------------------------------------
# the kernels' chunk rule (what "different chunks" means in the CPU conditions)
# ---------------------------------------------------------------------------
def chunk_of(S: int) -> int:
    """Points per chunk: at least 16, at most 64 chunks, even."""
    return (max(16, (S + 63) // 64) + 1) & ~1


def super_of(S: int) -> int:
    return 8 * chunk_of(S)


# ---------------------------------------------------------------------------
# the plain statement
# ---------------------------------------------------------------------------
def _d2(seg, x, y):
    """(q - p).squaredNorm() of Vector3f with p.z = 0: dx*dx + (dy*dy + dz*dz), float32.  seg (S, 3); x, y (...)."""
    x, y = np.asarray(x, F), np.asarray(y, F)
    dx = seg[:, 0] - x[..., None]
    dy = seg[:, 1] - y[..., None]
    dz = seg[:, 2] - F(0.0)
    return dx * dx + (dy * dy + dz * dz)


def segment_length_np(seg):
    """View::totalSegmentLength, path.h:85-91: float32 sum of the edge lengths in index order."""
    if len(seg) < 2:
        return F(0.0)
    d = seg[:-1] - seg[1:]
    e = np.sqrt(d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))
    return np.cumsum(e, dtype=F)[-1]          # (cumsum adds sequentially; sum would add pairwise)


def path_goal_np(seg, acc, ref_len, px, py):
    """pathCostFunc and goalCostFunc by brute force.  -> path[N], goal[N] float32, argmin[N], n_minima[N] (the
    last two for the end point)."""
    seg = np.asarray(seg, F).reshape(-1, 3)
    acc = np.asarray(acc, F)
    px, py = np.asarray(px, F), np.asarray(py, F)
    N, P = px.shape
    L = F(ref_len)
    seg_len = segment_length_np(seg)
    path, goal = np.zeros(N, F), np.zeros(N, F)
    arg, cnt = np.zeros(N, np.int64), np.zeros(N, np.int64)
    with np.errstate(all="ignore"):
        for n in range(N):
            d2 = _d2(seg, px[n], py[n])                        # (P, S)
            mind = np.sqrt(d2.min(axis=1))                     # one sqrt per point (sqrt is monotonic)
            total = np.cumsum(mind, dtype=F)[-1]               # sequential, in point order
            e = d2[-1]
            end_err = np.sqrt(e[-1]) / seg_len
            path[n] = (total / F(P) + end_err) / F(2.0)
            j = int(np.argmin(e)) if (e < np.finfo(F).max).any() else 0   # first minimum; nothing below FLT_MAX: 0
            arg[n] = j
            cnt[n] = int((e == e[j]).sum())
            goal[n] = (L - acc[j]) / L + np.sqrt(e[j]) / L
    return path, goal, arg, cnt


def totals_np(path, goal, w_path, w_goal, ref_len):
    """cost_evaluator.cpp:59-74: the goal term first, each += a double multiply-add rounded into the float."""
    total = np.zeros(len(path), F)
    if F(ref_len) > 0:
        with np.errstate(all="ignore"):
            if w_goal > 0.0:
                total = (total.astype(np.float64) + w_goal * goal.astype(np.float64)).astype(F)
            if w_path > 0.0:
                total = (total.astype(np.float64) + w_path * path.astype(np.float64)).astype(F)
    return total


def select_np(costs):
    """cost_evaluator.cpp:102-106: first cost strictly below FLT_MAX-so-far; -1 when none is (NaN, inf)."""
    best, idx = np.finfo(F).max, -1
    for n, c in enumerate(costs):
        if c < best:
            best, idx = c, n
    return idx, F(best)


def minima_np(seg, x, y):
    """Indices of the float32 minima of the squared distance from (x, y, 0)."""
    e = _d2(np.asarray(seg, F).reshape(-1, 3), F(x), F(y))
    return set(np.flatnonzero(e == e.min()).tolist())


def exact_ties(seg, x, y):
    """Indices of the true geometric minima: every coordinate times a power of two is an integer, the squared
    distances are Python ints."""
    seg = np.asarray(seg, F).reshape(-1, 3)
    vals = [float(v) for v in seg.ravel()] + [float(F(x)), float(F(y))]
    den = max(v.as_integer_ratio()[1] for v in vals)

    def scaled(v):
        n, d = float(v).as_integer_ratio()
        return n * (den // d)

    X, Y = scaled(F(x)), scaled(F(y))
    d2 = [(scaled(p[0]) - X) ** 2 + (scaled(p[1]) - Y) ** 2 + scaled(p[2]) ** 2 for p in seg]
    m = min(d2)
    return {j for j, v in enumerate(d2) if v == m}


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------
def _acc(xyz):
    d = np.diff(np.asarray(xyz, np.float64), axis=0)
    return np.concatenate([[0.0], np.cumsum(np.sqrt((d * d).sum(axis=1)))]).astype(F)


class Scene:
    """seg (S, 3) float32, acc (S,) float32, ref_len, ends = [(x, y, (ax, ay))]: the end points with the direction
    (in steps of 1/64) of the third approach.  kind: "tie", "circle", "zero", "degenerate"."""

    def __init__(self, name, seg, ends, kind, ref_len=None, acc=None, rot=0, far_super=False):
        self.name = name
        self.seg = np.ascontiguousarray(seg, F).reshape(-1, 3)
        self.acc = _acc(self.seg) if acc is None else np.asarray(acc, F)
        self.ref_len = float(self.acc[-1]) if ref_len is None else float(ref_len)
        self.ends = list(ends)
        self.kind = kind
        self.rot = rot
        self.far_super = far_super      # the ties of some end point lie in different super-chunks
        self.S = len(self.seg)
        self._stacks = None

    # -- variants ---------------------------------------------------------------
    def with_z(self, z, tag):
        seg = self.seg.copy()
        seg[:, 2] = F(z)
        return Scene(f"{self.name}-{tag}", seg, self.ends, self.kind, self.ref_len, self.acc, self.rot + 1,
                     self.far_super)

    def shifted(self, dx, dy, tag):
        seg = self.seg.copy()
        seg[:, 0] += F(dx)
        seg[:, 1] += F(dy)
        ends = [(x + dx, y + dy, a) for x, y, a in self.ends]
        return Scene(f"{self.name}-{tag}", seg, ends, self.kind, self.ref_len, self.acc, self.rot + 3, self.far_super)

    # -- trajectories -----------------------------------------------------------
    def stacks(self):
        """[(px, py)] one stack per trajectory length: for every end point a constant trajectory, an approach along
        +x and an approach along the end point's own direction, all in steps of 1/64.  The trajectory that the
        statement selects under the weighting (0.7, 1.3) is never the first of its stack."""
        if self._stacks is not None:
            return self._stacks
        by_p = {}
        for i, (ex, ey, (ax, ay)) in enumerate(self.ends):
            P = PS[(i + self.rot) % len(PS)]
            back = np.arange(P - 1, -1, -1, dtype=np.float64) * STEP
            rows = by_p.setdefault(P, [])
            for ux, uy in ((0.0, 0.0), (1.0, 0.0), (ax, ay)):
                rows.append((ex - back * ux, ey - back * uy))
        out = []
        for P in sorted(by_p):
            px = np.stack([r[0] for r in by_p[P]])
            py = np.stack([r[1] for r in by_p[P]])
            assert (px.astype(F) == px).all() and (py.astype(F) == py).all(), "a trajectory point is not a float32"
            px, py = px.astype(F), py.astype(F)
            assert len(px) <= 64
            for _ in range(len(px)):     # (rows of equal cost: the first of them is selected, so roll again)
                path, goal, _, _ = path_goal_np(self.seg, self.acc, self.ref_len, px, py)
                if select_np(totals_np(path, goal, 0.7, 1.3, self.ref_len))[0] != 0:
                    break
                px, py = np.roll(px, 1, axis=0), np.roll(py, 1, axis=0)
            out.append((np.ascontiguousarray(px), np.ascontiguousarray(py)))
        self._stacks = out
        return out


def closed_square(n_side=128, name="closed_square"):
    """A closed loop on the 1/16 grid: first point == last point."""
    h = 1.0 / 16.0
    side = n_side * h
    k = np.arange(n_side, dtype=np.float64) * h
    z = np.zeros(n_side)
    xs = np.concatenate([k, z + side, side - k, z, [0.0]])
    ys = np.concatenate([z, k, z + side, side - k, [0.0]])
    seg = np.stack([xs, ys, np.zeros_like(xs)], 1)
    ends = [(0.0, 0.0, (1.0, 1.0)),                  # the start corner: indices 0 and 4 n
            (h / 2, 0.0, (1.0, 0.0)),                # 1/32 along the first side: 0, 1, 4 n
            (0.0, h / 2, (0.0, 1.0)),                # 1/32 along the last side: 0, 4 n - 1, 4 n
            (side / 2, side / 2, (1.0, 1.0)),        # the centre: the four side mid-points
            (side, side, (1.0, 1.0)),                # the far corner: one minimum
            (-1.0, -1.0, (1.0, 1.0))]                # outside: 0 and 4 n
    return Scene(name, seg, ends, "tie", far_super=n_side == 128)


def hairpin_bisector(lift=False):
    """Out along y = 0, back along y = 0.5, 400 points each on the 1/64 grid; queries on the bisector y = 0.25.
    lift: legs at (y = 0, z = 0.5) and (y = 0.5, z = 0), queries on y = 0: z makes the tie."""
    k = np.arange(400, dtype=np.float64) * STEP
    leg1 = np.stack([k, np.zeros(400), np.full(400, 0.5 if lift else 0.0)], 1)
    leg2 = np.stack([k[::-1], np.full(400, 0.5), np.zeros(400)], 1)
    seg = np.concatenate([leg1, leg2])
    yq = 0.0 if lift else 0.25
    # (the approach along +x is the one along the bisector; the third comes in across the first leg)
    ends = [(-0.5, yq, (1.0, 1.0)),                  # below the segment: 0 and 799
            (200 * STEP, yq, (1.0, 1.0)),            # the middle
            (160 * STEP, yq, (-1.0, 1.0)),           # at a chunk head of the first leg
            (159 * STEP, yq, (1.0, 1.0)),            # one before it
            (7.0, yq, (-1.0, 1.0))]                  # beyond the far end: 399 and 400
    return Scene("hairpin_lifted" if lift else "hairpin_bisector", seg, ends, "tie", far_super=True)


def hairpin_even():
    """The hairpin with the return leg one step further out: x = m / 64 lies at index m of the first leg and at
    index 800 - m of the second.  For m = 8 (mod 16) both tied indices are even, no chunk head, and 16 apart modulo
    16: in a search that deals the pair records of a chunk over eight (or four) lanes, ONE lane meets both, the
    lower first, and no other lane holds the minimum -- only that lane's own tie rule decides.  m = 4 (mod 8)
    does the same for four lanes."""
    k = np.arange(400, dtype=np.float64) * STEP
    leg1 = np.stack([k, np.zeros(400), np.zeros(400)], 1)
    leg2 = np.stack([(400 - np.arange(400)) * STEP, np.full(400, 0.5), np.zeros(400)], 1)
    ends = [(120 * STEP, 0.25, (1.0, 1.0)),          # 120 and 680: both 8 (mod 16)
            (196 * STEP, 0.25, (-1.0, 1.0)),         # 196 and 604: both 4 (mod 8)
            (200 * STEP, 0.25, (1.0, 1.0)),          # 200 and 600
            (-0.5, 0.25, (1.0, 1.0)),                # below: index 0 alone
            (7.0, 0.25, (-1.0, 1.0))]                # beyond: index 400 alone
    return Scene("hairpin_even", np.concatenate([leg1, leg2]), ends, "tie", far_super=True)


def circle_centre():
    th = 2.0 * np.pi * np.arange(1000, dtype=np.float64) / 1000.0
    seg = np.stack([(2.0 * np.cos(th)).astype(F), (2.0 * np.sin(th)).astype(F), np.zeros(1000, F)], 1)
    e = 2.0 ** -10
    ends = [(0.0, 0.0, (1.0, 1.0)), (e, e, (0.0, 1.0)), (-e, e, (1.0, 1.0))]
    return Scene("circle_centre", seg, ends, "circle", far_super=True)


def stationary_run(S, first, count, name):
    """A straight path on the 1/16 grid that stands still for `count` points from index `first`."""
    idx = np.arange(S)
    steps = np.where((idx > first) & (idx < first + count), 0, 1)
    steps[0] = 0
    x = np.cumsum(steps).astype(np.float64) / 16.0
    seg = np.stack([x, np.zeros(S), np.zeros(S)], 1)
    xr = float(x[first])
    ends = [(xr, 0.0, (0.0, 1.0)),                   # on the run
            (xr, 0.5, (1.0, 1.0)),                   # beside it
            (-3.0, 2.0, (1.0, -1.0)),                # far from it
            (xr + 1.0 / 32.0, 0.0, (0.0, 1.0))]      # between the run and the next point
    return Scene(name, seg, ends, "zero")


def lattice_zigzag():
    """A staircase on the integer grid, two steps along x and one along y: index 3 s + t is (2 s + t, s)."""
    j = np.arange(257)
    s, t = j // 3, j % 3
    seg = np.stack([2.0 * s + t, 1.0 * s, np.zeros(257)], 1)
    ends = [(0.5, 0.5, (1.0, 1.0)),                  # cell A_0: indices 0, 1
            (10.5, 5.5, (1.0, 1.0)),                 # A_5: 15, 16 (two chunks)
            (85.5, 42.5, (0.0, 1.0)),                # B_42: 127, 128, 129 (two super-chunks)
            (41.5, 20.5, (1.0, -1.0)),               # B_20: 61, 62, 63
            (30.0, 40.0, (1.0, 1.0))]                # off the stair: one minimum
    return Scene("lattice_zigzag", seg, ends, "tie")


def degenerate(S):
    seg = np.tile(np.array([[1.5, -0.25, 0.0]]), (S, 1))
    ends = [(1.5, -0.25, (0.0, 1.0)), (2.0, 0.0, (1.0, 1.0))]
    return Scene(f"degenerate{S}", seg, ends, "degenerate", ref_len=4.0, acc=np.zeros(S, F))


def straight_large(S):
    """For the near table's size guard (16 bits of seed: from S = 65536 on no table is built): a straight segment
    of spacing 1/64 with S = 65535 / 65536 points and N = 8, P = 5; end points nearest to the last point, to index
    0 and to points in the last chunk, one of them between two (a tie inside one pair record)."""
    x = np.arange(S, dtype=np.float64) * STEP
    seg = np.stack([x, np.zeros(S), np.zeros(S)], 1)
    last = float(x[-1])
    ends = [(last + 0.25, 0.0, (0.0, 1.0)), (last, 0.125, (1.0, 1.0)), (last + 0.5, -0.5, (0.0, 1.0)),
            (-0.25, 0.0, (0.0, 1.0)), (0.0, 0.125, (1.0, 1.0)),
            (last - 5 * STEP, 0.0625, (0.0, 1.0)), (last - 300 * STEP, -0.125, (1.0, 1.0)),
            (last - 5 * STEP - STEP / 2, 0.0, (0.0, 1.0))]
    sc = Scene(f"straight{S}", seg, ends, "large")
    P = 5
    back = np.arange(P - 1, -1, -1, dtype=np.float64) * STEP
    px = np.stack([ex - back * ax for ex, _, (ax, _) in ends]).astype(F)
    py = np.stack([ey - back * ay for _, ey, (_, ay) in ends]).astype(F)
    sc._stacks = [(px, py)]
    return sc


def _build():
    base = [closed_square(), closed_square(4, "closed_small17"), closed_square(8, "closed_small33"),
            hairpin_bisector(), hairpin_even(), circle_centre(), stationary_run(200, 30, 40, "stationary_run40"),
            stationary_run(400, 120, 150, "stationary_run128"), lattice_zigzag()]
    for i, s in enumerate(base):
        s.rot = i
    out = list(base)
    for s in base:
        out.append(s.with_z(-0.0, "negzero"))
        out.append(s.with_z(0.5, "z05"))
    out.append(hairpin_bisector(lift=True))
    for s in base:
        for (dx, dy), tag in zip(OFFSETS, ("east", "west")):
            out.append(s.shifted(dx, dy, tag))
    return {s.name: s for s in out}


SCENES = _build()
DEGENERATE = {s.name: s for s in (degenerate(1), degenerate(2), degenerate(3))}
TIE_SCENES = sorted(n for n, s in SCENES.items() if s.kind == "tie")


# ---------------------------------------------------------------------------
# the roll-out scenes of the full cycles
# ---------------------------------------------------------------------------
def cycle_inputs(scene, state, P, ks=range(1, 13)):
    """A controller cycle over `scene` with no obstacles: vx = 0.125 k for k in ks (up to 1.5), vy = omega = 0,
    dt = 0.125 -- every roll-out point stays on the 1/64 grid of the robot's line."""
    import synthetic as syn

    s = SCENES[scene]
    vx = 0.125 * np.asarray(list(ks), dtype=np.float64)
    return dict(name=scene, vx=vx, vy=np.zeros_like(vx), omega=np.zeros_like(vx), P=P, dt=0.125, state=state,
                points=np.zeros((0, 3), F), octree_res=0.05, seg_xyz=s.seg, acc_at_seg=s.acc, ref_len=s.ref_len,
                weights=(0.7, 1.3, 0.0, 0.0, 0.0), max_range=10.0, robot=syn.ROBOT_CYLINDER,
                acc_limits=(syn.LIMITS["vx"][1], syn.LIMITS["vy"][1], syn.LIMITS["omega"][2]))


CYCLES = [("hairpin_bisector", (0.0, 0.25, 0.0, 0.0)), ("hairpin_bisector", (3.0, 0.25, 0.0, 0.0)),
          ("closed_square", (0.0, 0.0, 0.0, 0.0)),
          ("hairpin_even", (0.0, 0.25, 0.0, 0.0)), ("hairpin_even", (3.0, 0.25, 0.0, 0.0))]
CYCLE_PS = (31, 44, 64)
# One to four samples on hairpin_even from x = 0 with P = 31 (end points at x = 30 k / 64): a workgroup of the
# single-launch cycle costs so few survivors by teams of lanes (group_segment_search: eight lanes a point for one or
# two survivors, four for three or four).  k = 4, 12: tied indices 8 (mod 16); k = 2, 6, 10: 4 (mod 8).
TEAM_KS = ((4,), (4, 12), (2, 4, 6), (2, 6, 10, 12))


def bits(a):
    """uint32 views with every NaN made one pattern: a NaN equals a NaN whatever its payload or sign."""
    a = np.ascontiguousarray(a, F)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))
