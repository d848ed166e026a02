"""Independent Python restatement of the reference LocalMapper (mapping/local_mapper.{h,cpp}) and of
bresenhamEnhanced (mapping/line_drawing.h:55-124), for the tests.  Not collected by pytest.

It shares nothing with the oracle (oracle/kompass_oracle.c) or the kernels (csrc/kc_mapper.hip): the line is
walked step by step from the start cell, every step, with the reference's three emit branches in their order --
no step range, no closed-form state.  Integers are exact (numpy int64 / Python int), which equals the
reference's `int` arithmetic wherever that does not overflow (its `error + ddy` reaches about 4 dx, so from
dx >= 2^29 on).  Floats follow the reference's promotions as DESIGN.md §5 reads them.  The rules this build adds
where the reference is undefined: a beam whose end cell offset x / res or y / res is not below
2^30 in magnitude (NaN and inf included) is skipped, and so is a sensor whose own offset is not below 2^30.

Emissions are (beam, i, j) arrays in the reference's order: beam by beam, and within a beam in the order
bresenhamEnhanced appends points.  Only the emissions inside the grid are kept (local_mapper.cpp:142, 176)."""
from __future__ import annotations

import math
import shutil
import subprocess
from pathlib import Path

import numpy as np

F = np.float32
UNEXPLORED, EMPTY, OCCUPIED = -1, 0, 100          # local_mapper.h:9
MAX_OFFSET = 2.0 ** 30                            # the skip rule


def central_point(H, W):
    """m_centralPoint, local_mapper.h:26-27: std::round of the INTEGER quotient, minus one."""
    return H // 2 - 1, W // 2 - 1


def _offset(v, res):
    """static_cast<int>(poseTargetInCentral(k) / m_resolution) of localToGrid (local_mapper.h:216-219): a float
    quotient truncated toward zero; None where this build's 2^30 rule applies."""
    with np.errstate(all="ignore"):
        q = F(v) / F(res)
    if not abs(float(q)) < MAX_OFFSET:
        return None
    return int(q)


def start_cell(H, W, res, pos):
    """m_startPoint = localToGrid(laserscanPosition.xy), local_mapper.h:30-31."""
    c0, c1 = central_point(H, W)
    o0, o1 = _offset(pos[0], res), _offset(pos[1], res)
    if o0 is None or o1 is None:
        raise ValueError("sensor offset not below 2^30 cells")
    return c0 + o0, c1 + o1


def end_cell(H, W, res, pos, orient, angle, rng):
    """updateGrid_ (local_mapper.cpp:129-134): float angle and range; `m_laserscanOrientation + angle` is a float
    sum handed to ::cos(double); range * cos is double, the position is added in double, x narrows to float; then
    localToGrid.  None for a skipped beam."""
    th = F(F(orient) + F(angle))
    if not math.isfinite(float(th)):
        return None
    c, s = math.cos(float(th)), math.sin(float(th))
    with np.errstate(all="ignore"):
        r = float(F(rng))
        x = F(float(F(pos[0])) + r * c)
        y = F(float(F(pos[1])) + r * s)
    c0, c1 = central_point(H, W)
    o0, o1 = _offset(x, res), _offset(y, res)
    if o0 is None or o1 is None:
        return None
    return c0 + o0, c1 + o1


def walk(s, ends, H=None, W=None, max_steps=1 << 20):
    """bresenhamEnhanced (line_drawing.h:55-124) from s to every end cell, all beams in lockstep.  Returns
    (beam, seq, x, y) int64 arrays of the emitted points (with H, W: only those inside the grid), where seq orders
    the points of one beam as the reference appends them.  Raises when a line is longer than max_steps (the native
    walker takes those)."""
    ends = np.asarray(ends, np.int64).reshape(-1, 2)
    nb = len(ends)
    out_b, out_q, out_x, out_y = [], [], [], []

    def emit(sel, q, x, y):
        if H is not None:
            keep = (x >= 0) & (x < H) & (y >= 0) & (y < W)
            sel, x, y = sel[keep], x[keep], y[keep]
        out_b.append(sel)
        out_q.append(np.broadcast_to(np.int64(q), sel.shape))
        out_x.append(x)
        out_y.append(y)

    x = np.full(nb, s[0], np.int64)
    y = np.full(nb, s[1], np.int64)
    dx = ends[:, 0] - s[0]
    dy = ends[:, 1] - s[1]
    emit(np.arange(nb), 0, x.copy(), y.copy())                # points.emplace_back(x, y) before the loop
    xstep = np.where(dx >= 0, 1, -1)
    ystep = np.where(dy >= 0, 1, -1)
    dx, dy = np.abs(dx), np.abs(dy)
    ddy, ddx = 2 * dy, 2 * dx
    first = ddx >= ddy                                        # first octant (0 <= slope <= 1)
    if nb and int(np.maximum(dx, dy).max()) > max_steps:
        raise ValueError("line too long for the Python walk")
    for octant in (True, False):
        idx = np.nonzero(first == octant)[0]
        if len(idx) == 0:
            continue
        # major / minor names only to write the two octants once; each branch below is the reference's
        X, Y = x[idx], y[idx]
        XS, YS = xstep[idx], ystep[idx]
        DDX, DDY = ddx[idx], ddy[idx]
        n = dx[idx] if octant else dy[idx]
        error = n.copy()
        errorprev = n.copy()
        for i in range(int(n.max()) if len(n) else 0):
            act = i < n
            q = 1 + 3 * i
            if octant:
                X = np.where(act, X + XS, X)
                error = np.where(act, error + DDY, error)
                inc = act & (error > DDX)
                Y = np.where(inc, Y + YS, Y)
                error = np.where(inc, error - DDX, error)
                tot = error + errorprev
                lt, gt, eq = inc & (tot < DDX), inc & (tot > DDX), inc & (tot == DDX)
                # if (<) (x, y - ystep); else if (>) (x - xstep, y); else both, (x - xstep, y) first
                one = lt | gt | eq
                emit(idx[one], q, np.where(lt, X, X - XS)[one], np.where(lt, Y - YS, Y)[one])
                emit(idx[eq], q + 1, X[eq], (Y - YS)[eq])
            else:
                Y = np.where(act, Y + YS, Y)
                error = np.where(act, error + DDX, error)
                inc = act & (error > DDY)
                X = np.where(inc, X + XS, X)
                error = np.where(inc, error - DDY, error)
                tot = error + errorprev
                lt, gt, eq = inc & (tot < DDY), inc & (tot > DDY), inc & (tot == DDY)
                # if (<) (x - xstep, y); else if (>) (x, y - ystep); else both, (x - xstep, y) first
                one = lt | gt | eq
                emit(idx[one], q, np.where(gt, X, X - XS)[one], np.where(gt, Y - YS, Y)[one])
                emit(idx[eq], q + 1, X[eq], (Y - YS)[eq])
            emit(idx[act], q + 2, X[act], Y[act])             # points.emplace_back(x, y)
            errorprev = np.where(act, error, errorprev)
    cat = lambda v: np.concatenate(v).astype(np.int64) if v else np.zeros(0, np.int64)
    return cat(out_b), cat(out_q), cat(out_x), cat(out_y)


def in_grid_emissions(H, W, walked):
    """The emissions inside the grid, beam by beam in the reference's order: (beam, i, j)."""
    b, q, i, j = walked
    keep = (i >= 0) & (i < H) & (j >= 0) & (j < W)
    b, q, i, j = b[keep], q[keep], i[keep], j[keep]
    order = np.lexsort((q, b))
    return b[order], i[order], j[order]


def beams(H, W, res, pos, orient, angles, ranges):
    """(start cell, beam indices that are not skipped, their end cells [k, 2])."""
    s = start_cell(H, W, res, pos)
    kept, ends = [], []
    for k, (a, r) in enumerate(zip(np.asarray(angles, np.float64), np.asarray(ranges, np.float64))):
        t = end_cell(H, W, res, pos, orient, float(a), float(r))
        if t is not None:
            kept.append(k)
            ends.append(t)
    return s, np.asarray(kept, np.int64), np.asarray(ends, np.int64).reshape(-1, 2)


def emissions(H, W, res, pos, orient, angles, ranges, walker=None):
    """Every in-grid emission of the scan, as (beam, i, j) in the reference's order, plus the end cells [n, 2]
    (a skipped beam's end cell is (INT64_MIN, INT64_MIN): it emits nothing).  walker(s, ends, H, W) -> the walk()
    tuple; native_walker() fits there for lines Python cannot walk."""
    s, kept, ends = beams(H, W, res, pos, orient, angles, ranges)
    b, i, j = in_grid_emissions(H, W, (walker or walk)(s, ends, H, W))
    all_ends = np.full((len(np.atleast_1d(ranges)), 2), np.iinfo(np.int64).min, np.int64)
    all_ends[kept] = ends
    return s, kept[b] if len(b) else b, i, j, all_ends


def _stamp(H, W, b, i, j, ends):
    """local_mapper.cpp:147-155 in emission order: the end cell of the beam gets OCCUPIED by assignment, any other
    cell max(cell, EMPTY)."""
    grid = np.full((H, W), UNEXPLORED, np.int32)
    at_end = (i == ends[b, 0]) & (j == ends[b, 1])
    # the assignments of OCCUPIED and the maxima with EMPTY commute (OCCUPIED is above EMPTY and a maximum never
    # lowers it), so the two sets of writes are applied as sets
    grid[i[~at_end], j[~at_end]] = np.maximum(grid[i[~at_end], j[~at_end]], EMPTY)
    grid[i[at_end], j[at_end]] = OCCUPIED
    return grid


def scan_to_grid(H, W, res, pos, orient, angles, ranges, walker=None):
    """LocalMapper::scanToGrid (local_mapper.cpp:204-220), single thread: fill UNEXPLORED, then every beam."""
    _, b, i, j, ends = emissions(H, W, res, pos, orient, angles, ranges, walker)
    return _stamp(H, W, b, i, j, ends)


def cell_probability(distance, current_range, previous_prob, res, p):
    """LocalMapper::updateGridCellProbability (local_mapper.cpp:106-125), elementwise.  Every name is float; the
    literal 1.0 makes pSensor / (1.0 - pSensor) a double, and with it the product and the sums around it; the
    result narrows to float on return.  The products associate left to right."""
    res, prior = F(res), F(p["p_prior"])
    distance = F(distance) * res
    current_range = F(current_range) - F(p["wall_size"])
    pF = np.where(distance < current_range, F(p["p_empty"]), F(p["p_occupied"])).astype(F)
    delta = np.where(distance < F(p["range_sure"]), F(0.0), F(1.0)).astype(F)
    p_sensor = pF + (delta * ((distance - F(p["range_sure"])) / F(p["range_max"])) * (prior - pF))
    prev_odds = previous_prob / (F(1) - previous_prob)
    sensor_odds = p_sensor.astype(np.float64) / (1.0 - p_sensor.astype(np.float64))
    prior_odds = (F(1) - prior) / prior
    p_curr = 1 - (1 / (1 + ((prev_odds.astype(np.float64) * sensor_odds) * np.float64(prior_odds))))
    return p_curr.astype(F)


def eigen_int_norm(di, dj):
    """(pt - m_startPoint).norm() on Vector2i (local_mapper.cpp:180): Eigen's norm is sqrt(squaredNorm()) in the
    scalar type, so the double square root of the integer squared norm is truncated back to an integer.  The
    squared norm is exact here (the reference's int overflows from 46 341 cells on: DESIGN.md §5)."""
    d2 = np.asarray(di, np.int64) ** 2 + np.asarray(dj, np.int64) ** 2
    return np.sqrt(d2.astype(np.float64)).astype(np.int64)


def scan_to_grid_baysian(H, W, res, pos, orient, angles, ranges, previous, params, walker=None):
    """LocalMapper::scanToGridBaysian (local_mapper.cpp:222-241), single thread, with updateGridBaysian_
    (:161-202): every in-grid point of every beam, in order, writes its probability -- the last write wins.
    previous: previousGridDataProb [H, W] float32.  -> (grid int32, prob float32)."""
    s, b, i, j, ends = emissions(H, W, res, pos, orient, angles, ranges, walker)
    grid = _stamp(H, W, b, i, j, ends)
    prob = np.full((H, W), F(params["p_prior"]), F)                      # gridDataProb.fill(m_pPrior)
    if len(b):
        rng = np.asarray(ranges, np.float64).astype(F)[b]
        dist = eigen_int_norm(i - s[0], j - s[1]).astype(F)
        val = cell_probability(dist, rng, np.asarray(previous, F)[i, j], res, params)
        # the writes in emission order: the last one to each cell stays
        flat = i * W + j
        rev = flat[::-1]
        _, last = np.unique(rev, return_index=True)
        keep = len(flat) - 1 - last
        prob[i[keep], j[keep]] = val[keep]
    return grid, prob


def warp_sources(H, W, inv):
    """srcX / srcY of every cell [H, W] (local_mapper.cpp:44-52): the lazy 3-term products reduce as a0 + (a1 + a2)
    (Eigen's unrolled redux) in float, and the results widen to double."""
    inv = np.asarray(inv, F)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    fx, fy = xx.astype(F), yy.astype(F)
    src_x = (inv[0, 0] * fx + (inv[0, 1] * fy + inv[0, 2] * F(1))).astype(np.float64)
    src_y = (inv[1, 0] * fx + (inv[1, 1] * fy + inv[1, 2] * F(1))).astype(np.float64)
    return src_x, src_y


def warp(previous, inv):
    """The per-cell part of getPreviousGridInCurrentPose (local_mapper.cpp:44-75): inv is the inverted Matrix3f.
    srcX / srcY are doubles of the float results (warp_sources); the blend is float."""
    previous = np.asarray(previous, F)
    H, W = previous.shape
    src_x, src_y = warp_sources(H, W, inv)
    ok = (src_x >= 0) & (src_x < W - 1) & (src_y >= 0) & (src_y < H - 1)
    x0 = np.floor(np.where(ok, src_x, 0)).astype(np.int64)
    y0 = np.floor(np.where(ok, src_y, 0)).astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    w0 = (np.where(ok, src_x, 0) - x0).astype(F)
    w1 = F(1) - w0
    h0 = (np.where(ok, src_y, 0) - y0).astype(F)
    h1 = F(1) - h0
    x1c, y1c = np.minimum(x1, W - 1), np.minimum(y1, H - 1)
    value = h1 * (w1 * previous[y0, x0] + w0 * previous[y0, x1c]) + h0 * (w1 * previous[y1c, x0] +
                                                                          w0 * previous[y1c, x1c])
    return ok, value.astype(F)


def warp_previous(previous, inv, p_prior):
    """getPreviousGridInCurrentPose: transformedGrid.fill(m_pPrior), then the cells whose source lies inside."""
    ok, value = warp(previous, inv)
    out = np.full(np.shape(previous), F(p_prior), F)
    out[ok] = value[ok]
    return out


# ---------------------------------------------------------------------------
# the same walk in C++ with int64 error terms (tests/native/bresenham_literal.cpp), for lines of up to ~2^30 steps
# ---------------------------------------------------------------------------
NATIVE_SRC = Path(__file__).resolve().parent / "native" / "bresenham_literal.cpp"


def have_gxx():
    return shutil.which("g++") is not None


def build_native(dst_dir):
    exe = Path(dst_dir) / "bresenham_literal"
    p = subprocess.run(["g++", "-std=c++17", "-O2", str(NATIVE_SRC), "-o", str(exe)], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return exe


def native_walker(exe):
    """walker(s, ends, H, W) for emissions(): the in-grid points the native program prints, in its order."""
    def run(s, ends, H, W):
        args = [str(exe), str(H), str(W), str(int(s[0])), str(int(s[1]))]
        args += [str(int(v)) for e in np.asarray(ends, np.int64).reshape(-1, 2) for v in e]
        r = subprocess.run(args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        rows = [ln.split() for ln in r.stdout.splitlines() if not ln.startswith("steps")]
        a = np.array(rows, np.int64).reshape(-1, 4)
        return a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    return run


# ---------------------------------------------------------------------------
# scenes shared by the CPU and GPU tests
# ---------------------------------------------------------------------------
def aim(H, W, res, pos, targets):
    """(angles, ranges) of beams from the sensor at pos (orientation 0) whose end cells are the target cells: each
    end point sits half a cell inside its cell (the offset is truncated toward zero), so float rounding cannot move
    it.  Returns the end cells the restatement computes too."""
    c = central_point(H, W)
    t = np.asarray(targets, np.float64).reshape(-1, 2)
    q = (t - c) + 0.5 * np.sign(t - c)
    v = q * float(F(res)) - np.array([float(F(pos[0])), float(F(pos[1]))])
    ang, rng = np.arctan2(v[:, 1], v[:, 0]), np.hypot(v[:, 0], v[:, 1])
    got = [end_cell(H, W, res, pos, 0.0, a, r) for a, r in zip(ang, rng)]
    return ang, rng, np.array(got, np.int64).reshape(-1, 2)


def sensor_pos(H, W, res, cell):
    """A sensor position whose start cell is `cell` (res a power of two: the quotient is exact)."""
    c = central_point(H, W)
    return ((cell[0] - c[0]) * res, (cell[1] - c[1]) * res, 0.0)


def border_and_outside_cells(H, W, dists=(1, 2, 3, 64, 10_000)):
    """Sensor cells: the four corners and the middle of each border, and outside each side and corner by d."""
    cells = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0),
             (H // 2, W - 1), (H // 2, W // 2)]
    for d in dists:
        cells += [(-d, W // 2), (H - 1 + d, W // 2), (H // 2, -d), (H // 2, W - 1 + d), (-d, -d),
                  (H - 1 + d, W - 1 + d)]
    return cells
