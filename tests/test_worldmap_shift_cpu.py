"""The rolling window without a device (DESIGN.md 4.11 rules 46 to 50): the library's host-only kc_worldmap_recentre_plan
and kc_worldmap_check_shift against the numpy statement tests/worldmap_shift_ref.py, the refusals of the entries that
need a context, and the statement against itself -- where origin and quantisation are exact, a shift commutes with an
update, which fixes rule 47's sign convention.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import kompass_cpp
import kompass_hip as kh
import worldmap_mcl_ref as mref
import worldmap_ref as ref
import worldmap_shift_ref as sref

KC_ERR_INVALID = -1  # include/kompass_hip.h
PLAN_SHAPES = [(70, 45), (45, 70), (64, 64), (7, 5), (1, 1), (2004, 1204), (33, 2)]


def plan_cells(S, margin):
    """Cells that bracket every branch of rule 49 along an axis of size S."""
    edge = {margin - 1, margin, margin + 1, S - 2 - margin, S - 1 - margin, S - margin}
    return sorted(edge | {-1000, -65, -1, 0, S // 2 - 1, S // 2, S // 2 + 1, S - 1, S, S + 64, 3 * S + 7, 1 << 20, -(1 << 20)})


@pytest.mark.parametrize("W,H", PLAN_SHAPES)
def test_recentre_plan_equals_the_statement(W, H):
    n = 0
    for margin in sorted({0, 1, 10, (min(W, H) - 1) // 2}):
        if not 2 * margin < min(W, H):
            continue
        for stride in (1, 3, 16, 64, max(W, H) + 1, 5000):
            for ic in plan_cells(W, margin):
                for jc in plan_cells(H, margin)[::3] + [H - 1 - margin, margin]:
                    want = sref.recentre_plan(W, H, ic, jc, margin, stride)
                    assert kh.worldmap_recentre_plan(W, H, ic, jc, margin, stride) == want, (ic, jc, margin, stride)
                    n += 1
    assert n >= 200                                   # (a 1 x 1 map folds most of the bracket cells together)
    assert kompass_cpp.mapping.WorldMap.recentre_plan(W, H, W + 3, -2, 0, 1) == sref.recentre_plan(W, H, W + 3, -2, 0, 1)


def test_recentre_plan_by_hand():
    # 70 cells, margin 10: cells 10 .. 59 stay; 60 is 25 right of the centre cell 35: one stride of 16, two of 8, 25 of 1
    assert kh.worldmap_recentre_plan(70, 45, 10, 22, 10, 16) == (0, 0)
    assert kh.worldmap_recentre_plan(70, 45, 59, 34, 10, 16) == (0, 0)
    assert kh.worldmap_recentre_plan(70, 45, 60, 35, 10, 16) == (16, 0)        # 35 - 22 = 13: below one stride
    assert kh.worldmap_recentre_plan(70, 45, 60, 35, 10, 8) == (24, 8)
    assert kh.worldmap_recentre_plan(70, 45, 60, 35, 10, 1) == (25, 13)
    assert kh.worldmap_recentre_plan(70, 45, 9, 9, 10, 16) == (-16, 0)         # truncation towards zero: -26 / 16 = -1
    assert kh.worldmap_recentre_plan(70, 45, -13, 9, 10, 16) == (-48, 0)
    assert kh.worldmap_recentre_plan(70, 45, 9, 9, 10, 100) == (0, 0)          # a stride above the size: no move yet
    assert kh.worldmap_recentre_plan(71, 45, 200, 9, 10, 100) == (100, 0)      # odd size: the centre cell is 35


@pytest.mark.parametrize("args", [(70, 45, 0, 0, -1, 1), (70, 45, 0, 0, 0, 0), (70, 45, 0, 0, 0, -3), (70, 45, 0, 0, 23, 1),
                                  (70, 45, 0, 0, 40, 1), (1, 1, 0, 0, 1, 1), (0, 45, 0, 0, 0, 1), (70, -2, 0, 0, 0, 1)])
def test_recentre_plan_refusals(args):
    with pytest.raises(ValueError):
        sref.recentre_plan(*args)
    with pytest.raises(ValueError):
        kh.worldmap_recentre_plan(*args)
    with pytest.raises(ValueError):
        kompass_cpp.mapping.WorldMap.recentre_plan(*args)
    assert kh.worldmap_recentre_plan(70, 45, 0, 0, 22, 1) == sref.recentre_plan(70, 45, 0, 0, 22, 1)   # 2 * 22 < 45 just holds


def test_offset_cap():
    cap = sref.MAX_SHIFT
    for off, d, ok in [((0, 0), (cap, -cap), True), ((0, 0), (cap + 1, 0), False), ((cap, 0), (1, 0), False),
                       ((cap, -cap), (-5, 5), True), ((0, -cap), (0, -1), False), ((-cap, 0), (2 ** 31 - 1, 0), True),
                       ((-cap + 1, 0), (2 ** 31 - 1, 0), True), ((-cap + 2, 0), (2 ** 31 - 1, 0), False), ((5, 5), (-2 ** 31, 0), False), ((7, -9), (0, 0), True)]:
        if ok:
            sref.check_offset(*off, *d)
            kh.worldmap_check_shift(off, *d)
        else:
            with pytest.raises(IndexError):
                sref.check_offset(*off, *d)
            with pytest.raises(IndexError):
                kh.worldmap_check_shift(off, *d)


def test_null_context_is_refused_before_anything_else():
    L = kh.lib()
    a, b = C.c_int32(7), C.c_int32(7)
    assert L.kc_worldmap_shift(None, 1, 0) == KC_ERR_INVALID
    assert L.kc_worldmap_shift(None, 0, 0) == KC_ERR_INVALID
    assert L.kc_worldmap_offset(None, C.byref(a), C.byref(b)) == KC_ERR_INVALID
    assert L.kc_worldmap_recentre(None, 0.0, 0.0, 1, 1, C.byref(a), C.byref(b)) == KC_ERR_INVALID
    assert L.kc_worldmap_recentre_plan(70, 45, 0, 0, 1, 1, None, C.byref(b)) == KC_ERR_INVALID
    assert L.kc_worldmap_recentre_plan(70, 45, 60, 0, -1, 1, C.byref(a), C.byref(b)) == KC_ERR_INVALID
    assert (a.value, b.value) == (0, 0)                                          # a refusal reports no shift


# ---- the statement against itself ----
def mixed_state(w, seed=3, n=3):
    """`n` updates from seeded local grids: evidence strictly between e_min and e_max among the cells."""
    rng = np.random.default_rng(seed)
    for k in range(n):
        g = rng.choice(np.int32([-1, 0, 100, 50]), size=(31, 27), p=[0.2, 0.45, 0.3, 0.05]).astype(np.int32)
        ox, oy = w.origin
        r = w.resolution
        w.update(g, (ox + (20 + 12 * k) * r, oy + (18 + 4 * k) * r, 0.4 * k))
    e = w.evidence
    m = w.map.model if hasattr(w, "map") else w.model
    assert ((e > m["e_min"]) & (e < m["e_max"]) & (e != ref.NEVER)).sum() > 50
    return w


SHIFTS = [(1, 0), (-1, 0), (0, 1), (0, -1), (3, -2), (63, 7), (64, 0), (69, 0), (70, 0), (-75, 46), (0, 0)]


@pytest.mark.parametrize("d", SHIFTS)
def test_slices_equal_the_cell_loop(d):
    w = mixed_state(sref.RollingWorldMapRef(70, 45, 0.05, (-0.33, 1.7)))
    e, c = sref.shift_planes(w.evidence, w.cls, *d)
    np.testing.assert_array_equal(e, sref.shift_plane(w.evidence, *d, ref.NEVER))
    np.testing.assert_array_equal(c, sref.shift_plane(w.cls, *d, ref.UNEXPLORED))
    if abs(d[0]) >= 70 or abs(d[1]) >= 45:
        assert (e == ref.NEVER).all() and (c == ref.UNEXPLORED).all()            # a clear
    if d == (3, -2):
        assert e[0, 44] == w.evidence[3, 42] and c[66, 2] == w.cls[69, 0] and e[67, 10] == ref.NEVER and c[5, 1] == ref.UNEXPLORED


@pytest.mark.parametrize("d", [d for d in SHIFTS if d != (0, 0)] + [(-16, 16)])
def test_update_commutes_with_shift_where_arithmetic_is_exact(d):
    """res = 2^-4, origins and poses on multiples of 2^-10: origin_after and quantise_pose are exact, so the cell a world
    point falls into moves by exactly (di, dj).  Update then shift must equal shift then update on every cell of the new
    window whose source lay in the old one.  A flipped sign in rule 47 moves the map the wrong way and fails here."""
    res, origin = 0.0625, (-3.0 + 5 / 1024, 7.0 - 123 / 1024)
    rng = np.random.default_rng(11)
    g = rng.choice(np.int32([-1, 0, 100]), size=(41, 33), p=[0.2, 0.5, 0.3]).astype(np.int32)
    pose = (origin[0] + 30 * res + 37 / 1024, origin[1] + 20 * res - 411 / 1024, 0.7)
    a = mixed_state(sref.RollingWorldMapRef(70, 45, res, origin))
    b = mixed_state(sref.RollingWorldMapRef(70, 45, res, origin))
    np.testing.assert_array_equal(a.evidence, b.evidence)
    a.update(g, pose)
    a.shift(*d)
    b.shift(*d)
    b.update(g, pose)
    assert a.origin == b.origin == (origin[0] + d[0] * res, origin[1] + d[1] * res)     # exact
    I, J = np.meshgrid(np.arange(70), np.arange(45), indexing="ij")
    had_source = (I + d[0] >= 0) & (I + d[0] < 70) & (J + d[1] >= 0) & (J + d[1] < 45)
    np.testing.assert_array_equal(a.evidence[had_source], b.evidence[had_source])
    np.testing.assert_array_equal(a.cls[had_source], b.cls[had_source])
    assert (a.evidence[~had_source] == ref.NEVER).all()
    if had_source.any() and abs(d[0]) < 20 and abs(d[1]) < 15:
        assert (a.evidence[had_source] != ref.NEVER).sum() > 100                  # the check is not vacuous


def test_origin_is_never_accumulated():
    """res = 0.05 is no binary fraction; the origin is the one product and the one sum of rule 46 at every offset, with
    the float32 resolution widened, and comes back to the very origin given when the offset comes back to 0."""
    ox0, r = -0.33, 0.05
    w = sref.RollingWorldMapRef(70, 45, r, (ox0, 1.7))
    for k in range(1, 400):
        w.shift(3, -1)
        assert w.origin == (sref.origin_after(ox0, r, 3 * k), sref.origin_after(1.7, r, -k))
        assert w.origin[0] == ox0 + float(3 * k) * float(np.float32(r)) != ox0 + float(3 * k) * r
    assert w.offset == (1197, -399)
    w.shift(-1197, 399)
    assert w.origin == (ox0, 1.7) and w.offset == (0, 0)
    with pytest.raises(IndexError):
        w.shift(sref.MAX_SHIFT + 1, 0)
    assert w.offset == (0, 0)


def test_shift_particles_clamps():
    cap = mref.MAX_OFFSET
    tx, ty = sref.shift_particles([0, 5, cap, -cap, cap - 65536], [1, -cap + 3, 0, cap, -cap], 4, -2)
    assert tx == [-4 << 16, 5 - (4 << 16), cap - (4 << 16), -cap, cap - 5 * 65536]
    assert ty == [1 + (2 << 16), -cap + 3 + (2 << 16), 2 << 16, cap, -cap + (2 << 16)]
    assert sref.shift_particles([7], [9], 0, 0) == ([7], [9])


def test_follow_rolls_the_statement_off_its_first_rectangle():
    w = sref.RollingWorldMapRef(70, 45, 0.05, (0.0, 0.0))
    g = np.zeros((9, 9), np.int32)
    moves = []
    for k in range(60):
        x = 0.5 + 0.15 * k
        before = w.offset
        w.update(g, (x, 1.0, 0.0), follow=(10, 16))
        moves.append((w.offset[0] - before[0], w.offset[1] - before[1]))
        ic, jc = sref.robot_cell(0.05, w.origin, x, 1.0)
        assert 10 <= ic <= 59 and 10 <= jc <= 34 and w.cls[ic, jc] == ref.EMPTY
    assert w.offset[0] >= 70 and w.offset[1] == 0 and set(moves) == {(0, 0), (16, 0)}
