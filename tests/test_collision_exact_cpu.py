"""The oracle's shape-against-voxel tests (ko.Collision.check_at: the planar round and box tests, the tilted
sphere / box / cylinder tests, the height gate and the key formation) against the exact geometry of
collision_exact_ref.py: contact itself, +-4 eps and +-64 eps about it, word boundaries and negative keys, where
a `<` for a `<=`, a missing separating axis or a floor on the wrong side of zero shows.  The band eps = 2^-20 L
(derivation: collision_exact_ref.py) stays near 1e-6 m: 0 in the dyadic family, 2.7e-7 .. 8.4e-7 m in the
identity frame, 1.3e-6 .. 2.8e-6 m behind the planar mount and 1.9e-6 .. 3.4e-6 m behind the tilted ones; every
message names the value used.  The fuzz family has no undecided pose at all (0 of 4800, cap 1 %)."""
import math

import numpy as np
import pytest

import collision_exact_ref as cx
from oracle import ko


def oracle_of(sc):
    c = ko.Collision(sc.shape, sc.dims, sc.spos, sc.srot, sc.res)
    c.update_state(*sc.state[:3])
    if sc.feed[0] == "scan":
        c.update_scan(sc.feed[1], sc.feed[2])
    else:
        c.update_points(sc.feed[1], sc.feed[2])
    return c


def check(b):
    c = oracle_of(b.scene)
    got = [c.check_at(b.x[i], b.y[i], b.yaw[i]) for i in range(len(b.x))]
    cx.assert_batch(b, got, "the oracle")
    return c


# -- the reference itself, against closed forms worked out by hand ------------------------------------------------
def test_reference_closed_forms():
    """(a)'s contacts are asserted where they are generated (3-4-5: 0.375^2 + 0.5^2 = 0.625^2; 2-3-6-7:
    0.25^2 + 0.375^2 + 0.75^2 = 0.875^2; 1-2-2-3; |q| = a + h; zlo = zc + h / 2): contact a HIT, 2^-20 m off a
    MISS, at eps = 0.  A rectangle at 45 degrees about the origin reaches a along its own axis, so it meets the
    square whose nearest corner is (p, p) exactly when p sqrt 2 <= a, while its bounding box
    ((a + b) / sqrt 2 = 0.32 > p) overlaps the square either way: p = 0.25, a = 0.36 meets, a = 0.35 does not."""
    assert len(cx.family_dyadic()) > 0
    for length, want in ((0.72, cx.HIT), (0.70, cx.MISS)):
        sc = cx.points_scene(cx.BOX, [length, 0.2, 0.5], 0.125, [(2, 2, 0)])
        assert (length / 2 + 0.1) / math.sqrt(2) > 0.25
        for yaw in (math.pi / 4, -3 * math.pi / 4):
            assert sc.classify(0.0, 0.0, yaw) == want
        assert sc.classify(0.0, 0.0, 3 * math.pi / 4) == cx.MISS       # (turned away: its width 0.1 is too short)
    # a disc against a corner at exactly its radius, by the same polygon routine the tilted cylinder uses
    sq = [(cx.Fr(3, 8), cx.Fr(1, 2)), (cx.Fr(1), cx.Fr(1, 2)), (cx.Fr(1), cx.Fr(1)), (cx.Fr(3, 8), cx.Fr(1))]
    assert cx._origin_poly_d2(cx._hull(sorted(sq))) == cx.Fr(25, 64)
    tri = [(cx.Fr(-1), cx.Fr(1)), (cx.Fr(1), cx.Fr(1)), (cx.Fr(0), cx.Fr(3))]
    assert cx._origin_poly_d2(cx._hull(sorted(tri))) == 1           # nearest point inside an edge
    assert cx._origin_poly_d2(cx._hull(sorted(tri + [(cx.Fr(0), cx.Fr(-1))]))) == 0    # the origin inside


def test_reference_pitched_by_90_degrees():
    """The configuration of test_tilted_mount.test_closed_form_cases_pin_the_tilted_tests: one scan point straight
    ahead, the mount pitched by 90 degrees about y, so the voxel lies below the robot at depth r and a shape that
    reaches down to -0.55 m meets it exactly when the voxel's nearest face floor(r / res) res lies above that."""
    res, srot = 0.1, cx.quat((0, 1, 0), math.pi / 2)
    for shape, dims in ((cx.CYLINDER, [0.3, 1.1]), (cx.SPHERE, [0.55]), (cx.BOX, [0.6, 0.6, 1.1])):
        for r, expect in ((0.45, cx.HIT), (0.55, cx.HIT), (0.62, cx.MISS), (0.9, cx.MISS)):
            sc = cx.Scene(shape, dims, res, ("scan", np.array([r]), np.array([0.0])), srot, (0, 0, 0), midvoxel=False)
            assert not sc.planar and len(sc.keys) == 1
            assert (math.floor(r / res) * res <= 0.55) == (expect == cx.HIT)
            b = cx.classify_batch(sc, [(cx.BODY[0], cx.BODY[1], 0.0)], "pitched")
            assert list(b.want) == [expect], (shape, r)
            check(b)


# -- the oracle over the families -----------------------------------------------------------------------------------
def test_dyadic_contact_without_a_band():
    for b in cx.family_dyadic():
        assert b.eps == 0.0
        check(b)


@pytest.mark.parametrize("shape", list(cx.SHAPES))
@pytest.mark.parametrize("frame", cx.FRAMES)
def test_near_contact(frame, shape):
    b = cx.family_near(frame, shape)
    assert cx.UNDECIDED not in b.want
    check(b)


@pytest.mark.parametrize("shape", list(cx.SHAPES))
def test_near_contact_points_behind_the_planar_mount(shape):
    check(cx.family_near_points(shape))


def test_edge_against_edge_of_the_tilted_box():
    seen = set()
    for b in cx.family_edge_edge():
        check(b)
        seen.update(b.only_axes)
    assert seen == set(range(9))


@pytest.mark.parametrize("along", (0, 1))
@pytest.mark.parametrize("shape", ("cylinder", "box"))
@pytest.mark.parametrize("frame", ("identity", "planar"))
def test_rows_of_voxels_across_key_zero(frame, shape, along):
    check(cx.family_masks(frame, shape, along))


def test_pose_counts():
    for b in cx.family_counts():
        check(b)


@pytest.mark.parametrize("shape", ("cylinder", "box", "sphere"))
@pytest.mark.parametrize("frame", ("identity", "planar"))
def test_window_about_a_distant_first_pose(frame, shape):
    check(cx.family_crop(frame, shape))


def test_height_gate():
    for b in cx.family_height():
        check(b)


def test_key_formation():
    """Not in test_extreme_inputs.py in this form: that file compares device cycles with the oracle's over points at
    the key window; here the kept keys are restated (floor of the double product) and located with a needle."""
    for b in cx.family_keys():
        c = check(b)
        assert c.num_voxels == b.columns, (b.name, c.num_voxels, b.columns)


@pytest.mark.parametrize("shape", list(cx.SHAPES))
@pytest.mark.parametrize("frame", cx.FRAMES)
def test_fuzz(frame, shape):
    b = cx.family_fuzz(frame, shape)
    cx.assert_fuzz_conditions(b)
    check(b)
