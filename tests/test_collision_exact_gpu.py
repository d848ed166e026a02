"""DwaContext.check_poses (pose_check_kernel: hit_round / hit_box over the host-built window; the tilted kernel:
tilt_cube_hit) against the exact geometry of collision_exact_ref.py, over the very cases
test_collision_exact_cpu.py puts to the oracle.  The planar tests are reached through set_points and set_scan, the
tilted ones through set_scan behind the tilted mounts; the height gate also through both sensor builds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import collision_exact_ref as cx  # noqa: E402
import kompass_hip as kh  # noqa: E402


def check(b, **options):
    sc = b.scene
    ctx = kh.DwaContext(sc.shape, sc.dims, sc.spos, sc.srot, sc.res, 0.1, max_samples=16, max_points=8)
    try:
        for name, value in options.items():
            ctx.set_option(name, value)
        if sc.feed[0] == "scan":
            ctx.set_scan(sc.state, sc.feed[1], sc.feed[2], 10.0)
        else:
            ctx.set_points(sc.state, np.ascontiguousarray(sc.feed[1], np.float32), 10.0, global_frame=sc.feed[2])
        got = ctx.check_poses(b.x, b.y, b.yaw)
    finally:
        ctx.close()
    cx.assert_batch(b, got, f"the device {options or ''}")


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
    """The planar kernel through set_points in the sensor's frame (set_scan reaches that frame in test_near_contact)."""
    check(cx.family_near_points(shape))


def test_edge_against_edge_of_the_tilted_box():
    for b in cx.family_edge_edge():
        check(b)


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


@pytest.mark.parametrize("on_host", (0, 1))
def test_height_gate_through_the_sensor_builds(on_host):
    for b in cx.family_height():
        check(b, sensor_on_host=on_host)


@pytest.mark.parametrize("on_host", (0, 1))
def test_key_formation(on_host):
    for b in cx.family_keys():
        check(b, sensor_on_host=on_host)


@pytest.mark.parametrize("shape", list(cx.SHAPES))
@pytest.mark.parametrize("frame", cx.FRAMES)
def test_fuzz(frame, shape):
    b = cx.family_fuzz(frame, shape)
    cx.assert_fuzz_conditions(b)
    check(b)
