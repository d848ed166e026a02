"""The world map's CPU statement (tests/worldmap_ref.py) on cases worked out by hand, the pose
quantisation of the library against it, and the refusals that need no device.  No GPU needed."""
import math

import numpy as np
import pytest

import kompass_hip as kh
import worldmap_ref as ref

YAWS = [0.0, math.pi / 2, -math.pi / 2, math.pi, 0.3, -2.5]


def local_grid(gh=9, gw=7, seed=0):
    rng = np.random.default_rng(seed)
    return rng.choice(np.int32([-1, 0, 100, 50]), size=(gh, gw)).astype(np.int32)


def latest(w, h, res=0.1, origin=(0.0, 0.0)):
    return ref.WorldMapRef(w, h, res, origin, **ref.LATEST_WINS)


def paste(world_shape, local, corner):
    """The class plane a plain paste of `local`, its cell (0, 0) at world cell `corner`, leaves on an empty map."""
    cls = np.full(world_shape, -1, np.int8)
    for i in range(local.shape[0]):
        for j in range(local.shape[1]):
            I, J = corner[0] + i, corner[1] + j
            if 0 <= I < world_shape[0] and 0 <= J < world_shape[1] and local[i, j] in (0, 100):
                cls[I, J] = local[i, j]
    return cls


def test_yaw_zero_whole_cell_offset_is_a_plain_paste():
    g = local_grid()
    c0, c1 = ref.central(*g.shape)
    assert (c0, c1) == (3, 2)
    for cell in [(12, 10), (2, 1), (35, 27), (0, 0)]:   # the robot's world cell: inside, and clipped at every side
        m = latest(37, 29, 0.1, origin=(-1.0, 2.0))
        x, y = -1.0 + cell[0] * m.resolution, 2.0 + cell[1] * m.resolution
        q = ref.quantise_pose(m.resolution, m.origin, x, y, 0.0)
        assert q == (65536, 0, cell[0] << 16, cell[1] << 16)
        n, box = m.update(g, q)
        want = paste((37, 29), g, (cell[0] - c0, cell[1] - c1))
        np.testing.assert_array_equal(m.cls, want)
        assert n == int((want != -1).sum())
        ii, jj = np.nonzero(want != -1)
        assert box == (ii.min(), jj.min(), ii.max(), jj.max())


def test_quarter_turn_is_the_paste_of_the_rotated_array():
    q = ref.quantise_pose(0.1, (0.0, 0.0), 1.5, 1.2, math.pi / 2)
    assert q[:2] == (0, 65536)   # cos(pi / 2) * 65536 = 4.0e-12 rounds to 0, sin to 65536 exactly
    assert q[2:] == (15 << 16, 12 << 16)
    g = local_grid()
    c0, c1 = ref.central(*g.shape)
    m = latest(37, 29)
    m.update(g, q)
    # local (i, j) -> offset (a, b) = (i - c0, j - c1) -> world offset (-b, a): cell (15 - (j - c1), 12 + (i - c0))
    want = np.full((37, 29), -1, np.int8)
    for i in range(g.shape[0]):
        for j in range(g.shape[1]):
            if g[i, j] in (0, 100):
                want[15 - (j - c1), 12 + (i - c0)] = g[i, j]
    np.testing.assert_array_equal(m.cls, want)
    # the same through numpy: rot90 of the local array, pasted whole
    r = np.flip(g.T, axis=0)   # the array turned by a quarter: r[u, v] = g[v, gw - 1 - u]
    corner = (15 - (g.shape[1] - 1 - c1), 12 - c0)
    np.testing.assert_array_equal(m.cls, paste((37, 29), r, corner))


def test_a_pose_wholly_outside_changes_nothing():
    g = local_grid()
    for pose in [(-3.0, 1.0, 0.3), (1.0, 40.0, -2.5), (90.0, 90.0, 0.0)]:
        m = ref.WorldMapRef(37, 29, 0.1)
        assert m.update(g, pose) == (0, (-1, -1, -1, -1))
        assert (m.cls == -1).all() and (m.evidence == ref.NEVER).all()


def test_half_cell_offsets_round_up():
    # tx = 2.5 cells: world cell I sees a = floor(I - 2.5 + 0.5) = I - 2, so local row c0 lands on world cell 2
    g = np.full((3, 3), -1, np.int32)
    g[0, 0] = 100                      # central cell of a 3 x 3 grid is (0, 0)
    m = latest(8, 8, 1.0)
    m.update(g, (65536, 0, (2 << 16) + (1 << 15), (5 << 16) - (1 << 15)))
    assert np.argwhere(m.cls == 100).tolist() == [[2, 4]]   # ty = 4.5: b = floor(J - 4.5 + 0.5) = J - 4


def test_the_model_saturates_and_the_class_flips_at_occ_thr():
    occ = np.full((3, 3), 100, np.int32)
    free = np.zeros((3, 3), np.int32)
    m = ref.WorldMapRef(1, 1, 1.0)      # defaults: hit 3, miss 1, -8 .. 14, occ_thr 1
    pose = (65536, 0, 0, 0)
    seen = []
    for _ in range(6):
        m.update(occ, pose)
        seen.append(int(m.evidence[0, 0]))
    assert seen == [3, 6, 9, 12, 14, 14] and m.cls[0, 0] == 100
    for k in range(13):
        n, _ = m.update(free, pose)
        assert m.evidence[0, 0] == 13 - k and m.cls[0, 0] == 100 and n == 0
    n, box = m.update(free, pose)       # 1 -> 0: below occ_thr
    assert m.evidence[0, 0] == 0 and m.cls[0, 0] == 0 and (n, box) == (1, (0, 0, 0, 0))
    for _ in range(12):
        m.update(free, pose)
    assert m.evidence[0, 0] == -8
    assert m.update(occ, pose)[0] == 0 and m.evidence[0, 0] == -5 and m.cls[0, 0] == 0
    m.update(occ, pose)
    assert m.evidence[0, 0] == -2 and m.cls[0, 0] == 0
    assert m.update(occ, pose)[0] == 1 and m.evidence[0, 0] == 1 and m.cls[0, 0] == 100   # -2 + 3 = occ_thr
    # a first observation counts from 0, and other values leave the cell alone
    m.clear()
    assert m.update(np.full((3, 3), 50, np.int32), pose)[0] == 0 and m.evidence[0, 0] == ref.NEVER
    assert m.update(free, pose)[0] == 1 and m.evidence[0, 0] == -1 and m.cls[0, 0] == 0
    # occ_thr in the middle of the range
    m = ref.WorldMapRef(1, 1, 1.0, hit=2, miss=2, e_min=-4, e_max=6, occ_thr=4)
    m.update(occ, pose)
    assert (m.evidence[0, 0], m.cls[0, 0]) == (2, 0)
    m.update(occ, pose)
    assert (m.evidence[0, 0], m.cls[0, 0]) == (4, 100)
    m.update(free, pose)
    assert (m.evidence[0, 0], m.cls[0, 0]) == (2, 0)


def test_prior_maps_to_the_ends_of_the_range():
    m = ref.WorldMapRef(4, 3, 0.5)
    g = np.int32([[100, 0, -1], [50, 100, 0], [0, 0, 0], [-1, -1, 7]])
    m.set_prior(g)
    np.testing.assert_array_equal(m.evidence, np.int8([[14, -8, -128], [-128, 14, -8], [-8, -8, -8], [-128, -128, -128]]))
    np.testing.assert_array_equal(m.cls, np.int8([[100, 0, -1], [-1, 100, 0], [0, 0, 0], [-1, -1, -1]]))


@pytest.mark.parametrize("yaw", YAWS)
def test_quantise_pose_of_the_library_is_the_reference(yaw):
    for res, origin, x, y in [(0.05, (0.0, 0.0), 1.0, 2.0), (0.1, (-3.25, 7.5), 0.37, -1.234567), (0.25, (100.0, -50.0), 99.9, 3.3),
                              (0.03, (0.013, -0.007), 12.3456789, 9.87654321), (1.0, (0.0, 0.0), 0.5, 1.5)]:
        p = kh.worldmap_quantise_pose(res, origin, x, y, yaw)
        assert (p.cq, p.sq, p.tx, p.ty) == ref.quantise_pose(res, origin, x, y, yaw), (res, origin, x, y, yaw)
    import kompass_cpp

    assert kompass_cpp.mapping.WorldMap.quantise_pose(0.05, 0.0, 0.0, 1.0, 2.0, yaw) == ref.quantise_pose(0.05, (0, 0), 1.0, 2.0, yaw)


def test_quantise_pose_refuses_what_it_cannot_hold():
    far = (1 << 20) * 0.1
    p = kh.worldmap_quantise_pose(0.1, (0.0, 0.0), far * 0.999, 0.0, 0.0)
    assert p.tx == ref.quantise_pose(0.1, (0.0, 0.0), far * 0.999, 0.0, 0.0)[2]
    with pytest.raises(IndexError):
        kh.worldmap_quantise_pose(0.1, (0.0, 0.0), far * 1.001, 0.0, 0.0)
    with pytest.raises(IndexError):
        kh.worldmap_quantise_pose(0.1, (0.0, 0.0), 0.0, -far * 1.001, 0.0)
    with pytest.raises(ValueError):
        kh.worldmap_quantise_pose(0.1, (0.0, 0.0), 0.0, 0.0, float("nan"))
    with pytest.raises(ValueError):
        kh.worldmap_quantise_pose(0.0, (0.0, 0.0), 0.0, 0.0, 0.0)


def test_bad_arguments_raise_before_a_device_is_needed():
    with pytest.raises(ValueError):
        kh.WorldMapContext(0, 5, 0.1)
    with pytest.raises(ValueError):
        kh.WorldMapContext(5, 5, 0.0)
    with pytest.raises(IndexError):
        kh.WorldMapContext(32769, 1, 0.1)
    with pytest.raises(IndexError):
        kh.WorldMapContext(32768, 32768, 0.1)
    kh.worldmap_check_model()                       # the defaults, and "the latest wins"
    kh.worldmap_check_model(**ref.LATEST_WINS)
    for bad in [dict(occ_thr=-8), dict(occ_thr=-9), dict(occ_thr=15), dict(hit=0), dict(miss=0), dict(hit=128),
                dict(e_min=-128), dict(e_min=1, occ_thr=2), dict(e_max=128), dict(e_max=-1, e_min=-8, occ_thr=-1)]:
        with pytest.raises(ValueError):
            kh.worldmap_check_model(**bad)
    L = kh.lib()
    assert L.kc_worldmap_set_model(None, 0, 1, -8, 14, 1) == -1 and b"hit" in L.kc_last_error()
    kh.worldmap_check_grid(0.05, 9, 7, (3, 2), 0.05)
    with pytest.raises(ValueError, match="resolution"):
        kh.worldmap_check_grid(0.05, 9, 7, (3, 2), float(np.nextafter(np.float32(0.05), np.float32(1.0))))
    with pytest.raises(ValueError):
        kh.worldmap_check_grid(0.05, 0, 7, (3, 2), 0.05)
    import kompass_cpp

    with pytest.raises(ValueError):
        kompass_cpp.mapping.WorldMap(0, 5, 0.1)
    from kompass_core.mapping import WorldMap

    with pytest.raises(ValueError):
        WorldMap(5, -1, 0.1)


def test_world_map_is_present_in_every_layer():
    import kompass_cpp

    L = kh.lib()
    for name in ("kc_worldmap_create", "kc_worldmap_destroy", "kc_worldmap_set_model", "kc_worldmap_quantise_pose",
                 "kc_worldmap_update_device", "kc_worldmap_update_host", "kc_worldmap_update_from_mapper",
                 "kc_worldmap_set_prior_host", "kc_worldmap_set_prior_device", "kc_worldmap_clear", "kc_worldmap_grid_device",
                 "kc_worldmap_get"):
        assert hasattr(L, name) and name in kh.SIGNATURES, name
    cls = kompass_cpp.mapping.WorldMap
    for name in ("set_model", "set_prior", "update", "clear", "get_cls", "get_evidence", "get_changed", "get_changed_box",
                 "device_grid"):
        assert hasattr(cls, name), name
    from kompass_core.mapping import WorldMap
    from kompass_core.planning import GridPlanner  # noqa: F401

    for name in ("update", "set_prior", "occupancy", "evidence", "device_grid", "map_meta_data"):
        assert hasattr(WorldMap, name), name
    assert issubclass(kh.WorldMapContext, kh._Owner) and kh.WorldMapContext._kc == "kc_worldmap"
    if kh.device_count() == 0:  # no device: an error, never a CPU fallback
        with pytest.raises(kh.KompassHipError):
            kh.WorldMapContext(8, 8, 0.1)
        with pytest.raises(RuntimeError):
            cls(8, 8, 0.1)
