"""The world map's distance plane on the device (kc_worldmap_*distance*; DESIGN.md 4.11 rules 42 and 43) against the
brute-force statement tests/worldmap_dist_ref.py, bit for bit: the tiled kernel up to reach 63 and the two global passes
above it, full and partial refreshes, and the front ends.

The worlds are 130 x 67 and 70 x 45: more than one 64-cell tile each way (the second along I only), widths that are no
multiple of 4 or 64."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import worldmap_dist_ref as dref  # noqa: E402
import worldmap_ref as ref  # noqa: E402

RES, ORIGIN = 0.05, (-0.4, 0.9)
OCC, UNK, EMP = ref.OCCUPIED, ref.UNEXPLORED, ref.EMPTY
WORLDS = [(130, 67), (70, 45)]
REACHES = [1, 5, 16, 63, 254]                                   # 63: the last tiled reach; 254: the largest, on the fallback path


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


def world(w, h, kind):
    """corners: the four corner cells alone; seams: cells on both sides of every tile seam and a few unknown ones;
    seeded: all three classes everywhere; nowhere: no occupied cell."""
    c = np.full((w, h), EMP, np.int8)
    if kind == "corners":
        c[0, 0] = c[-1, 0] = c[0, -1] = c[-1, -1] = OCC
    elif kind == "seams":
        for i in (63, 64, 127, 128):
            if i < w:
                c[i, 5] = c[i, h - 3] = OCC
        c[10, 63 if h > 64 else h // 2] = c[11, 64 if h > 64 else h // 2 + 1] = OCC
        c[30:34, 20:22] = UNK
    elif kind == "seeded":
        rng = np.random.default_rng(w * 1000 + h)
        c = rng.choice(np.int8([OCC, UNK, EMP]), size=(w, h), p=[0.01, 0.03, 0.96]).astype(np.int8)
    elif kind == "nowhere":
        c[40:50, 10:20] = UNK
    return c


_WANT = {}


def want(shape, kind, reach, flags):
    """The statement's plane, computed once a case and left unchanged."""
    key = (shape, kind, reach, flags)
    if key not in _WANT:
        _WANT[key] = dref.dist2_plane(world(*shape, kind), reach, flags)
        _WANT[key].setflags(write=False)
    return _WANT[key]


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("reach", REACHES)
@pytest.mark.parametrize("shape", WORLDS)
def test_plane_equals_the_statement(shape, reach, flags):
    with kh.WorldMapContext(*shape, RES, ORIGIN) as m:
        m.set_distance(reach, flags=flags)
        for kind in ("corners", "seams", "seeded", "nowhere"):
            m.set_prior(world(*shape, kind))
            got = m.distance()
            w = want(shape, kind, reach, flags)
            assert got.dtype == np.uint16 and np.array_equal(got, w), (kind, np.argwhere(got != w)[:5].tolist())
            assert m.distance_info() == (reach, flags, (0, 0, shape[0] - 1, shape[1] - 1), True)
        assert (want(shape, "nowhere", reach, 0) == dref.FAR).all()


def test_off_by_default_and_refusals():
    with kh.WorldMapContext(70, 45, RES, ORIGIN) as m:
        assert m.distance_info() == (0, 0, (-1, -1, -1, -1), False)
        for call in (m.distance, m.distance_refresh, m.distance_device_ptr):
            with pytest.raises(kh.KompassHipError, match=r"\[kc -5\]"):
                call()
        for reach, flags, exc in ((-1, 0, IndexError), (255, 0, IndexError), (255, 2, IndexError), (3, 2, ValueError), (0, 1, ValueError)):
            with pytest.raises(exc):
                m.set_distance(reach, flags=flags)
        assert m.distance_info()[0] == 0
        m.set_distance(3)
        assert m.distance_info() == (3, 0, (-1, -1, -1, -1), False)         # lazily: nothing has run yet
        m.distance_refresh()
        assert m.distance_info() == (3, 0, (0, 0, 69, 44), True)
        m.distance_refresh()
        assert m.distance_info() == (3, 0, (-1, -1, -1, -1), False)         # the dirty box was empty: no launch
        assert m.distance_device_ptr() != 0
        m.set_distance(0)
        assert m.distance_info()[0] == 0
        with pytest.raises(kh.KompassHipError, match=r"\[kc -5\]"):
            m.distance()


def local_grid(rng, gh, gw, p_seen=0.7):
    return rng.choice(np.int32([100, 0, -1]), size=(gh, gw), p=[0.3 * p_seen, 0.7 * p_seen, 1.0 - p_seen]).astype(np.int32)


@pytest.mark.parametrize("reach,flags", [(5, 0), (16, 1), (70, 0)])     # tiled, tiled with the flag, the fallback
def test_refresh_follows_prior_clear_and_updates(reach, flags):
    """After set_prior, after clear and after each update of a sequence the plane equals the statement's (kept by rule
    43's bookkeeping) and a second context's full recompute, and distance_info reports the statement's box."""
    W, H = 130, 67
    rng = np.random.default_rng(7)
    wref = ref.WorldMapRef(W, H, RES, ORIGIN)
    with kh.WorldMapContext(W, H, RES, ORIGIN) as m, kh.WorldMapContext(W, H, RES, ORIGIN) as other:
        m.set_distance(reach, flags=flags)
        other.set_distance(reach, flags=flags)
        stmt = dref.DistRef(wref.cls, reach, flags)

        def agree(what, partial=None):
            stmt.cls = wref.cls
            box = stmt.refresh()
            got = m.distance()
            info = m.distance_info()
            assert info == (reach, flags, stmt.last_box, stmt.last_full), (what, info, stmt.last_box)
            assert np.array_equal(got, stmt.plane), (what, np.argwhere(got != stmt.plane)[:5].tolist())
            assert np.array_equal(stmt.plane, dref.dist2_plane(wref.cls, reach, flags)), what
            other.set_prior(m.planes()[0])
            assert np.array_equal(other.distance(), got) and other.distance_info()[3], what
            if partial is not None:
                assert (box is not None and not stmt.last_full) == partial, (what, box)

        agree("enabled")
        prior = world(W, H, "seeded")
        m.set_prior(prior)
        wref.set_prior(prior)
        stmt.mark_all()
        agree("prior", partial=False)
        m.clear()
        wref.clear()
        stmt.mark_all()
        agree("clear", partial=False)
        wide = reach >= 32                                       # a box grown by such a reach covers this map's height anyway
        # (centre in cells, yaw, local shape): across the seam at I = 64, on the border, across the seam at J = 64, small
        updates = [((64.0, 20.0), 0.3, (11, 9)), ((2.0, 3.0), -1.0, (9, 9)), ((100.0, 64.0), 2.0, (7, 13)), ((30.0, 40.0), 0.0, (3, 3)),
                   ((127.0, 60.0), 0.7, (9, 7))]
        partial_seen = 0
        for k, ((ci, cj), yaw, shape) in enumerate(updates):
            pose = (ORIGIN[0] + ci * RES, ORIGIN[1] + cj * RES, yaw)
            g = local_grid(rng, *shape)
            got = m.update(g, pose)
            want_upd = wref.update(g, pose)
            assert got == want_upd and got[0] > 0, (k, got, want_upd)
            stmt.mark(*want_upd)
            agree(f"update {k}", partial=None if wide else True)
            partial_seen += not stmt.last_full
        assert wide or partial_seen == len(updates)
        nothing = np.full((5, 5), -1, np.int32)
        assert m.update(nothing, (ORIGIN[0] + 1.0, ORIGIN[1] + 1.0, 0.1))[0] == 0 == wref.update(nothing, (ORIGIN[0] + 1.0, ORIGIN[1] + 1.0, 0.1))[0]
        stmt.mark(0, (-1, -1, -1, -1))
        agree("an update that changed nothing")
        assert m.distance_info()[2] == (-1, -1, -1, -1)
        # two updates merged into one dirty box before anyone reads
        for (ci, cj) in ((20.0, 10.0), (70.0, 50.0)):
            pose = (ORIGIN[0] + ci * RES, ORIGIN[1] + cj * RES, 0.5)
            g = local_grid(rng, 5, 5, p_seen=1.0)
            got = m.update(g, pose)
            assert got == wref.update(g, pose)
            stmt.mark(*got)
        agree("merged", partial=None if wide else True)


def test_front_ends():
    import kompass_cpp
    from kompass_core.mapping import WorldMap

    W, H = 70, 45
    c = world(W, H, "seeded")
    m = WorldMap(W, H, RES, ORIGIN)
    m.set_prior(c)
    with pytest.raises(RuntimeError):
        m.distance_field()
    assert m.enable_distance(reach_m=0.22) == 5                  # ceil(4.4)
    want5 = dref.dist2_plane(c, 5)
    got = m.distance_field()
    assert got.dtype == np.uint16 and got.shape == (W, H) and np.array_equal(got, want5)
    metres = m.distance_field(metres=True)
    assert metres.dtype == np.float32 and np.isinf(metres[want5 == dref.FAR]).all()
    near = want5 != dref.FAR
    assert np.array_equal(metres[near], np.sqrt(want5[near].astype(np.float32)) * np.float32(RES))
    i, j = (int(v) for v in np.argwhere(want5 == 4)[0])
    assert m.distance_at(ORIGIN[0] + i * RES + 0.01, ORIGIN[1] + j * RES - 0.01) == 2.0 * float(np.float32(RES))
    assert m.distance_at(ORIGIN[0] - 1.0, ORIGIN[1]) == float("inf")
    with pytest.raises(TypeError):
        m.enable_distance()
    assert m.enable_distance(reach_cells=2, unknown_blocks=True) == 2
    assert np.array_equal(m.distance_field(), dref.dist2_plane(c, 2, dref.UNKNOWN_BLOCKS))
    with pytest.raises(IndexError):
        m.enable_distance(reach_cells=255)
    m.enable_distance(reach_cells=0)
    with pytest.raises(RuntimeError):
        m.distance_field()
    # the class itself
    cm = kompass_cpp.mapping.WorldMap(width=W, height=H, resolution=RES, origin_x=ORIGIN[0], origin_y=ORIGIN[1])
    assert cm.distance_reach == 0
    cm.set_prior(c)
    cm.enable_distance(16)
    assert cm.distance_reach == 16 and np.array_equal(cm.distance_field(), dref.dist2_plane(c, 16))
    assert cm.distance_last_box() == (0, 0, W - 1, H - 1) and cm.device_distance_ptr() != 0
    assert cm.distance_last_box() == (-1, -1, -1, -1)
