"""Create, use, destroy -- eight times in one process for each of the seven device contexts, with the smallest real
call in between: every round's result is bit-identical to the first.  The contexts' buffers free themselves when the
context is deleted (DevBuf / PinBuf / Timing in kc_internal.h); a buffer that was moved from and then used, or freed
twice (HIP reports that as an error, not a fault), shows here as a failing call or a different result.

What this does NOT measure is leaked device memory: hipMemGetInfo is device-wide, and on a shared card other
processes' allocations swamp it.  That no buffer leaks rests on the types (move-only, freeing destructors, the
static_asserts beside them) and on review.

kc_depth opens its device lazily: its create function takes any device index and the first compute call refuses
an index out of range; every other create function refuses it itself."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import synthetic as syn  # noqa: E402

ROUNDS = 8
RNG = np.random.default_rng(21)
ANGLES32, RANGES32 = syn.dense_scan(32, 0.2)
POINTS64 = RNG.uniform(-2.0, 2.0, (64, 3)).astype(np.float32)
GRID8 = RNG.choice(np.array([0, 0, 0, 0, 100], np.int32), (8, 8))
GRID8[0, 0] = GRID8[7, 7] = 0
FRAME8 = RNG.integers(50, 12000, (8, 8)).astype(np.uint16)
LIMITS = kh.make_limits(syn.LIMITS["vx"], syn.LIMITS["vy"], syn.LIMITS["omega"])


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert kh.device_count() >= 1, "no HIP device visible"


def _dwa_inputs():
    inp = syn.make_controller_inputs("cfg1", seed=1)
    vx, vy, om = syn.lattice_nonholonomic(2, 8)
    assert len(vx) == 16
    return dict(inp, vx=vx, vy=vy, omega=om, points=np.ascontiguousarray(inp["points"][:64], np.float32), P=8)


def make_dwa(device=0):
    inp = _dwa_inputs()
    rb = inp["robot"]
    return kh.DwaContext(rb["shape"], rb["dims"], (0, 0, 0), (0, 0, 0, 1), inp["octree_res"], inp["dt"], max_samples=64,
                         max_points=inp["P"], max_segment=len(inp["seg_xyz"]), max_obstacles=64,
                         acc_limits=inp["acc_limits"], device=device)


def use_dwa(ctx):
    """One 16-sample cycle."""
    inp = _dwa_inputs()
    ctx.set_weights(kh.make_weights(*inp["weights"]))
    ctx.set_points(inp["state"], inp["points"], inp["max_range"])
    ctx.set_tracked_segment(inp["seg_xyz"], inp["acc_at_seg"], inp["ref_len"])
    ctx.set_samples(inp["vx"], inp["vy"], inp["omega"])
    r = ctx.cycle(inp["state"], inp["P"])
    px, py, raw, costs = ctx.get_samples(with_costs=True)
    assert r.n_samples == 16
    return [np.array([r.found, r.index, r.raw_index, r.n_admissible]), np.float32(r.cost), px, py, raw, costs]


def make_mapper(device=0):
    return kh.MapperContext(32, 32, 0.1, (0, 0, 0), 0.0, 32, device=device)


def use_mapper(ctx):
    """One 32-beam scan into a 32 x 32 grid."""
    return [ctx.scan_to_grid(ANGLES32, RANGES32)]


def make_cloud(device=0):
    return kh.CloudContext(1 << 12, 64, device=device)


def use_cloud(ctx):
    """64 points to an occupancy grid."""
    return list(ctx.occupancy_grid(POINTS64, 0.25, -0.5, 1.0))


def make_zone(device=0):
    return kh.ZoneContext(kh.CYLINDER, [0.1, 0.4], (0, 0, 0), (0, 0, 0, 1), 160.0, 0.3, 0.6, ANGLES32, 0.1, 2.0, 20.0,
                          device=device)


def use_zone(ctx):
    """One 32-beam check in each direction."""
    r = np.linspace(0.2, 1.5, 32)
    return [np.float32(ctx.check(r, True)), np.float32(ctx.check(r, False))]


def make_depth(device=0):
    return kh.DepthContext(np.array([0.1, 10.0], np.float32), [0, 0, 0], [0, 0, 0, 1], [500.0, 500.0], [4.0, 4.0], 1e-3,
                           device=device)


def use_depth(ctx):
    """Two boxes on an 8 x 8 frame."""
    return list(ctx.box_stats(FRAME8, [(0, 0, 7, 7), (2, 1, 3, 4)]))


def make_dvz(device=0):
    return kh.DvzContext(64, device=device)


def use_dvz(ctx):
    """One 32-beam deformation."""
    out = ctx.deform((1.0, 0.6, 0.1, 0.0, 0.0), ANGLES32, RANGES32 * 0.5, radii=True)
    return [np.array(out[:3]), out[3]]


def make_planner(device=0):
    return kh.PlannerContext(device=device)


def use_planner(ctx):
    """One 8 x 8 solve and its path."""
    ctx.set_grid(GRID8)
    return [np.array(ctx.solve((0, 0), (7, 7))), ctx.path(), *ctx.field()]


CONTEXTS = {"dwa": (make_dwa, use_dwa), "mapper": (make_mapper, use_mapper), "cloud": (make_cloud, use_cloud),
            "zone": (make_zone, use_zone), "depth": (make_depth, use_depth), "dvz": (make_dvz, use_dvz),
            "planner": (make_planner, use_planner)}


def bits(values):
    return [np.asarray(v).copy().tobytes() for v in values]


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_create_use_destroy_rounds(name):
    make, use = CONTEXTS[name]
    first = None
    for _ in range(ROUNDS):
        ctx = make()
        got = bits(use(ctx))
        ctx.close()
        if first is None:
            first = got
        assert got == first


def test_dwa_patterns_change_places_before_destroy():
    """Two sample patterns alternate across the cycles of one context: from the third cycle on find_pattern moves
    the pattern's buffers between the context and a kept slot, and every cycle repeats the first of its pattern."""
    inp = _dwa_inputs()
    ctx = make_dwa()
    ctx.set_weights(kh.make_weights(*inp["weights"]))
    seg, acc = np.asarray(inp["seg_xyz"], np.float32), np.ascontiguousarray(inp["acc_at_seg"], np.float32)
    curs = [(0.6, 0.0, 0.0), (0.0, 0.0, 0.3)]
    first = {}
    for i in range(10):
        cur = curs[i % 2]
        r = ctx.find_best_path(inp["state"], inp["P"], window=(syn.DIFFERENTIAL_DRIVE, LIMITS, cur, 4, 5),
                               points=inp["points"], max_sensor_range=inp["max_range"], segment=(seg, acc, inp["ref_len"]))
        got = bits([np.array([r.found, r.index, r.raw_index, r.n_admissible, r.n_samples]), np.float32(r.cost),
                    *(ctx.get_best() if r.found else ())])
        assert got == first.setdefault(i % 2, got)
    assert ctx.get_option("pattern_hits") >= 4
    ctx.close()


def test_destroy_takes_a_null_handle():
    for name in ("kc_dwa_destroy", "kc_mapper_destroy", "kc_cloud_destroy", "kc_zone_destroy", "kc_depth_destroy",
                 "kc_dvz_destroy", "kc_planner_destroy", "kc_comm_destroy"):
        getattr(kh.lib(), name)(None)


def _floats(*values):
    return (C.c_float * len(values))(*values)


def create_dwa(device, h):
    p = kh.DwaParams()
    p.shape, p.ndims, p.octree_res, p.time_step, p.max_samples, p.max_points = kh.CYLINDER, 2, 0.05, 0.1, 16, 8
    p.dims[0], p.dims[1], p.sensor_rot_xyzw[3], p.device = 0.1, 0.4, 1.0, device
    return kh.lib().kc_dwa_create(C.byref(p), h)


def create_mapper(device, h):
    return kh.lib().kc_mapper_create(32, 32, 0.1, _floats(0, 0, 0), 0.0, 32, device, h)


def create_cloud(device, h):
    return kh.lib().kc_cloud_create(1 << 12, 64, device, h)


def create_zone(device, h):
    return kh.lib().kc_zone_create(kh.CYLINDER, _floats(0.1, 0.4), 2, _floats(0, 0, 0), _floats(0, 0, 0, 1), 160.0, 0.3, 0.6,
                                   ANGLES32.ctypes.data_as(C.POINTER(C.c_double)), 32, 0.1, 2.0, 20.0, device, h)


def create_dvz(device, h):
    return kh.lib().kc_dvz_create(device, 64, h)


def create_planner(device, h):
    return kh.lib().kc_planner_create(device, h)


CREATE = {"dwa": create_dwa, "mapper": create_mapper, "cloud": create_cloud, "zone": create_zone, "dvz": create_dvz,
          "planner": create_planner}


@pytest.mark.parametrize("name", list(CONTEXTS))
@pytest.mark.parametrize("device", [-1, None], ids=["negative", "one_past"])
def test_device_index_out_of_range(name, device):
    """KC_ERR_HIP and a null handle from the create function (kc_depth: KC_ERR_HIP from the first compute call)."""
    device = kh.device_count() if device is None else device
    if name == "depth":
        ctx = make_depth(device)
        with pytest.raises(kh.KompassHipError, match=r"\[kc -3\].*not available"):
            use_depth(ctx)
        ctx.close()
        return
    h = C.c_void_p(1)
    assert CREATE[name](device, C.byref(h)) == -3   # KC_ERR_HIP
    assert h.value is None
    assert "not available" in kh.lib().kc_last_error().decode()
