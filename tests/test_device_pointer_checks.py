"""The one check behind every "this memory is already on the device" entry point (check_device_range, kc_common.hip),
through the three calls that use it: kc_cloud_grid_extent with data_on_device = 1, kc_planner_set_grid_device and
the depth detector's device-frame path.

Each case works in one allocation of twice the object's size whose halves hold different data: an object the
allocation holds is accepted and gives what the host-memory call gives on the same data; a host pointer, an object
that ends one element past the allocation, a misaligned grid and a frame that starts in front of it are refused
with KC_ERR_INVALID before anything is read."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402

from helpers import DeviceArray, hip_runtime  # noqa: E402


class Cloud:
    """64 xyz points of 12 bytes; an element is a point."""
    noun, n, elem = "cloud", 64, 12

    def __init__(self):
        self.ctx = kh.CloudContext()
        rng = np.random.default_rng(11)
        self.host = rng.uniform(-2.0, 2.0, (2 * self.n, 3)).astype(np.float32)

    def on_host(self, half):
        return self.ctx.occupancy_grid(self.host[half * self.n:(half + 1) * self.n], 0.25, -0.5, 1.0)

    def on_host_all(self):
        return self.ctx.occupancy_grid(self.host, 0.25, -0.5, 1.0)

    def on_device(self, ptr, n=None):
        n = self.n if n is None else n
        return self.ctx.occupancy_grid(None, 0.25, -0.5, 1.0, device_ptr=ptr, n_points=n, nbytes=n * self.elem)


class Grid:
    """An 8 x 8 int32 grid (n cells as an n x 1 grid where the case asks for another length)."""
    noun, n, elem = "grid", 64, 4

    def __init__(self):
        self.ctx = kh.PlannerContext()
        rng = np.random.default_rng(12)
        self.host = rng.choice(np.array([-1, 0, 0, 0, 0, 100], np.int32), 2 * self.n)
        self.host[[0, 63, 64, 127]] = 0   # the ends of the solve are free

    def _solve(self):
        return self.ctx.solve((0, 0), (7, 7)) + self.ctx.field()

    def on_host(self, half):
        self.ctx.set_grid(self.host[half * self.n:(half + 1) * self.n].reshape(8, 8, order="F"))
        return self._solve()

    def on_host_all(self):
        self.ctx.set_grid(self.host.reshape(8, 16, order="F"))
        return self._solve()

    def on_device(self, ptr, n=None):
        shape = {None: (8, 8), 2 * self.n: (8, 16)}.get(n, (n, 1))
        self.ctx.set_grid_device(ptr, *shape, elem_bytes=4)
        return self._solve()


class Frame:
    """An 8 x 8 uint16 frame in row-major order (a 1 x n frame where the case asks for another length)."""
    noun, n, elem = "frame", 64, 2
    boxes = [(0, 0, 7, 7), (2, 1, 3, 4)]

    def __init__(self):
        self.ctx = kh.DepthContext(np.array([0.1, 10.0], np.float32), [0, 0, 0], [0, 0, 0, 1], [500.0, 500.0],
                                   [4.0, 4.0], 1e-3)
        rng = np.random.default_rng(13)
        self.host = rng.integers(50, 12000, 2 * self.n).astype(np.uint16)

    def on_host(self, half, flip=False):
        img = self.host[half * self.n:(half + 1) * self.n].reshape(8, 8)
        return self.ctx.box_stats(img[::-1] if flip else img, self.boxes)

    def on_host_all(self):
        return self.ctx.box_stats(self.host.reshape(16, 8), self.boxes)

    def on_device(self, ptr, n=None, strides=None):
        shape = {None: (8, 8), 2 * self.n: (16, 8)}.get(n, (1, n))
        return self.ctx.box_stats(None, self.boxes, device_ptr=ptr, shape=shape, strides=strides or (shape[1], 1))


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


def refused(case, word, call, *args, **kw):
    """KC_ERR_INVALID (ValueError, "[kc -1]") whose message names the object and carries `word`."""
    with pytest.raises(ValueError) as e:
        call(*args, **kw)
    msg = str(e.value)
    assert "[kc -1]" in msg and f"device {case.noun}" in msg and word in msg, msg


@pytest.fixture(scope="module", params=[Cloud, Grid, Frame], ids=["cloud", "grid", "frame"])
def case(request):
    assert kh.device_count() >= 1, "no HIP device visible"
    c = request.param()
    yield c
    c.ctx.close()


def test_host_pointer_is_refused(case):
    """Pageable host memory: HIP either does not know the address or reports it as no device memory."""
    with pytest.raises(ValueError) as e:
        case.on_device(case.host.ctypes.data)
    msg = str(e.value)
    assert "[kc -1]" in msg and f"device {case.noun}" in msg, msg
    assert "is not memory HIP knows" in msg or "is not device memory" in msg, msg


def test_range_inside_one_allocation(case):
    half = case.n * case.elem
    with DeviceArray(case.host) as dev:
        assert dev.nbytes == 2 * half
        refused(case, "outside", case.on_device, dev.ptr, 2 * case.n + 1)    # one element past the end, from the base
        same(case.on_device(dev.ptr), case.on_host(0))                       # at the base
        same(case.on_device(dev.ptr, 2 * case.n), case.on_host_all())        # the whole allocation, to its last byte
        same(case.on_device(dev.ptr + half), case.on_host(1))                # from the middle to the very end
        refused(case, "outside", case.on_device, dev.ptr + half, case.n + 1)  # the same start, one element more
        same(case.on_device(dev.ptr), case.on_host(0))                       # a refusal leaves the context usable


def test_misaligned_grid_is_refused():
    case = Grid()
    with DeviceArray(case.host) as dev:
        refused(case, "aligned", case.on_device, dev.ptr + 2)   # inside the allocation: only the alignment refuses it
    case.ctx.close()


def test_negative_row_stride():
    case = Frame()
    with DeviceArray(case.host) as dev:
        last_row = dev.ptr + 7 * 8 * 2                          # the frame's first element; its lowest byte is the base
        same(case.on_device(last_row, strides=(-8, 1)), case.on_host(0, flip=True))
        refused(case, "outside", case.on_device, last_row - 8 * 2, strides=(-8, 1))   # one row down: 16 bytes in front
    case.ctx.close()


def test_memory_of_another_device_is_refused(case):
    if kh.device_count() < 2:
        pytest.skip("needs a second visible device")
    hip = hip_runtime()
    assert hip.hipSetDevice(1) == 0
    try:
        dev = DeviceArray(case.host)
    finally:
        assert hip.hipSetDevice(0) == 0
    with dev:
        refused(case, "lives on device 1", case.on_device, dev.ptr)
