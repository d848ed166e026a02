"""The torch check of test_planner_gpu.py, run in a fresh process by it: torch is imported BEFORE kompass_cpp, so
that the process has one HIP runtime (torch's).  A grid that is a torch tensor on the device goes to
GridPlanner.set_grid through __cuda_array_interface__ and gives the field of the same grid as a host array.  Not
collected by pytest."""
import sys
from pathlib import Path

import torch  # noqa: I001  (first: see above)

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kompass-core_amd"), str(Path(__file__).resolve().parent)]

import numpy as np  # noqa: E402

import kompass_cpp  # noqa: E402
import kompass_hip as kh  # noqa: E402
import planner_ref as ref  # noqa: E402

W, H, RES = 150, 70, 0.05
ORIGIN = (-2.0, 1.0)


def refused(kind, call):
    try:
        call()
    except kind:
        return
    raise AssertionError(f"accepted where {kind.__name__} was due")


def solved(p, start, goal):
    p.setup_problem(start[0], start[1], 0.0, goal[0], goal[1], 0.0)
    ok = p.solve()
    f, v = p.get_field()
    return ok, p.get_status(), p.get_cost(), np.array(p.get_path_cells()), np.array(f), np.array(v)


def main():
    rng = np.random.default_rng(23)
    grid = np.where(rng.random((W, H)) < 0.03, 100, 0).astype(np.int32)   # grid[i, j], i along x
    grid[rng.random((W, H)) < 0.02] = -1
    radius = 0.06
    r2 = ref.radius_to_r2(radius, RES)
    valid = ref.validity(grid, r2, False)
    # both ends in one connected component of the statement's field
    seed = tuple(int(c) for c in np.argwhere(valid)[0])
    reach = ref.cost_field(valid, seed)
    far = tuple(int(c) for c in np.unravel_index(np.argmax(np.where(reach == ref.INF, 0, reach)), reach.shape))
    assert reach[far] > 10 * 50
    xy = lambda c: (float(ref.cell_to_world(c[0], ORIGIN[0], RES)) + 0.01, float(ref.cell_to_world(c[1], ORIGIN[1], RES)) + 0.01)
    want = ref.plan(grid, ORIGIN, RES, xy(far), xy(seed), radius, False)
    assert want["status"] == ref.FOUND

    G = kompass_cpp.types.RobotGeometry
    p = kompass_cpp.planning.GridPlanner(G.SPHERE, [radius], allow_unknown=False)
    p.set_space_bounds_from_map(ORIGIN[0], ORIGIN[1], W, H, RES)
    assert p.get_footprint_r2() == r2
    p.set_grid(grid)
    host = solved(p, xy(far), xy(seed))
    assert host[0] and host[1] == ref.FOUND
    np.testing.assert_array_equal(host[3], want["cells"])
    np.testing.assert_array_equal(host[4], ref.cost_field(valid, seed))
    np.testing.assert_array_equal(host[5].astype(bool), valid)

    # a new grid forgets the last solve: no path and no cost until the next one, and no exception
    p.set_grid(grid)
    assert p.get_solution() is None and p.get_cost() == float("inf") and p.get_status() == -1
    assert len(p.get_path_cells()) == 0

    for dtype in (torch.int32, torch.int8):
        # a C-contiguous (height, width) tensor, as an image of the map; its transpose is grid[i, j] column-major
        img = torch.from_numpy(np.ascontiguousarray(grid.T)).to(dtype).cuda()
        t = img.T
        assert tuple(t.shape) == (W, H) and not t.is_contiguous()
        p.set_grid(t)                                      # ordered after torch's stream, read in place
        assert p.get_solution() is None
        got = solved(p, xy(far), xy(seed))
        assert got[:3] == host[:3]
        for a, b in zip(got[3:], host[3:]):
            np.testing.assert_array_equal(a, b)
        # by address, after the producer's stream
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            img2 = img.clone()
        p.set_grid(np.zeros((W, H), np.int32))
        ctx = kh.PlannerContext()
        ctx.after_stream(side.cuda_stream)
        ctx.set_grid_device(img2.data_ptr(), W, H, elem_bytes=img2.element_size())
        st, cost, _ = ctx.solve(far, seed, r2, False)
        assert st == ref.FOUND and cost == host[4][far]
        np.testing.assert_array_equal(ctx.field()[0], host[4])
        np.testing.assert_array_equal(ctx.path(), host[3])
        ctx.after_stream(None)
        ctx.close()
        side.synchronize()
        p.set_grid_device(img2.data_ptr(), img2.element_size())
        got = solved(p, xy(far), xy(seed))
        assert got[:3] == host[:3]
        np.testing.assert_array_equal(got[4], host[4])

    # what set_grid refuses before any read
    rows = torch.from_numpy(grid).cuda()                   # (width, height) row-major: not the grid's layout
    assert rows.is_contiguous()
    refused(ValueError, lambda: p.set_grid(rows))
    refused(ValueError, lambda: p.set_grid(rows.T))        # column-major, but height x width: not the announced shape
    refused(TypeError, lambda: p.set_grid(rows.T.to(torch.float32)))
    refused(ValueError, lambda: p.set_grid(torch.zeros((W, H, 1), dtype=torch.int32, device="cuda")))

    class Masked:
        __cuda_array_interface__ = dict(img.T.__cuda_array_interface__, mask=object())

    refused(ValueError, lambda: p.set_grid(Masked()))

    class StreamZero:
        __cuda_array_interface__ = dict(img.T.__cuda_array_interface__, stream=0, version=3)

    refused(ValueError, lambda: p.set_grid(StreamZero()))

    class OnStream:  # version 3 with the legacy default stream named
        __cuda_array_interface__ = dict(img.T.__cuda_array_interface__, stream=1, version=3)

    p.set_grid(OnStream())
    got = solved(p, xy(far), xy(seed))
    assert got[:3] == host[:3]
    np.testing.assert_array_equal(got[4], host[4])


if __name__ == "__main__":
    main()
    torch.cuda.synchronize()
    print("ok")
