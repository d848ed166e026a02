"""The torch check of test_planner_frontier_gpu.py, run in a fresh process by it: torch is imported BEFORE kompass_cpp, so
that the process has one HIP runtime (torch's).  A map that is a torch tensor on the device goes to
find_frontiers through __cuda_array_interface__ and gives what the same map gives as a host array, which is the
statement's.  Not collected by pytest."""
import sys
from pathlib import Path

import torch  # noqa: I001  (first: see above)

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kompass-core_amd"), str(Path(__file__).resolve().parent)]

import numpy as np  # noqa: E402

import planner_frontier_ref as fref  # noqa: E402
import planner_ref as ref  # noqa: E402
from kompass_core.planning import GridPlanner  # noqa: E402
from test_planner_frontier_cpu import ragged  # noqa: E402
from test_planner_gpu import _robot  # noqa: E402

W, H, RES = 150, 70, 0.05
ORIGIN = (-2.0, 1.0)


def main():
    grid = ragged((W, H), 0.03, 23)                        # grid[i, j], i along x
    meta = dict(origin_x=ORIGIN[0], origin_y=ORIGIN[1], width=W, height=H, resolution=RES)
    r2 = ref.radius_to_r2(0.1, RES)
    free = np.argwhere(fref.explore_validity(grid, r2))
    cell = tuple(int(v) for v in free[len(free) // 2])
    xy = [float(ref.cell_to_world(c, o, RES)) + 0.01 for c, o in zip(cell, ORIGIN)]
    want = fref.explore(grid, cell, r2, 0, 3)
    assert want["status"] == ref.FOUND
    fe = GridPlanner(_robot())
    host = fe.find_frontiers(xy[0], xy[1], map=grid, map_meta_data=meta, min_size=3)
    assert [f.entry_cell for f in host] == [r["entry"] for r in want["frontiers"]]
    assert [(f.size, f.root) for f in host] == [(r["size"], r["root"]) for r in want["frontiers"]]
    for dtype in (torch.int32, torch.int8):
        # a C-contiguous (height, width) tensor, as an image of the map; its transpose is grid[i, j] column-major
        img = torch.from_numpy(np.ascontiguousarray(grid.T)).to(dtype).cuda()
        dev = GridPlanner(_robot())
        got = dev.find_frontiers(xy[0], xy[1], map=img.T, map_meta_data=meta, min_size=3)   # read in place
        assert got == host and dev.components == want["components"]
        np.testing.assert_array_equal(np.asarray(dev.frontier_labels()), want["labels"])
        for k, path in enumerate(want["paths"]):
            np.testing.assert_array_equal(dev.frontier_path_cells(k), path)
        path = dev.explore(xy[0], xy[1], map=img.T, map_meta_data=meta, min_size=3)
        np.testing.assert_array_equal(np.asarray(path.x()), ref.cell_to_world(want["paths"][0][:, 0], ORIGIN[0], RES).astype(np.float32))


if __name__ == "__main__":
    main()
    torch.cuda.synchronize()
    print("ok")
