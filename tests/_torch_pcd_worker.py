"""The torch check of test_pcd_grid_gpu.py, run in a fresh process by it: torch is imported BEFORE kompass_cpp, so
that the process has one HIP runtime (torch's).  Not collected by pytest."""
import sys
from pathlib import Path

import torch  # noqa: I001  (first: see above)

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kompass-core_amd"), str(Path(__file__).resolve().parent)]

import numpy as np  # noqa: E402

import kompass_cpp  # noqa: E402
import kompass_hip as kh  # noqa: E402
import pcd_ref  # noqa: E402
import synthetic as syn  # noqa: E402

Z0, ZR = 0.1, 1.0


def same(got, want):
    grid, origin = got
    assert grid.shape == want[0].shape and [float(v) for v in origin] == [float(v) for v in want[1]]
    np.testing.assert_array_equal(np.asarray(grid).view(np.uint8), want[0].view(np.uint8))


def main():
    pts = syn.pcd_indoor_map(1_000_003, seed=40)
    pts[::777, 1] = np.nan
    for res in (0.05, 0.25):
        want = pcd_ref.grid(pts, res, Z0, ZR)
        same(kompass_cpp.utils.points_to_occupancy_grid(pts, res, Z0, ZR), want)
        t = torch.from_numpy(pts).cuda()
        same(kompass_cpp.utils.points_to_occupancy_grid(t, res, Z0, ZR), want)  # ordered after torch's stream
        # a strided view: x y z of (N, 4) records
        t4 = torch.zeros((len(pts), 4), dtype=torch.float32, device="cuda")
        t4[:, :3] = t
        v = t4[:, :3]
        assert not v.is_contiguous()
        same(kompass_cpp.utils.points_to_occupancy_grid(v, res, Z0, ZR), want)
        # a view that starts inside the allocation (12-byte records that are not 16-byte aligned)
        same(kompass_cpp.utils.points_to_occupancy_grid(t[1:], res, Z0, ZR), pcd_ref.grid(pts[1:], res, Z0, ZR))
        # the ctypes binding, by address
        torch.cuda.synchronize()
        c = kh.CloudContext()
        same(c.occupancy_grid(None, res, Z0, ZR, device_ptr=t.data_ptr(), n_points=len(pts)), want)
        # a cloud described larger than its allocation is refused before any read
        try:
            c.occupancy_grid(None, res, Z0, ZR, device_ptr=t.data_ptr(), n_points=len(pts) * 1000)
        except ValueError as e:
            assert "outside" in str(e)
        else:
            raise AssertionError("an oversized device cloud was accepted")
        try:
            c.occupancy_grid(None, res, Z0, ZR, device_ptr=pts.ctypes.data, n_points=len(pts))  # a host address
        except ValueError:
            pass
        else:
            raise AssertionError("a host address was accepted as a device cloud")
        c.close()
    class NoRows:  # what some producers report for an array without rows
        __cuda_array_interface__ = {"shape": (0, 3), "typestr": "<f4", "data": (0, False), "strides": (0, 4), "version": 3}

    same(kompass_cpp.utils.points_to_occupancy_grid(NoRows(), 0.05, Z0, ZR),
         pcd_ref.grid(np.zeros((0, 3), np.float32), 0.05, Z0, ZR))
    same(kompass_cpp.utils.points_to_occupancy_grid(torch.zeros((0, 3), device="cuda"), 0.05, Z0, ZR),
         pcd_ref.grid(np.zeros((0, 3), np.float32), 0.05, Z0, ZR))


if __name__ == "__main__":
    main()
    torch.cuda.synchronize()
    print("ok")
