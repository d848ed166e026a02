"""The depth histogram kernel (kc_depth.hip) at its counter, chunk, rank and band edges, bit for bit against the
restatement (depth_detector_ref.py).  The scenes are depth_scenes.py; test_depth_detector_cpu.py asserts on the
restatement alone that every scene reaches the edge it is named after.

What each group would catch:
- counter_*: a carry between the two 16-bit halves of an LDS word, or a lost count where one counter reaches the
  whole chunk ("a chunk never reaches 65536 of one value"), and the 32-bit global sum of saturated halves;
- chunk_*: the chunk limits p0 / p1, chunks that keep nothing, the kept count and the occupied span handed over
  by the ticket, slot numbering with several multi-chunk boxes in flight;
- rank_*: the lane that holds the selected rank in every pass ("exactly one lane"), bucket 255, the rank + 1 key
  when the selected key repeats past the rank and when it does not ("rank + 1 has the key x too");
- band_*: >= and <= of the band tests where a kept value lies exactly on a limit;
- view_*: strides of either sign and order of a frame read in place."""
import numpy as np
import pytest

import depth_scenes
from depth_detector_ref import Detector
from helpers import DeviceArray
from test_depth_detector_gpu import FOCAL, PRINCIPAL, TILT, check

pytestmark = pytest.mark.gpu

STATE = (1.0, 2.0, 0.3)


def pair_of(depth_range, factor):
    import kompass_hip as kh

    args = (np.array(depth_range, np.float32), TILT[0], TILT[1], FOCAL, PRINCIPAL, factor)
    return kh.DepthContext(*args), Detector(*args)


def run_scene(name):
    frame, boxes, depth_range, factor, _ = depth_scenes.SCENES[name].build()
    ctx, det = pair_of(depth_range, factor)
    return check(ctx, det, frame, boxes, state=STATE)


@pytest.mark.parametrize("name", depth_scenes.names("counter_"))
def test_counter_limits(name):
    assert run_scene(name) == 1


@pytest.mark.parametrize("name", depth_scenes.names("chunk_"))
def test_chunk_edges(name):
    kept = run_scene(name)
    if "kept0" in name or "kept1" in name:
        assert kept == 0
    else:
        assert kept >= 1


@pytest.mark.parametrize("name", depth_scenes.names("rank_"))
def test_rank_edges(name):
    assert run_scene(name) == 1


@pytest.mark.parametrize("name", depth_scenes.names("band_"))
def test_band_edges(name):
    assert run_scene(name) == 1


SPREAD = [n for n in depth_scenes.names("rank_") + depth_scenes.names("band_") if depth_scenes.SCENES[n].nbins < 65536]


@pytest.mark.parametrize("name", SPREAD)
def test_rank_and_band_edges_from_the_global_histogram(name):
    """The small scenes again as a box of three chunks, so that the select and the band loop read the 32-bit global
    histogram: the scene's pixels are spread over a frame of the first raw value above the kept interval.  The kept
    values are the scene's own, so its claim holds as it stands.  (Where every uint16 value is kept nothing can be
    rejected: those scenes have *_chunks versions of their own.)"""
    small, boxes, depth_range, factor, _ = depth_scenes.SCENES[name].build()
    d_lo, nbins = depth_scenes.raw_interval(depth_range, factor)
    chunk = depth_scenes.chunk_of(nbins)
    v = small.reshape(-1)
    n_px = 2 * chunk + 1
    flat = np.full(n_px, d_lo + nbins, np.uint16)
    where = np.arange(v.size) * (n_px // v.size) + 3
    assert where.max() < n_px and where[-1] // chunk > where[0] // chunk
    flat[where] = v
    frame = flat.reshape(depth_scenes.SHAPE[n_px])
    box = depth_scenes.whole(frame)
    np.testing.assert_array_equal(depth_scenes.kept_values(frame, box, depth_range, factor),
                                  depth_scenes.kept_values(small, boxes[0], depth_range, factor))
    ctx, det = pair_of(depth_range, factor)
    assert check(ctx, det, frame, [box], state=STATE) == 1


@pytest.mark.parametrize("name", depth_scenes.names("view_"))
def test_device_resident_views(name):
    frame, boxes, depth_range, factor, _ = depth_scenes.SCENES[name].build()
    root = depth_scenes.root_of(frame)
    first = frame.__array_interface__["data"][0] - root.__array_interface__["data"][0]
    h, w = frame.shape
    ends = [first + a * (h - 1) * frame.strides[0] + b * (w - 1) * frame.strides[1] for a in (0, 1) for b in (0, 1)]
    assert min(ends) >= 0 and max(ends) + 2 <= root.nbytes  # wholly inside the allocation
    ctx, det = pair_of(depth_range, factor)
    with DeviceArray(root) as dev:
        assert dev.nbytes == root.nbytes
        kept = check(ctx, det, None, boxes, state=STATE, host=frame, device_ptr=dev.ptr + first, shape=frame.shape,
                     strides=[s // 2 for s in frame.strides])
        assert ctx.last_upload() == 0
    assert kept >= 4
    assert check(ctx, det, frame, boxes, state=STATE) == kept  # the same view from the host
    assert ctx.last_upload() > 0


def test_one_context_shrinking_and_growing():
    """A multi-chunk call over every raw value, a one-pixel box, the multi-chunk call again: the global histogram
    and the per-box counters are zeroed to the size of each call."""
    frame, boxes, depth_range, factor, _ = depth_scenes.SCENES["shrink_grow"].build()
    ctx, det = pair_of(depth_range, factor)
    assert check(ctx, det, frame, boxes[:2], state=STATE) == 2
    assert check(ctx, det, frame, boxes[2:], state=STATE) == 0
    assert check(ctx, det, frame, boxes[:2], state=STATE) == 2
    assert check(ctx, det, frame, boxes[1:2] + boxes[2:] + boxes[:1], state=STATE) == 2  # the slots the other way
