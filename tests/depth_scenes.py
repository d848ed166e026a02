"""Hand-designed scenes that drive the depth histogram kernel (kc_depth.hip) to its counter, chunk, rank and band
edges, for the tests.  Not collected by pytest.

Every builder returns (frame, boxes, depth_range, factor, claim).  factor is 1.0 or 0.5, so every depth is an exact
float and a scene can be checked by hand.  claim(stats, kept) is a predicate over the restatement's own
(count, median, mad, min_d, max_d) of every box and over the sorted kept depths of every box: it states what the
scene is for, and test_depth_detector_cpu.py asserts it on depth_detector_ref alone, so that no GPU test passes
vacuously.  SCENES also records the raw interval's size and the chunk size each scene is meant to hit.

The kernel's work split, restated here for the claims: the kept raw values are one interval [d_lo, d_lo + nbins),
a box's pixels are cut into chunks of 8192 (nbins <= 16384) or 32768 pixels in the order of the frame's smaller
stride, bins 2j and 2j + 1 share one LDS word."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

F = np.float32
OUT = 60000  # a raw value above every narrow range used here

# depth ranges (factor 1) whose interval just keeps / just leaves the small chunk, and every uint16 value
RANGE_OF_CHUNK = {8192: (0.0, 16383.0), 32768: (0.0, 16384.0)}
NBINS_OF_CHUNK = {8192: 16384, 32768: 16385}
FULL_RANGE = (0.0, 65535.0)
# (rows, cols) with exactly that many pixels (8191 and 65537 are prime)
SHAPE = {8191: (1, 8191), 8192: (64, 128), 8193: (3, 2731), 16384: (128, 128), 16385: (113, 145),
         32767: (151, 217), 32768: (128, 256), 32769: (99, 331), 65536: (256, 256), 65537: (1, 65537)}


def raw_interval(depth_range, factor):
    """(d_lo, nbins) by the rule of kc_depth_create: the raw values d with min <= float(d) * factor <= max."""
    v = np.arange(65536, dtype=np.float32) * F(factor)
    keep = np.flatnonzero((v <= F(depth_range[1])) & (v >= F(depth_range[0])))
    return (int(keep[0]), int(keep[-1] - keep[0] + 1)) if len(keep) else (0, 0)


def chunk_of(nbins):
    return 32768 if nbins > 16384 else 8192


def clipped(frame, box):
    """The box's pixels (inclusive limits, clipped to the frame) as a view, or None."""
    tx, ty, sx, sy = (int(v) for v in box)
    h, w = frame.shape
    y0, y1, x0, x1 = max(ty, 0), min(ty + sy, h - 1), max(tx, 0), min(tx + sx, w - 1)
    return None if y0 > y1 or x0 > x1 else frame[y0:y1 + 1, x0:x1 + 1]


def kept_values(frame, box, depth_range, factor):
    """The kept depths of one box, sorted (float32)."""
    px = clipped(frame, box)
    if px is None:
        return np.zeros(0, np.float32)
    d = px.astype(np.float32) * F(factor)
    return np.sort(d[(d <= F(depth_range[1])) & (d >= F(depth_range[0]))])


def chunks_of(frame, box, chunk):
    px = clipped(frame, box)
    return 0 if px is None else -(-px.size // chunk)


def whole(frame):
    h, w = frame.shape
    return (0, 0, w - 1, h - 1)


def root_of(view):
    """The array that owns a view's memory."""
    while view.base is not None:
        view = view.base
    return view


def _flat(values, shape=None):
    """A C-ordered frame whose whole-frame box reads `values` in chunk order."""
    v = np.asarray(values, np.uint16)
    return np.ascontiguousarray(v.reshape(shape if shape is not None else (1, v.size)))


def _deviations(kept, med):
    return np.sort(np.abs(kept - F(med)))


# ---------------------------------------------------------------- counter limits
def counter_single(chunk, value):
    """One chunk of one raw value: one 16-bit counter reaches the chunk size (0x8000 for the large chunk, in the
    high half of its word when the bin is odd)."""
    frame = np.full(SHAPE[chunk], value, np.uint16)

    def claim(stats, kept):
        n, med, mad, mn, mx = stats[0]
        return (n == chunk == frame.size and bool((kept[0] == F(value)).all()) and med == value and mad == 0
                and mn == value and mx == value)

    return frame, [whole(frame)], RANGE_OF_CHUNK[chunk], 1.0, claim


def counter_split(chunk):
    """One chunk, half in bin 2j and half in bin 2j + 1: both halves of one word at chunk / 2."""
    rng = np.random.default_rng(chunk)
    frame = _flat(rng.permutation(np.repeat([1000, 1001], chunk // 2)), SHAPE[chunk])

    def claim(stats, kept):
        n, med, mad, mn, mx = stats[0]
        k = kept[0]
        return (n == chunk and int((k == 1000).sum()) == int((k == 1001).sum()) == chunk // 2
                and 1000 >> 1 == 1001 >> 1 and med == 1000.5 and mad == 0.5 and mn == 1000 and mx == 1001)

    return frame, [whole(frame)], RANGE_OF_CHUNK[chunk], 1.0, claim


def counter_multi(chunk, value):
    """2 * chunk + 1 pixels of one raw value: the global histogram gets two saturated halves and a single count."""
    n_px = 2 * chunk + 1
    frame = np.full(SHAPE[n_px], value, np.uint16)

    def claim(stats, kept):
        n, med, mad, mn, mx = stats[0]
        return (n == n_px and n_px // chunk == 2 and n_px % chunk == 1 and bool((kept[0] == F(value)).all())
                and med == value and mad == 0 and mn == value and mx == value)

    return frame, [whole(frame)], RANGE_OF_CHUNK[chunk], 1.0, claim


# ---------------------------------------------------------------- chunk edges
def chunk_random(chunk, n_px):
    """n_px pixels of random kept values over the whole interval."""
    nbins = NBINS_OF_CHUNK[chunk]
    rng = np.random.default_rng(n_px)
    frame = _flat(rng.integers(0, nbins, n_px), SHAPE[n_px])

    def claim(stats, kept):
        return (stats[0][0] == n_px == len(kept[0]) and chunks_of(frame, whole(frame), chunk) == -(-n_px // chunk)
                and len(np.unique(kept[0])) > 256)

    return frame, [whole(frame)], RANGE_OF_CHUNK[chunk], 1.0, claim


def chunk_first_empty(chunk):
    """Three chunks: nothing kept, random kept values, one kept pixel."""
    nbins = NBINS_OF_CHUNK[chunk]
    n_px = 2 * chunk + 1
    v = np.random.default_rng(chunk + 1).integers(0, nbins, n_px)
    v[:chunk] = OUT
    frame = _flat(v, SHAPE[n_px])

    def claim(stats, kept):
        flat = frame.reshape(-1)
        return bool((flat[:chunk] >= nbins).all()) and bool((flat[chunk:] < nbins).all()) and stats[0][0] == chunk + 1

    return frame, [whole(frame)], RANGE_OF_CHUNK[chunk], 1.0, claim


def chunk_last_empty(chunk):
    """Two chunks: random kept values, then nothing kept."""
    nbins = NBINS_OF_CHUNK[chunk]
    n_px = 2 * chunk
    v = np.random.default_rng(chunk + 2).integers(0, nbins, n_px)
    v[chunk:] = OUT
    frame = _flat(v, SHAPE[n_px])

    def claim(stats, kept):
        flat = frame.reshape(-1)
        return bool((flat[chunk:] >= nbins).all()) and bool((flat[:chunk] < nbins).all()) and stats[0][0] == chunk

    return frame, [whole(frame)], RANGE_OF_CHUNK[chunk], 1.0, claim


def chunk_few_kept(chunk, k):
    """Two chunks with k = 0, 1 or 2 kept pixels in all; the two lie in different chunks, more than 256 bins
    apart (the rank + 1 pass on the global histogram)."""
    n_px = 2 * chunk
    v = np.full(n_px, OUT)
    where = [5, chunk + 7][:k]
    v[where] = [3, 16000][:k]
    frame = _flat(v, SHAPE[n_px])

    def claim(stats, kept):
        n, med, mad, mn, mx = stats[0]
        if n != k or len(kept[0]) != k:
            return False
        if k < 2:
            return med == 0 and mad == 0  # dropped
        return (where[0] // chunk != where[1] // chunk and kept[0][1] - kept[0][0] > 256 and med == 8001.5
                and mad == 7998.5 and mn == 3 and mx == 16000)

    return frame, [whole(frame)], RANGE_OF_CHUNK[chunk], 1.0, claim


def chunk_interleaved(chunk):
    """One call with single-chunk boxes, multi-chunk boxes, boxes with no pixel and exact duplicates of the
    multi-chunk boxes, interleaved: slot numbering and concurrent tickets."""
    nbins = NBINS_OF_CHUNK[chunk]
    frame = np.random.default_rng(chunk + 3).integers(0, 20000, (257, 256)).astype(np.uint16)
    full, mid, edge = (0, 0, 255, 256), (10, 10, 199, 199), (-5, -5, 300, 200)
    small, small2 = (5, 5, 9, 9), (100, 100, 63, 63)
    boxes = [small, full, (300, 0, 5, 5), mid, full, small2, (0, 300, 5, 5), full, mid, (20, 20, -1, 10), edge, small]
    per = 65792, 40000, 50176  # pixels of full, mid, edge (clipped to 196 x 256)
    c_full, c_mid, c_edge = (-(-p // chunk) for p in per)
    expect = [1, c_full, 0, c_mid, c_full, 1, 0, c_full, c_mid, 0, c_edge, 1]

    def claim(stats, kept):
        same = lambda i, j: all(a == b for a, b in zip(stats[i], stats[j]))  # noqa: E731
        return ([chunks_of(frame, b, chunk) for b in boxes] == expect and min(c_full, c_mid, c_edge) >= 2
                and all(stats[i][0] == 0 for i in (2, 6, 9)) and same(1, 4) and same(1, 7) and same(3, 8)
                and same(0, 11) and all(1 < len(kept[i]) < clipped(frame, boxes[i]).size for i in (0, 1, 3, 5, 10))
                and int(frame.max()) >= nbins)

    return frame, boxes, RANGE_OF_CHUNK[chunk], 1.0, claim


# ---------------------------------------------------------------- rank edges
def _rank_scene(values, depth_range, factor, claim, seed=0):
    v = np.random.default_rng(seed).permutation(np.asarray(values))
    frame = _flat(v)
    return frame, [whole(frame)], depth_range, factor, claim


def rank_middle_identical():
    def claim(stats, kept):
        k, n = kept[0], stats[0][0]
        return n == 4 and k[n // 2 - 1] == k[n // 2] == 5 and stats[0][1] == 5

    return _rank_scene([1, 5, 5, 9], (0.0, 100.0), 1.0, claim)


def rank_middle_adjacent():
    def claim(stats, kept):
        k, n = kept[0], stats[0][0]
        return n == 4 and k[n // 2] - k[n // 2 - 1] == 1 and stats[0][1] == 5.5

    return _rank_scene([1, 5, 6, 9], (0.0, 100.0), 1.0, claim)


def rank_middle_far(gap, depth_range, half=50, shape=None):
    """An even count (2 * half) whose upper middle element lies more than `gap` bins above the lower one."""
    rng = np.random.default_rng(gap + half)
    values = np.concatenate([rng.integers(0, 100, half), gap + 100 + rng.integers(0, 100, half)])
    frame = _flat(rng.permutation(values), shape)

    def claim(stats, kept):
        k, n = kept[0], stats[0][0]
        a, b = k[n // 2 - 1], k[n // 2]
        return n == 2 * half and a < 100 and b - a > gap and stats[0][1] == F(0.5) * (a + b)

    return frame, [whole(frame)], depth_range, 1.0, claim


def rank_bucket_255(counts=(1, 1, 3), shape=None):
    """Odd count of raw 0xFF00, 0xFFFE and 0xFFFF, most of them 0xFFFF: every pass of the median's select ends in
    bucket 255 and the median is the highest raw value."""
    values = np.repeat([0xFF00, 0xFFFE, 0xFFFF], counts)
    frame = _flat(np.random.default_rng(255).permutation(values), shape)

    def claim(stats, kept):
        n, med = stats[0][:2]
        return (n == sum(counts) and n % 2 == 1 and counts[2] > n // 2 and med == 0xFFFF and kept[0][-1] == 0xFFFF
                and kept[0][n // 2] == 0xFFFF and kept[0][0] == 0xFF00)

    return frame, [whole(frame)], FULL_RANGE, 1.0, claim


def rank_bucket_255_then_next():
    """Two kept values 0x00FF and 0xFFFF: the lower is in bucket 255 of the last pass, the upper (rank + 1, found by
    the extra pass) is the highest raw value."""
    def claim(stats, kept):
        n, med, mad = stats[0][:3]
        return n == 2 and list(kept[0]) == [0x00FF, 0xFFFF] and med == 32895 and mad == 32640

    return _rank_scene([0x00FF, 0xFFFF], FULL_RANGE, 1.0, claim)


def rank_nbins(nbins):
    """Intervals of 1, 2 and 3 (odd) raw values from raw 7 up, with rejected values on both sides."""
    values = {1: [0, 6, 7, 7, 8, 7, 7, 10, 65535], 2: [6, 7, 7, 8, 8, 9, 0], 3: [7, 8, 9, 9, 9, 6, 10, 65535]}[nbins]
    expect = {1: (4, 7, 0, 7, 7), 2: (4, 7.5, 0.5, 7, 8), 3: (5, 9, 0, 9, 9)}[nbins]

    def claim(stats, kept):
        return tuple(float(v) for v in stats[0]) == tuple(float(v) for v in expect)

    return _rank_scene(values, (7.0, 6.0 + nbins), 1.0, claim)


def rank_mad_tie(values, inside):
    """A MAD whose key is shared by bins on both sides of the median.  inside: ranks r and r + 1 of the deviations
    both lie in the tie; else the tie ends at r and r + 1 is the next key."""
    def claim(stats, kept):
        n, med, mad = stats[0][:3]
        k = kept[0]
        d = _deviations(k, med)
        r = n // 2 - 1 if n % 2 == 0 else n // 2
        both_sides = bool(((k < med) & (med - k == d[r])).any()) and bool(((k > med) & (k - med == d[r])).any())
        if n % 2:
            return both_sides and d[r - 1] == d[r] and mad == d[r]
        return both_sides and d[r - 1] == d[r] and (d[r + 1] == d[r]) == inside and mad == F(0.5) * (d[r] + d[r + 1])

    return _rank_scene(values, (0.0, 200.0), 1.0, claim)


def rank_mad_zero_even():
    def claim(stats, kept):
        n, med, mad, mn, mx = stats[0]
        return n == 6 and med == 5 and mad == 0 and mn == 5 and mx == 5 and kept[0][0] == 1 and kept[0][-1] == 9

    return _rank_scene([1, 5, 5, 5, 5, 9], (0.0, 100.0), 1.0, claim)


def rank_median_not_kept():
    def claim(stats, kept):
        n, med = stats[0][:2]
        return n == 4 and med == 1.75 and not bool((kept[0] == med).any())

    return _rank_scene([1, 2, 5, 9], (0.0, 100.0), 0.5, claim)


# ---------------------------------------------------------------- band edges
def band(lower, upper, factor):
    """Raw values 100 - lower, 98, 100, 102, 100 + upper (lower, upper >= 3): median raw 100, MAD raw 2, so the band
    ends exactly on raw 97 and raw 103.  An offset of 3 puts a kept value on the limit, 4 one bin outside."""
    m = 100
    values = [m - lower, m - 2, m, m + 2, m + upper]

    def claim(stats, kept):
        n, med, mad, mn, mx = stats[0]
        k = kept[0]
        lo = float(med) - 1.5 * float(mad)
        hi = float(med) + 1.5 * float(mad)
        if not (n == 5 and med == F(m) * F(factor) and mad == F(2) * F(factor)):
            return False
        f = float(F(factor))
        ok_lo = {3: float(k[0]) == lo and mn == k[0], 4: float(k[0]) == lo - f and mn == k[1],
                 5: float(k[0]) == lo - 2 * f and mn == k[1]}[lower]
        ok_hi = {3: float(k[-1]) == hi and mx == k[-1], 4: float(k[-1]) == hi + f and mx == k[-2],
                 5: float(k[-1]) == hi + 2 * f and mx == k[-2]}[upper]
        return ok_lo and ok_hi

    return _rank_scene(values, (0.0, 200.0 * factor), factor, claim, seed=lower * 8 + upper)


# ---------------------------------------------------------------- device-resident views
def view(kind):
    """A non-contiguous view of a larger frame; the GPU test uploads root_of(frame) and describes the view by
    pointer, shape and strides.  Boxes cover the whole view (several chunks), inner parts and clipped parts."""
    base = np.random.default_rng(11).integers(0, 20000, (200, 300)).astype(np.uint16)
    frame = {"step": lambda: base[::2, ::3], "fortran": lambda: np.asfortranarray(base)[3:190, 5:280],
             "neg_rows": lambda: base[::-1, :], "neg_cols": lambda: base[:, ::-1],
             "neg_both": lambda: np.asfortranarray(base)[::-1, ::-2]}[kind]()
    h, w = frame.shape
    boxes = [whole(frame), (3, 4, w // 2, h // 2), (-4, -4, 20, 30), (w - 10, h - 10, 50, 50), (w, 0, 3, 3), (7, 9, 0, 0)]

    def claim(stats, kept):
        root = root_of(frame)
        rs, cs = (s // 2 for s in frame.strides)
        first = (frame.__array_interface__["data"][0] - root.__array_interface__["data"][0]) // 2
        ends = [first + a * (h - 1) * rs + b * (w - 1) * cs for a in (0, 1) for b in (0, 1)]
        shaped = {"step": rs == 600 and cs == 3, "fortran": rs == 1 and cs == 200 and first > 0,
                  "neg_rows": rs == -300 and cs == 1 and first == 199 * 300,
                  "neg_cols": rs == 300 and cs == -1 and first == 299,
                  "neg_both": rs == -1 and cs == -400 and first == 199 + 299 * 200}[kind]
        return (shaped and min(ends) >= 0 and max(ends) < root.size and not frame.flags.c_contiguous
                and not frame.flags.f_contiguous and chunks_of(frame, boxes[0], 8192) >= 2
                and stats[4][0] == 0 and all(s[0] > 1 for s in stats[:4]))

    return frame, boxes, RANGE_OF_CHUNK[8192], 1.0, claim


# ---------------------------------------------------------------- one context, shrinking and growing
def shrink_grow():
    """boxes[:2]: a 3-chunk and a 2-chunk box over every raw value; boxes[2]: one pixel.  The test runs the first two,
    then the last, then the first two again on one context."""
    frame = np.random.default_rng(12).integers(0, 65536, (257, 256)).astype(np.uint16)
    boxes = [whole(frame), (0, 0, 255, 199), (17, 23, 0, 0)]

    def claim(stats, kept):
        return ([chunks_of(frame, b, 32768) for b in boxes] == [3, 2, 1] and stats[0][0] == 65792
                and stats[1][0] == 51200 and stats[2][0] == 1 and kept[0][-1] - kept[0][0] > 65000)

    return frame, boxes, FULL_RANGE, 1.0, claim


# ---------------------------------------------------------------- the registry
Scene = namedtuple("Scene", "build nbins chunk")
SCENES: dict[str, Scene] = {}


def _add(name, nbins, build):
    SCENES[name] = Scene(build, nbins, chunk_of(nbins))


for _c in (8192, 32768):
    _nb = NBINS_OF_CHUNK[_c]
    _add(f"counter_even_{_c}", _nb, lambda c=_c: counter_single(c, 1000))
    _add(f"counter_odd_{_c}", _nb, lambda c=_c: counter_single(c, 1001))
    _add(f"counter_last_bin_{_c}", _nb, lambda c=_c, v=_nb - 1: counter_single(c, v))
    _add(f"counter_split_{_c}", _nb, lambda c=_c: counter_split(c))
    _add(f"counter_multi_even_{_c}", _nb, lambda c=_c: counter_multi(c, 1000))
    _add(f"counter_multi_odd_{_c}", _nb, lambda c=_c: counter_multi(c, 1001))
    for _n in (_c - 1, _c, _c + 1, 2 * _c, 2 * _c + 1):
        _add(f"chunk_random_{_c}_{_n}", _nb, lambda c=_c, n=_n: chunk_random(c, n))
    _add(f"chunk_first_empty_{_c}", _nb, lambda c=_c: chunk_first_empty(c))
    _add(f"chunk_last_empty_{_c}", _nb, lambda c=_c: chunk_last_empty(c))
    for _k in (0, 1, 2):
        _add(f"chunk_kept{_k}_{_c}", _nb, lambda c=_c, k=_k: chunk_few_kept(c, k))
    _add(f"chunk_interleaved_{_c}", _nb, lambda c=_c: chunk_interleaved(c))

_add("rank_middle_identical", 101, rank_middle_identical)
_add("rank_middle_adjacent", 101, rank_middle_adjacent)
_add("rank_middle_far_256", 4001, lambda: rank_middle_far(256, (0.0, 4000.0)))
_add("rank_middle_far_32768", 65536, lambda: rank_middle_far(32768, FULL_RANGE))
# (the same two over three chunks: every uint16 value is kept, so no padding can spread the small scenes out)
_add("rank_middle_far_32768_chunks", 65536, lambda: rank_middle_far(32768, FULL_RANGE, 32769, (198, 331)))
_add("rank_bucket_255", 65536, rank_bucket_255)
_add("rank_bucket_255_chunks", 65536, lambda: rank_bucket_255((10000, 20000, 35537), SHAPE[65537]))
_add("rank_bucket_255_then_next", 65536, rank_bucket_255_then_next)
for _nb in (1, 2, 3):
    _add(f"rank_nbins_{_nb}", _nb, lambda nb=_nb: rank_nbins(nb))
_add("rank_mad_tie_inside_even", 201, lambda: rank_mad_tie([97, 99, 99, 101, 101, 103], True))
_add("rank_mad_tie_ends_at_rank", 201, lambda: rank_mad_tie([98, 99, 101, 102], False))
_add("rank_mad_tie_odd", 201, lambda: rank_mad_tie([98, 99, 100, 101, 102], True))
_add("rank_mad_zero_even", 101, rank_mad_zero_even)
_add("rank_median_not_kept", 201, rank_median_not_kept)

for _lo, _hi, _f in ((3, 3, 1.0), (3, 3, 0.5), (3, 5, 1.0), (5, 3, 1.0), (4, 5, 1.0), (5, 4, 1.0), (4, 4, 0.5)):
    _tag = {3: "on", 4: "out", 5: "far"}
    _add(f"band_lower_{_tag[_lo]}_upper_{_tag[_hi]}_factor_{_f}", 201, lambda a=_lo, b=_hi, f=_f: band(a, b, f))

for _kind in ("step", "fortran", "neg_rows", "neg_cols", "neg_both"):
    _add(f"view_{_kind}", 16384, lambda k=_kind: view(k))

_add("shrink_grow", 65536, shrink_grow)


def names(prefix):
    return [n for n in SCENES if n.startswith(prefix)]
