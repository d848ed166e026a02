"""Restatement, for the tests, of the reference's PCD reader and PCD -> occupancy grid
(src/kompass_cpp/kompass_cpp/include/utils/pointcloud.h:286-437 and :468-540), in numpy float32, expression by
expression.  It imports nothing of the code under test.  The places where this project defines what the
reference leaves wrong or undefined are marked DEVIATION; test_pcd_cpu.py pins `grid` to grids
worked out by hand."""
import re

import numpy as np

MAX_CELLS = 1 << 30  # KC_CLOUD_GRID_MAX_CELLS
_BLANK = b" \t\r\n\f\v"


class PcdError(Exception):
    pass


_NUMBER = re.compile(r"-?(?:(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?|inf(?:inity)?|nan(?:\([A-Za-z0-9_]*\))?)", re.I)


def parse_float(tok: str) -> np.float32:
    """std::from_chars<float> as the reader calls it (the end pointer is ignored, as in the reference): the longest
    prefix of the token that is a number counts ("1.5abc" is 1.5, "1e" is 1); one rounding to float; nan / inf in
    any case with an optional '-'; no leading '+' and no hex.  A token without such a prefix, or whose number is
    outside float's range (it would round to +-inf, or underflows to zero), leaves 0."""
    m = _NUMBER.match(tok)
    if not m:
        return np.float32(0)
    t = m.group(0)
    low = t.lower().lstrip("-")
    if low.startswith(("nan", "inf")):
        return np.float32(("-" if t[0] == "-" else "") + low[:3])
    with np.errstate(all="ignore"):
        v = np.float32(t)  # correctly rounded, straight from the decimal text
    if v == 0 and any(c in "123456789" for c in low.split("e")[0]):
        return np.float32(0)  # underflow is out of range too: +0, not the signed zero of the rounding
    return np.float32(0) if np.isinf(v) else v


def read(path) -> np.ndarray:
    """readPCD (:286-437) -> (N, 3) float32; PcdError where the reader returns nullopt."""
    raw = open(path, "rb").read()
    pos = 0
    fields, sizes, n_points, fmt = [], None, None, None
    while pos < len(raw):  # :304-359
        end = raw.find(b"\n", pos)
        end = len(raw) if end < 0 else end
        line, pos = raw[pos:end], end + 1
        if not line or line[:1] == b"#" or b" " not in line:
            continue
        key, rest = line.split(b" ", 1)
        toks = rest.split()  # DEVIATION: trailing '\r' / blanks and repeated blanks are separators
        if key == b"FIELDS":
            fields = [t.decode() for t in toks]
        elif key == b"SIZE":
            try:
                sizes = [int(t) for t in toks]
            except ValueError:
                raise PcdError("SIZE")
            if any(not (1 <= s <= 8) for s in sizes):
                raise PcdError("SIZE")
        elif key == b"COUNT":
            if any(t != b"1" for t in toks):  # DEVIATION: the reference ignores COUNT and misreads such files
                raise PcdError("COUNT")
        elif key == b"POINTS":
            if len(toks) != 1 or not toks[0].isdigit():
                raise PcdError("POINTS")
            n_points = int(toks[0])
        elif key == b"DATA":
            fmt = toks[0].decode() if toks else ""
            break
    if not all(f in fields for f in "xyz"):
        raise PcdError("x, y, z required")  # :361-365
    if n_points is None:
        raise PcdError("POINTS missing")  # DEVIATION: the reference returns an empty cloud
    if fmt not in ("ascii", "binary"):
        raise PcdError("DATA")  # :430-434
    # the last FIELDS line counts, and of a name that repeats the last position, as in the reference's loop (:315-330)
    ix = [len(fields) - 1 - fields[::-1].index(f) for f in "xyz"]
    if sizes is not None or fmt == "binary":
        if sizes is None or len(sizes) != len(fields):
            raise PcdError("FIELDS / SIZE")  # :370-373
        if any(sizes[i] != 4 for i in ix):
            raise PcdError("x / y / z size")  # DEVIATION: the reference memcpy's 4 bytes whatever SIZE says
    body = raw[pos:]
    if fmt == "ascii":
        toks = body.split()
        # DEVIATION: a point is len(FIELDS) tokens and x / y / z go by field index (the reference takes the first
        # three tokens of a running stream)
        if len(toks) < n_points * len(fields):
            raise PcdError("POINTS larger than the data")  # DEVIATION: the reference leaves zeros
        out = np.zeros((n_points, 3), np.float32)
        for i in range(n_points):
            for k in range(3):
                out[i, k] = parse_float(toks[i * len(fields) + ix[k]].decode("latin-1"))
        return out
    stride = sum(sizes)
    offs = [sum(sizes[:i]) for i in ix]  # :374-382
    if len(body) < n_points * stride:
        raise PcdError("short file")  # :414-418
    out = np.zeros((n_points, 3), np.float32)
    rec = np.frombuffer(body[:n_points * stride], np.uint8).reshape(n_points, stride)
    for k in range(3):
        out[:, k] = np.ascontiguousarray(rec[:, offs[k]:offs[k] + 4]).view("<f4")[:, 0]
    return out


def grid(points, grid_resolution, z_ground_limit, robot_height):
    """readPCDToOccupancyGrid (:468-540) on an (N, 3) cloud -> (int8 grid (cells_x, cells_y), float32 origin[3]).
    IndexError where the C ABI answers KC_ERR_RANGE."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    res, zg, rh = np.float32(grid_resolution), np.float32(z_ground_limit), np.float32(robot_height)
    if not (res > 0 and np.isfinite(res)):
        raise IndexError("grid_resolution")  # DEVIATION: the reference divides by it
    empty = np.empty((0, 0), np.int8), np.zeros(3, np.float32)
    if len(p) == 0:
        return empty  # :482-484
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    ok = np.isfinite(x) & np.isfinite(y)  # DEVIATION: a non-finite x or y takes part in neither pass
    if not ok.any():
        return empty
    with np.errstate(all="ignore"):
        min_x, max_x = x[ok].min(), x[ok].max()  # :486-497
        min_y, max_y = y[ok].min(), y[ok].max()
        fx = np.ceil((max_x - min_x) / res)  # :500-503, float32 throughout
        fy = np.ceil((max_y - min_y) / res)
        if not (fx <= MAX_CELLS and fy <= MAX_CELLS and float(fx) * float(fy) <= MAX_CELLS):
            raise IndexError("grid above the cap")  # DEVIATION: the reference overflows its int
        cells_x, cells_y = int(fx), int(fy)
        inv_res = np.float32(1.0) / res  # :506
        g = np.full((cells_x, cells_y), -1, np.int8)  # :509
        cls = np.where((z > zg) & (z <= rh), 100, np.where(z <= zg, 0, -1)).astype(np.int8)  # :523-532
        cxf = (x - min_x) * inv_res  # :517-518
        cyf = (y - min_y) * inv_res
        # static_cast<int> of a float no int holds (or of NaN) is INT_MIN on x86: outside every grid
        fits = ok & (cxf < 2147483648.0) & (cyf < 2147483648.0)
        cx = np.where(fits, cxf, -1).astype(np.int64)  # truncation toward zero
        cy = np.where(fits, cyf, -1).astype(np.int64)
        inside = fits & (cx >= 0) & (cx < cells_x) & (cy >= 0) & (cy < cells_y)  # :520
        np.maximum.at(g, (cx[inside], cy[inside]), cls[inside])  # :534
    return g, np.array([min_x, min_y, 0.0], np.float32)


def write_pcd(path, fields, sizes, types, columns, binary, newline="\n", comments=(), counts=None, points=None,
              data_tag=None, fmt="%.9g"):
    """A PCD file from per-field numpy columns (test fixture writer; nothing of the reference)."""
    n = len(columns[0]) if columns else 0
    head = ["# .PCD v0.7 - Point Cloud Data file format", *comments, "VERSION 0.7", "FIELDS " + " ".join(fields),
            "SIZE " + " ".join(str(s) for s in sizes), "TYPE " + " ".join(types),
            "COUNT " + " ".join(str(c) for c in (counts or [1] * len(fields))), f"WIDTH {n}", "HEIGHT 1",
            "VIEWPOINT 0 0 0 1 0 0 0", f"POINTS {n if points is None else points}",
            "DATA " + (data_tag or ("binary" if binary else "ascii"))]
    blob = (newline.join(head) + newline).encode()
    if binary:
        rec = np.zeros((n, sum(sizes)), np.uint8)
        o = 0
        for c, s in zip(columns, sizes):
            rec[:, o:o + s] = np.ascontiguousarray(c).view(np.uint8).reshape(n, s)
            o += s
        blob += rec.tobytes()
    else:
        for i in range(n):
            blob += (" ".join(c[i] if isinstance(c[i], str) else fmt % c[i] for c in columns) + newline).encode()
    with open(path, "wb") as f:
        f.write(blob)
