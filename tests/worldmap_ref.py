"""The world map's rule (include/kompass_hip.h kc_worldmap_*) as a literal numpy statement: int64
arithmetic over ALL world cells, no bounding box, the pose quantised with math.cos / math.sin and round to even.
Planes are arrays m[I, J] of shape (W, H); a local grid is g[i, j] of shape (gh, gw), as the mapper hands it out."""
import math

import numpy as np

NEVER = -128
UNEXPLORED, EMPTY, OCCUPIED = -1, 0, 100
FRAC = 16
ONE = 1 << FRAC
MAX_OFFSET = 1 << 36  # 2^20 cells

DEFAULT_MODEL = dict(hit=3, miss=1, e_min=-8, e_max=14, occ_thr=1)
# "the latest observation wins" as the design note gives it.  Not quite: a hit on a cell at -127 lands on 0, which is
# below occ_thr = 1, so a cell seen empty and then occupied stays empty once.  int8 leaves no symmetric choice; with
# e_min = -126 every observation of 0 or 100 decides the class: -126 + 127 = 1 is occupied, 127 - 127 = 0 is not.
LATEST_WINS = dict(hit=127, miss=127, e_min=-127, e_max=127, occ_thr=1)
LATEST_WINS_EXACT = dict(hit=127, miss=127, e_min=-126, e_max=127, occ_thr=1)


def quantise_pose(resolution, origin, x, y, yaw):
    """-> (cq, sq, tx, ty).  All in double; round() is round-half-to-even, as lrint / llrint in the default mode."""
    r = float(np.float32(resolution))
    cq = round(math.cos(yaw) * 65536.0)
    sq = round(math.sin(yaw) * 65536.0)
    tx = round((x - origin[0]) / r * 65536.0)
    ty = round((y - origin[1]) / r * 65536.0)
    if abs(tx) > MAX_OFFSET or abs(ty) > MAX_OFFSET:
        raise IndexError("pose more than 2^20 cells from the origin")
    return cq, sq, tx, ty


def central(gh, gw):
    """The mapper's central cell: round(size / 2) - 1 in integer division."""
    return gh // 2 - 1, gw // 2 - 1


def classify(evidence, occ_thr):
    return np.where(evidence == NEVER, UNEXPLORED, np.where(evidence >= occ_thr, OCCUPIED, EMPTY)).astype(np.int8)


class WorldMapRef:
    def __init__(self, width, height, resolution, origin=(0.0, 0.0), **model):
        self.W, self.H = int(width), int(height)
        self.resolution = float(np.float32(resolution))
        self.origin = (float(origin[0]), float(origin[1]))
        self.model = dict(DEFAULT_MODEL)
        self.model.update(model)
        self.clear()

    def clear(self):
        self.evidence = np.full((self.W, self.H), NEVER, np.int8)
        self.cls = np.full((self.W, self.H), UNEXPLORED, np.int8)

    def set_model(self, **model):
        self.model = dict(DEFAULT_MODEL)
        self.model.update(model)
        self.clear()

    def set_prior(self, grid):
        g = np.asarray(grid)
        assert g.shape == (self.W, self.H)
        m = self.model
        e = np.full((self.W, self.H), NEVER, np.int64)
        e[g == OCCUPIED] = m["e_max"]
        e[g == EMPTY] = m["e_min"]
        self.evidence = e.astype(np.int8)
        self.cls = classify(self.evidence, m["occ_thr"])

    def observe(self, local, qpose, c=None):
        """-> (obs int64 [W, H], seen bool [W, H]): the local cell every world cell falls into."""
        local = np.asarray(local)
        gh, gw = local.shape
        c0, c1 = central(gh, gw) if c is None else c
        cq, sq, tx, ty = (int(v) for v in qpose)
        I = np.arange(self.W, dtype=np.int64)[:, None]
        J = np.arange(self.H, dtype=np.int64)[None, :]
        dx = (I << FRAC) - tx
        dy = (J << FRAC) - ty
        a = (cq * dx + sq * dy + (1 << 31)) >> 32   # numpy's >> on int64 is arithmetic: floor
        b = (-sq * dx + cq * dy + (1 << 31)) >> 32
        i = c0 + a
        j = c1 + b
        seen = (i >= 0) & (i < gh) & (j >= 0) & (j < gw)
        obs = np.full((self.W, self.H), -1, np.int64)
        obs[seen] = local[i[seen], j[seen]]
        return obs, seen

    def update(self, local, pose, c=None):
        """pose: (x, y, yaw), or the quantised (cq, sq, tx, ty).  -> (changed, (i_min, j_min, i_max, j_max))."""
        q = pose if len(pose) == 4 else quantise_pose(self.resolution, self.origin, *pose)
        obs, seen = self.observe(local, q, c)
        m = self.model
        e = self.evidence.astype(np.int64)
        base = np.where(e == NEVER, 0, e)
        hit = seen & (obs == OCCUPIED)
        miss = seen & (obs == EMPTY)
        e = np.where(hit, np.minimum(base + m["hit"], m["e_max"]), e)
        e = np.where(miss, np.maximum(base - m["miss"], m["e_min"]), e)
        self.evidence = e.astype(np.int8)
        cls = classify(self.evidence, m["occ_thr"])
        diff = cls != self.cls
        self.cls = cls
        n = int(diff.sum())
        if n == 0:
            return 0, (-1, -1, -1, -1)
        ii, jj = np.nonzero(diff)
        return n, (int(ii.min()), int(jj.min()), int(ii.max()), int(jj.max()))
