"""The free space of the closed map restated in int64 / fp64 numpy: the contract the device is checked
against bit for bit.  No operation here is contracted; the rays and their walk are tests/closed_map_carve_np.py's (rays, Walk).

The grid: bricks of 4 x 4 x 4 cells of the map's grid, one uint64 a brick, bit ((cz & 3) << 4) | ((cy & 3) << 2) | (cx & 3); the
brick of a cell is c >> 2 (flooring); a box of bricks [blo, blo + nb) per axis, brick (bx, by, bz) at word
((bz - blo_z) * nby + (by - blo_y)) * nbx + (bx - blo_x).
The free condition of a ray from O to E (skip rule, set-up and stepping: closed_map_carve_np's): the visited cells are the
carve's, the start cell and the first n - 1 cells stepped into.  t_in of a visited cell is 0 for the start cell, else the tMax of
the axis the step into it took, read before the step -- the row minimum of Walk.tmax at the previous yield.  With
tlim = 1.0 - end_margin / L the cell is marked when t_in < tlim; the walk stops at the first cell that fails.  A marked cell
inside the box sets its bit and counts in cells_marked, one outside counts in cells_outside.
A voxel counts when N >= min_count and not (carve_gate and M >= min_miss and (double) M > miss_ratio * (double) N).  A point or
cell is INVALID (not finite, or |i| >= 2^20), OCCUPIED (a counting voxel), FREE (inside the box, its bit set) or UNKNOWN."""
from __future__ import annotations

import numpy as np

import closed_map_carve_np as CN
import voxel_map_np as VN

INVALID, UNKNOWN, FREE, OCCUPIED = 0, 1, 2, 3
DEFAULTS = dict(max_range=60.0, end_margin=1.0, max_bytes=1 << 30, min_count=1, min_miss=3, miss_ratio=1.0, carve_gate=0)
CELL_MAX = VN.LIMIT - 1


def auto_box(poses, voxel, origin, max_range):
    """(lo (3,), hi (3,)) int64 cells, inclusive: the host's arithmetic, in double, in its order"""
    P = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    if not len(P):
        return np.zeros(3, np.int64), np.zeros(3, np.int64)
    c = np.floor((P[:, :3, 3] - np.asarray(origin, np.float64)) / np.float64(voxel))
    R = np.float64(int(np.ceil(np.float64(max_range) / np.float64(voxel))) + 1)
    lo = np.clip(c.min(axis=0) - R, -float(CELL_MAX), float(CELL_MAX))
    hi = np.clip(c.max(axis=0) + R, -float(CELL_MAX), float(CELL_MAX))
    return lo.astype(np.int64), hi.astype(np.int64)


def marked(O, E, voxel, origin, max_range=60.0, end_margin=1.0):
    """the cells the rays O -> E mark, with multiplicity, in no contractual order -> (cells (m, 3) int64, skipped rays, cells
    visited)"""
    v, o = np.float64(voxel), np.asarray(origin, np.float64)
    O, E = np.asarray(O, np.float64).reshape(-1, 3), np.asarray(E, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        D = E - O
        L = np.sqrt(CN.dot(D, D))
        s0, s1 = (O - o) / v, (E - o) / v
        inside = (np.abs(np.floor(s0)) < VN.LIMIT).all(axis=1) & (np.abs(np.floor(s1)) < VN.LIMIT).all(axis=1)
        ok = np.isfinite(E).all(axis=1) & ~(L > max_range) & ~(L == 0.0) & inside
        tlim = 1.0 - np.float64(end_margin) / L
    take = np.flatnonzero(ok)
    tlim = tlim[take]
    W = CN.Walk(s0[take], s1[take])
    t_in = np.zeros(len(take))
    alive = np.ones(len(take), bool)
    out, visited = [np.zeros((0, 3), np.int64)], 0
    for rows, cells in W:
        visited += len(rows)
        good = alive[rows] & (t_in[rows] < tlim[rows])
        alive[rows] = good
        out.append(cells[good])
        t_in[rows] = W.tmax[rows].min(axis=1)   # (the walk has not stepped yet: the tMax the step is about to take)
    return np.concatenate(out), int(len(ok) - len(take)), int(visited)


def cell_keys(cells):
    """the sorted set of a list of cells, as the map's keys"""
    return np.unique(VN.pack(np.asarray(cells, np.int64).reshape(-1, 3)))


class FreeNP:
    """the grid beside the restated map V (tests/voxel_map_np.py's VoxelMapNP, read when the grid is read)"""

    def __init__(self, V, **cfg):
        assert set(cfg) <= set(DEFAULTS) | {"ray_mask"}
        self.V, self.cfg = V, dict(DEFAULTS, **cfg)
        self.v, self.o = np.float64(V.voxel), np.asarray(V.origin, np.float64)
        self.words = None

    # ---- the box
    def reset(self, lo=None, hi=None, poses=None):
        """lo, hi: the caller's cells; both None: the auto box over `poses`.  False (and nothing changed): a refused box"""
        if lo is None:
            lo, hi = auto_box(poses, self.v, self.o, self.cfg["max_range"])
        lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
        if (lo > hi).any() or (np.abs(lo) >= VN.LIMIT).any() or (np.abs(hi) >= VN.LIMIT).any():
            return False
        blo, nb = lo >> 2, (hi >> 2) - (lo >> 2) + 1
        n_words = int(nb[0]) * int(nb[1]) * int(nb[2])   # (python integers: no overflow)
        if 8 * n_words > self.cfg["max_bytes"]:
            return False
        self.blo, self.nb = blo, nb
        self.words = np.zeros(n_words, np.uint64)
        self.keyframes = self.scans = 0
        self.last = dict(rays=0, skipped_rays=0, cells_marked=0, cells_outside=0)
        self.visited = 0
        return True

    def info(self):
        """the device's info without `launches`"""
        return dict(lo_cells=tuple(int(x) for x in 4 * self.blo), n_bricks=tuple(int(x) for x in self.nb), bytes=8 * len(self.words),
                    keyframes=self.keyframes, scans=self.scans, free_cells=int(self.bits().sum()),
                    bricks_nonzero=int((self.words != 0).sum()), reserved0=0, **self.last)

    def bits(self):
        """(n_words, 64) uint8: bit b of word i"""
        return ((self.words[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)

    def locate(self, cells):
        """(inside the box (m,) bool, word index (m,) int64 -- 0 outside --, bit (m,) int64)"""
        cells = np.asarray(cells, np.int64).reshape(-1, 3)
        b = (cells >> 2) - self.blo
        inside = ((b >= 0) & (b < self.nb)).all(axis=1)
        idx = np.where(inside, (b[:, 2] * self.nb[1] + b[:, 1]) * self.nb[0] + b[:, 0], 0)
        bit = ((cells[:, 2] & 3) << 4) | ((cells[:, 1] & 3) << 2) | (cells[:, 0] & 3)
        return inside, idx, bit

    # ---- the adds
    def add_rays(self, O, E):
        cells, skipped, visited = marked(O, E, self.v, self.o, self.cfg["max_range"], self.cfg["end_margin"])
        inside, idx, bit = self.locate(cells)
        np.bitwise_or.at(self.words, idx[inside], np.uint64(1) << bit[inside].astype(np.uint64))
        self.last = dict(rays=len(np.asarray(E).reshape(-1, 3)), skipped_rays=skipped, cells_marked=int(inside.sum()),
                         cells_outside=int((~inside).sum()))
        self.visited = visited
        self.marked_keys = cell_keys(cells)
        return self.info()

    def add_keyframes(self, poses, clouds, mask):
        """the rays of keyframes [self.keyframes, len(poses)) under `mask`"""
        k = self.keyframes
        O, E = CN.rays(poses[k:], clouds[k:], mask)
        self.keyframes = len(poses)
        return self.add_rays(O, E)

    def add_scan(self, pts, pose):
        pose = np.asarray(pose, np.float64)
        E = CN.transform(pose, pts)
        self.scans += 1
        return self.add_rays(np.broadcast_to(pose[:3, 3], E.shape), E)

    # ---- the reads
    def counting(self, cells, misses=None):
        """the id of the counting voxel of each cell, -1 without one"""
        V, g = self.V, self.cfg
        cells = np.asarray(cells, np.int64).reshape(-1, 3)
        ids = np.full(len(cells), -1, np.int64)
        if not len(V.keys) or not len(cells):
            return ids
        ok = (np.abs(cells) < VN.LIMIT).all(axis=1)
        order = np.argsort(V.keys, kind="stable")
        skeys = V.keys[order]
        key = VN.pack(np.where(ok[:, None], cells, 0))
        pos = np.minimum(np.searchsorted(skeys, key), len(skeys) - 1)
        hit = ok & (skeys[pos] == key)
        ids[hit] = order[pos[hit]]
        N = V.N[ids[hit]]
        counts = N >= g["min_count"]
        if g["carve_gate"]:
            M = np.asarray(misses, np.int64)[ids[hit]]
            counts &= ~((M >= g["min_miss"]) & (M.astype(np.float64) > np.float64(g["miss_ratio"]) * N.astype(np.float64)))
        ids[np.flatnonzero(hit)[~counts]] = -1
        return ids

    def cell_states(self, cells, misses=None):
        """(states (m,) uint8 of cells inside the grid's limits, ids (m,) int32)"""
        ids = self.counting(cells, misses)
        inside, idx, bit = self.locate(cells)
        seen = inside & (((self.words[idx] >> bit.astype(np.uint64)) & np.uint64(1)) != 0)
        state = np.where(ids >= 0, OCCUPIED, np.where(seen, FREE, UNKNOWN)).astype(np.uint8)
        return state, ids.astype(np.int32)

    def occupancy(self, pts, pose=None, misses=None):
        """-> (states (n,) uint8, ids (n,) int32, counts (4,) int64)"""
        P = np.asarray(pts, np.float64).reshape(-1, 3)
        if pose is not None:
            P = CN.transform(pose, P)
        with np.errstate(all="ignore"):
            f = np.floor((P - self.o) / self.v)
            ok = np.isfinite(P).all(axis=1) & (np.abs(f) < VN.LIMIT).all(axis=1)
        state, ids = np.zeros(len(P), np.uint8), np.full(len(P), -1, np.int32)
        state[ok], ids[ok] = self.cell_states(f[ok].astype(np.int64), misses)
        return state, ids, np.bincount(state, minlength=4).astype(np.int64)

    def free_cells(self, lo=None, hi=None, misses=None):
        """the centres (m, 3) of the FREE cells, word index ascending, then bit ascending"""
        word, bit = np.nonzero(self.bits())
        bz, rest = np.divmod(word, int(self.nb[0]) * int(self.nb[1]))
        by, bx = np.divmod(rest, int(self.nb[0]))
        cells = 4 * (np.stack([bx, by, bz], axis=1) + self.blo) + np.stack([bit & 3, (bit >> 2) & 3, bit >> 4], axis=1)
        cells = cells[self.counting(cells, misses) < 0]
        centres = self.o + (cells.astype(np.float64) + 0.5) * self.v
        if lo is not None:
            centres = centres[(centres >= np.asarray(lo, np.float64)).all(axis=1) & (centres <= np.asarray(hi, np.float64)).all(axis=1)]
        return centres

    def band(self, z_lo, z_hi):
        """the band's cells (z0, z1) clipped to the box; z0 > z1: it misses the box"""
        box0, box1 = float(4 * self.blo[2]), float(4 * (self.blo[2] + self.nb[2]) - 1)
        with np.errstate(all="ignore"):
            a, b = np.floor((np.float64(z_lo) - self.o[2]) / self.v), np.floor((np.float64(z_hi) - self.o[2]) / self.v)
        a, b = max(a, box0), min(b, box1)
        return (1, 0) if a > box1 or b < box0 else (int(a), int(b))

    def columns(self, z_lo, z_hi, min_free=1, misses=None):
        """(ny, nx) uint8 over the box's x-y footprint, y outer"""
        z0, z1 = self.band(z_lo, z_hi)
        nx, ny = 4 * int(self.nb[0]), 4 * int(self.nb[1])
        occupied, free = np.zeros((ny, nx), bool), np.zeros((ny, nx), np.int64)
        x, y = np.meshgrid(4 * int(self.blo[0]) + np.arange(nx), 4 * int(self.blo[1]) + np.arange(ny))
        for z in range(z0, z1 + 1):
            state, _ = self.cell_states(np.stack([x.ravel(), y.ravel(), np.full(nx * ny, z)], axis=1), misses)
            occupied |= (state == OCCUPIED).reshape(ny, nx)
            free += (state == FREE).reshape(ny, nx)
        return np.where(occupied, OCCUPIED, np.where(free >= min_free, FREE, UNKNOWN)).astype(np.uint8)
