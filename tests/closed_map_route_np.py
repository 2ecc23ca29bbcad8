"""The route through the closed map restated in int64 / fp64 numpy: the contract the device is checked
against bit for bit.  It sits on tests/closed_map_clearance_np.py's ClearNP (the built field d2, its box, R and the grid's origin
and voxel); anything with those attributes will do, so the CPU tests drive it over hand-made arrays.

The field: one uint32 per cell of the clearance field's box, [z][y][x]: the least total weight of a chain of 26-connected moves
between traversable cells (d2 >= max(need, 1)) to an accepted goal's cell, weights 3 / 4 / 5 for a face / edge / vertex step; 0
at a goal, UNREACHED where no goal reaches, BLOCKED where the cell is not traversable.  It is computed here by sweeps of 26
shifted-array minima to the fixpoint, which is unique: any order of relaxation that only lowers and stops when nothing can be
lowered ends there.  The descent: from a cell of cost k > 0 the first neighbour in the order dz, dy, dx (each -1, 0, 1) with
c + w == k."""
from __future__ import annotations

import numpy as np

import closed_map_carve_np as CN
import closed_map_clearance_np as KN
import voxel_map_np as VN

UNREACHED, BLOCKED, OUTSIDE = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD
PATH_OUTSIDE, PATH_REACHED, PATH_UNREACHED, PATH_BLOCKED, PATH_TRUNCATED = 0, 1, 2, 3, 4
TILE = (32, 8, 4)                                    # x, y, z: the device's tile, for `bytes` alone
DEFAULTS = dict(max_bytes=1 << 30, max_rounds=65536, rounds_per_wait=16)
DIAGNOSTICS = ("tile_updates", "rounds", "launches", "waits")
FAR = np.int64(1) << 40
STEPS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]


def weight(step):
    return 2 + sum(1 for s in step if s)


def field_bytes(n):
    """what the device holds for a box of n = (nx, ny, nz) cells: 4 bytes a cell, 8 bytes a tile"""
    tiles = 1
    for a in range(3):
        tiles *= -(-int(n[a]) // TILE[a])
    return 4 * int(n[0]) * int(n[1]) * int(n[2]) + 8 * tiles


def relax(trav, goals):
    """trav (nz, ny, nx) bool, goals (m, 3) local (x, y, z) cells, all traversable -> (the field (nz, ny, nx) uint32, sweeps)"""
    nz, ny, nx = trav.shape
    c = np.full((nz + 2, ny + 2, nx + 2), FAR, np.int64)        # a ring of FAR: nothing outside the box is traversable
    inner = c[1:-1, 1:-1, 1:-1]
    g = np.asarray(goals, np.int64).reshape(-1, 3)
    inner[g[:, 2], g[:, 1], g[:, 0]] = 0
    sweeps = 0
    while True:
        sweeps += 1
        best = inner.copy()
        for dz, dy, dx in STEPS:
            np.minimum(best, c[1 + dz:nz + 1 + dz, 1 + dy:ny + 1 + dy, 1 + dx:nx + 1 + dx] + weight((dz, dy, dx)), out=best)
        best[~trav] = FAR
        if (best == inner).all():
            break
        inner[...] = best
    out = np.where(trav, np.where(inner < FAR, inner, UNREACHED), BLOCKED)
    return out.astype(np.uint32), sweeps


def descend(field, start, max_cells):
    """the cells (local x, y, z) of the path from `start`, at most max_cells of them -> (cells, reached)"""
    nz, ny, nx = field.shape
    x, y, z = (int(v) for v in start)
    k = int(field[z, y, x])
    cells = []
    while len(cells) < max_cells:
        cells.append((x, y, z))
        if k == 0:
            return cells, True
        for dz, dy, dx in STEPS:
            ux, uy, uz = x + dx, y + dy, z + dz
            if 0 <= ux < nx and 0 <= uy < ny and 0 <= uz < nz:
                c = int(field[uz, uy, ux])
                if c < OUTSIDE and c + weight((dz, dy, dx)) == k:
                    x, y, z, k = ux, uy, uz, c
                    break
        else:
            return cells, False          # (a damaged field)
    return cells, False


class RouteNP:
    """the route over the restated clearance K (ClearNP, built): K.d2, K.lo, K.n, K.R, K.G.o, K.G.v"""

    def __init__(self, K, **cfg):
        assert set(cfg) <= set(DEFAULTS)
        self.K, self.cfg = K, dict(DEFAULTS, **cfg)
        self.cost = None

    def cells_of(self, pts, pose=None):
        """-> (cells (n, 3) int64, valid (n,) bool): a point that is not finite or beyond the grid's limits is INVALID"""
        G = self.K.G
        P = np.asarray(pts, np.float64).reshape(-1, 3)
        if pose is not None:
            P = CN.transform(pose, P)
        with np.errstate(all="ignore"):
            f = np.floor((P - G.o) / G.v)
            ok = np.isfinite(P).all(axis=1) & (np.abs(f) < VN.LIMIT).all(axis=1)
        return np.where(ok[:, None], f, 0).astype(np.int64), ok

    def _solve(self, d2, lo, R, goals, radius, pose, flat):
        """over the array d2 (nz, ny, nx), truncated at R, whose lowest cell is lo -> (field, info without the diagnostics), or
        None: refused"""
        need = KN.need_d2(radius, self.K.G.v, R)
        nz, ny, nx = d2.shape
        cells = nx * ny * nz
        if need is None or field_bytes((nx, ny, nz)) > self.cfg["max_bytes"] or 5 * cells >= OUTSIDE:
            return None
        trav = d2.astype(np.int64) >= max(need, 1)
        c, ok = self.cells_of(goals, pose)
        if flat:
            c[:, 2] = lo[2]
        c = c - np.asarray(lo, np.int64)
        ok &= ((c >= 0) & (c < np.array([nx, ny, nz]))).all(axis=1)
        c = np.where(ok[:, None], c, 0)
        ok &= trav[c[:, 2], c[:, 1], c[:, 0]]
        field, self.sweeps = relax(trav, c[ok])
        f = field.astype(np.int64)
        reached = f[f < OUTSIDE]
        info = dict(lo_cells=tuple(int(v) for v in lo), n_cells=(nx, ny, nz), bytes=field_bytes((nx, ny, nz)), need=need,
                    goals_accepted=int(ok.sum()), goals_rejected=int((~ok).sum()), traversable_cells=int(trav.sum()),
                    reached_cells=int(len(reached)), sum_cost=int(reached.sum()), max_cost=int(reached.max()) if len(reached) else 0,
                    reserved0=0)
        return field, info

    def build(self, goals, radius=0.0, pose=None):
        """False (and nothing changed): a refused build"""
        got = self._solve(self.K.d2, self.K.lo, self.K.R, goals, radius, pose, False)
        if got is None:
            return False
        self.cost, self._info = got
        return True

    def info(self):
        """the device's info without its DIAGNOSTICS"""
        return dict(self._info)

    def value(self, cells, valid):
        c = np.asarray(cells, np.int64).reshape(-1, 3) - self.K.lo
        inside = valid & ((c >= 0) & (c < self.K.n)).all(axis=1)
        c = np.where(inside[:, None], c, 0)
        return np.where(inside, self.cost[c[:, 2], c[:, 1], c[:, 0]].astype(np.int64), OUTSIDE)

    def points(self, pts, pose=None):
        """-> (cost (n,) uint32, distance (n,) float64, counts (4,) int64: reached, unreached, blocked, outside)"""
        v = self.value(*self.cells_of(pts, pose))
        dist = self.K.G.v * v.astype(np.float64) / 3.0
        dist[v == UNREACHED] = np.inf
        dist[(v == BLOCKED) | (v == OUTSIDE)] = np.nan
        kind = np.where(v < OUTSIDE, 0, np.where(v == UNREACHED, 1, np.where(v == BLOCKED, 2, 3)))
        return v.astype(np.uint32), dist, np.bincount(kind, minlength=4).astype(np.int64)

    def paths(self, starts, max_cells, pose=None):
        """-> (status (n,) uint8, n_cells (n,) int32, cost (n,) uint32, centres (n, max_cells, 3) float64), or None: refused"""
        cells, ok = self.cells_of(starts, pose)
        n = len(cells)
        if n == 0 or max_cells < 1 or n * max_cells * 24 > self.cfg["max_bytes"]:
            return None
        v = self.value(cells, ok)
        status, count = np.zeros(n, np.uint8), np.zeros(n, np.int32)
        centres = np.zeros((n, max_cells, 3), np.float64)
        G = self.K.G
        for i in range(n):
            if v[i] == OUTSIDE:
                status[i] = PATH_OUTSIDE
            elif v[i] == BLOCKED:
                status[i] = PATH_BLOCKED
            elif v[i] == UNREACHED:
                status[i] = PATH_UNREACHED
            else:
                walk, reached = descend(self.cost, cells[i] - self.K.lo, max_cells)
                status[i], count[i] = PATH_REACHED if reached else PATH_TRUNCATED, len(walk)
                centres[i, :len(walk)] = G.o + ((np.array(walk, np.int64) + self.K.lo).astype(np.float64) + 0.5) * G.v
        return status, count, v.astype(np.uint32), centres

    def columns(self, z_lo, z_hi, goals, radius=0.0, min_free=1, pose=None, misses=None):
        """-> (states (ny, nx) uint8, d2 (ny, nx) uint16, cost (ny, nx) uint32, info), or None: refused"""
        got = self.K.columns(z_lo, z_hi, min_free, misses)
        if got is None:
            return None
        state, d2 = got
        G = self.K.G
        lo = (4 * int(G.blo[0]), 4 * int(G.blo[1]), 0)
        solved = self._solve(d2[None], lo, KN.radius_cells(self.K.cfg["max_distance"], G.v), goals, radius, pose, True)
        if solved is None:
            return None
        return state, d2, solved[0][0], solved[1]
