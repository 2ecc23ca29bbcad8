"""The clearance of the closed map restated in int64 / fp64 numpy: the contract the device is checked
against bit for bit.  It sits on tests/closed_map_free_np.py's FreeNP (the states) and tests/closed_map_carve_np.py's Walk (the
segments' cells); no operation here is contracted.

The field: one uint16 per cell of the free-space grid's box, [z][y][x], the squared distance in cells between integer cell
coordinates to the nearest obstacle cell, exact up to R * R, BEYOND above; R = (int) ceil(max_distance / voxel).  An OCCUPIED cell
is an obstacle; with unknown_is_obstacle an UNKNOWN cell is one too and the box is wrapped in one layer of obstacles (the nearest
outside cell of an inside cell lies in that layer).  The transform is three windowed minima, out(t) = min over |j| <= R of
g(t + j) + j * j, one per axis: any obstacle within R has all three offsets within R, what lies further out is clamped at the end.
A segment's walk: the ray-cast's (skip rule, set-up, stepping; the start cell and every cell stepped into, the end cell included),
each cell with the free walk's t_in."""
from __future__ import annotations

import numpy as np

import closed_map_carve_np as CN
import closed_map_free_np as FN
import voxel_map_np as VN

BEYOND, OUTSIDE = 0xFFFF, 0xFFFE
SKIPPED, CLEAR, BLOCKED, LEFT_BOX = 0, 1, 2, 3
MAX_RADIUS = 128
DEFAULTS = dict(max_distance=4.0, max_segment=120.0, max_bytes=1 << 30, unknown_is_obstacle=1)
FAR = np.int64(1) << 40


def radius_cells(max_distance, voxel):
    """R, or None when it is outside 1 .. 128"""
    with np.errstate(all="ignore"):
        r = np.ceil(np.float64(max_distance) / np.float64(voxel))
    return int(r) if 1.0 <= r <= float(MAX_RADIUS) else None


def need_d2(radius, voxel, R):
    """the d2 below which a cell blocks a body of `radius`, or None when the call is refused"""
    radius = np.float64(radius)
    if not np.isfinite(radius) or radius < 0.0:
        return None
    with np.errstate(all="ignore"):
        q = radius / np.float64(voxel)
        n = np.ceil(q * q)
    return int(n) if n <= float(R * R + 1) else None


def windowed_min(g, axis, R):
    """out(t) = min over |j| <= R of g(t + j) + j * j along `axis`; positions outside the array do not contribute"""
    n = g.shape[axis]
    out = np.full_like(g, FAR)
    for j in range(-min(R, n - 1), min(R, n - 1) + 1):
        dst = [slice(None)] * g.ndim
        src = [slice(None)] * g.ndim
        dst[axis] = slice(max(0, -j), n - max(0, j))
        src[axis] = slice(max(0, j), n - max(0, -j))
        out[tuple(dst)] = np.minimum(out[tuple(dst)], g[tuple(src)] + j * j)
    return out


def transform(obstacle, R, wrap):
    """the truncated squared distance transform of a boolean array of any rank -> uint16 of the same shape"""
    g = np.where(np.asarray(obstacle, bool), np.int64(0), FAR)
    if wrap:
        g = np.pad(g, 1, constant_values=0)
    for axis in reversed(range(g.ndim)):
        g = windowed_min(g, axis, R)
    if wrap:
        g = g[(slice(1, -1),) * g.ndim]
    return np.where(g <= R * R, g, BEYOND).astype(np.uint16)


class ClearNP:
    """the field over the restated grid G (tests/closed_map_free_np.py's FreeNP, reset and filled)"""

    def __init__(self, G, **cfg):
        assert set(cfg) <= set(DEFAULTS)
        self.G, self.cfg = G, dict(DEFAULTS, **cfg)
        self.d2 = None

    def box_cells(self):
        """the box's cells (nz * ny * nx, 3) in the field's order, x fastest"""
        G = self.G
        n = 4 * G.nb
        lo = 4 * G.blo
        z, y, x = np.meshgrid(lo[2] + np.arange(n[2]), lo[1] + np.arange(n[1]), lo[0] + np.arange(n[0]), indexing="ij")
        return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)

    def build(self, misses=None):
        """False (and nothing changed): a refused build"""
        G = self.G
        R = radius_cells(self.cfg["max_distance"], G.v)
        n = 4 * G.nb
        cells = int(n[0]) * int(n[1]) * int(n[2])
        if R is None or 4 * cells > self.cfg["max_bytes"]:
            return False
        state, _ = G.cell_states(self.box_cells(), misses)
        obstacle = state == FN.OCCUPIED
        if self.cfg["unknown_is_obstacle"]:
            obstacle |= state == FN.UNKNOWN
        self.R, self.lo, self.n = R, 4 * G.blo, n
        self.states = state.reshape(n[2], n[1], n[0])
        self.d2 = transform(obstacle.reshape(n[2], n[1], n[0]), R, bool(self.cfg["unknown_is_obstacle"]))
        return True

    def info(self):
        """the device's info without `launches`"""
        d = self.d2.astype(np.int64)
        fin = d[d != BEYOND]
        return dict(lo_cells=tuple(int(x) for x in self.lo), n_cells=tuple(int(x) for x in self.n), bytes=4 * d.size,
                    obstacle_cells=int((d == 0).sum()), finite_cells=int(len(fin)), sum_d2=int(fin.sum()),
                    max_d2=int(fin.max()) if len(fin) else 0, radius_cells=self.R)

    def value(self, cells):
        """(d2 (m,) int64 as a query reads it, outside the box (m,) bool)"""
        c = np.asarray(cells, np.int64).reshape(-1, 3) - self.lo
        inside = ((c >= 0) & (c < self.n)).all(axis=1)
        c = np.where(inside[:, None], c, 0)
        got = self.d2[c[:, 2], c[:, 1], c[:, 0]].astype(np.int64)
        return np.where(inside, got, 0 if self.cfg["unknown_is_obstacle"] else OUTSIDE), ~inside

    def points(self, pts, pose=None, misses=None):
        """-> (states (n,) uint8, d2 (n,) uint16, distance (n,) float64, counts (4,) int64)"""
        G = self.G
        state, _, counts = G.occupancy(pts, pose, misses)
        P = np.asarray(pts, np.float64).reshape(-1, 3)
        if pose is not None:
            P = CN.transform(pose, P)
        d2 = np.full(len(P), OUTSIDE, np.int64)
        ok = state != FN.INVALID
        with np.errstate(all="ignore"):
            d2[ok] = self.value(np.floor((P[ok] - G.o) / G.v).astype(np.int64))[0]
            dist = G.v * np.sqrt(d2.astype(np.float64))
        dist[d2 == BEYOND] = np.inf
        dist[d2 == OUTSIDE] = np.nan
        return state, d2.astype(np.uint16), dist, counts

    def segments(self, starts, ends, radius, pose=None):
        """-> (status (n,) uint8, min_d2 (n,) uint16, t_block (n,) float64, counts (4,) int64), or None: a refused call"""
        G = self.G
        need = need_d2(radius, G.v, self.R)
        if need is None:
            return None
        wrap = bool(self.cfg["unknown_is_obstacle"])
        S, E = np.asarray(starts, np.float64).reshape(-1, 3), np.asarray(ends, np.float64).reshape(-1, 3)
        if pose is not None:
            S, E = CN.transform(pose, S), CN.transform(pose, E)
        with np.errstate(all="ignore"):
            D = E - S
            L = np.sqrt(CN.dot(D, D))
            s0, s1 = (S - G.o) / G.v, (E - G.o) / G.v
            inside = (np.abs(np.floor(s0)) < VN.LIMIT).all(axis=1) & (np.abs(np.floor(s1)) < VN.LIMIT).all(axis=1)
            ok = np.isfinite(E).all(axis=1) & ~(L > self.cfg["max_segment"]) & ~(L == 0.0) & inside
        take = np.flatnonzero(ok)
        m = len(take)
        status, least, t_block = np.full(m, CLEAR, np.uint8), np.full(m, BEYOND, np.int64), np.full(m, -1.0)
        t_in, alive = np.zeros(m), np.ones(m, bool)

        def visit(rows, cells):
            on = alive[rows]
            rows, cells = rows[on], cells[on]
            d2, outside = self.value(cells)
            left = outside & (not wrap)
            status[rows[left]], t_block[rows[left]] = LEFT_BOX, t_in[rows[left]]
            alive[rows[left]] = False
            rows, d2 = rows[~left], d2[~left]
            least[rows] = np.minimum(least[rows], d2)
            hit = d2 < need
            status[rows[hit]], t_block[rows[hit]] = BLOCKED, t_in[rows[hit]]
            alive[rows[hit]] = False

        W = CN.Walk(s0[take], s1[take])
        for rows, cells in W:
            visit(rows, cells)
            t_in[rows] = W.tmax[rows].min(axis=1)   # (the walk has not stepped yet: the tMax the step is about to take)
        rows = np.flatnonzero(alive)
        visit(rows, W.c[rows])                      # the end cell
        out_s, out_d, out_t = np.full(len(E), SKIPPED, np.uint8), np.full(len(E), OUTSIDE, np.int64), np.full(len(E), -1.0)
        out_s[take], out_d[take], out_t[take] = status, least, t_block
        return out_s, out_d.astype(np.uint16), out_t, np.bincount(out_s, minlength=4).astype(np.int64)

    def columns(self, z_lo, z_hi, min_free=1, misses=None):
        """-> (states (ny, nx) uint8 as FreeNP.columns, d2 (ny, nx) uint16), or None: R out of range"""
        R = radius_cells(self.cfg["max_distance"], self.G.v)
        if R is None:
            return None
        state = self.G.columns(z_lo, z_hi, min_free, misses)
        obstacle = state == FN.OCCUPIED
        if self.cfg["unknown_is_obstacle"]:
            obstacle |= state == FN.UNKNOWN
        return state, transform(obstacle, R, bool(self.cfg["unknown_is_obstacle"]))
