"""The carve of the closed map restated in int64 / fp64 numpy: the contract the device is checked against
bit for bit.  No operation here is contracted, and every expression is written in the order tl_carve.hip's header states.

Input: a built closed map (tests/voxel_map_np.py's VoxelMapNP: voxel v, origin o, rows key, N, Q), the K poses it was built
with and the keyframes' clouds ([four source clouds, four target clouds] per keyframe, the convention of
tests/test_gpu_closed_map.py).  Rays: the points of the clouds `mask` selects (bit side * 4 + kind), keyframes ascending, slots
ascending, points in stored order.  Per ray of keyframe k with stored point p:
    O = the translation of P_k,  E = map_transform_point(P_k, p),  D = E - O,  DD = (Dx*Dx + Dy*Dy) + Dz*Dz,  L = sqrt(DD)
skipped when E is not finite, L > max_range, L == 0, or the cell of O or E has |i| >= 2^20 on an axis.
The walk, per axis: s0 = (O - o) / v, s1 = (E - o) / v, c = floor(s0), ce = floor(s1), d = s1 - s0, step = sign(d),
    tMax = ((c + 1) - s0) / d  (d > 0),  (c - s0) / d  (d < 0),  +inf  (d == 0 or c == ce);  tDelta = step / d
n = sum |ce - c| steps: before each the current cell is visited, the step takes the axis of the smallest tMax (ties: the lowest
axis), c += step, tMax = +inf once c == ce, else tMax + tDelta.  So the start cell and the first n - 1 cells stepped into are
visited, the end cell never.
The miss test of a visited cell that is a voxel with centroid C: u = C - O, tt = ((ux*Dx + uy*Dy) + uz*Dz) / DD, w = u - tt * D;
a miss when 0 <= tt, tt < 1 - end_margin / L and (wx*wx + wy*wy) + wz*wz <= radius * radius.  Each miss adds 1 to the voxel's M."""
from __future__ import annotations

import numpy as np

import voxel_map_np as VN

DEFAULTS = dict(max_range=60.0, end_margin=1.0, radius=0.25)
READ_DEFAULTS = dict(min_count=1, min_miss=3, miss_ratio=1.0)


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def transform(P, pts):
    """map_transform_point: rows accumulated left to right, then the division by the fourth"""
    P = np.asarray(P, np.float64)
    x = np.asarray(pts, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        r = [((P[a, 0] * x[:, 0] + P[a, 1] * x[:, 1]) + P[a, 2] * x[:, 2]) + P[a, 3] * 1.0 for a in range(4)]
        return np.stack([r[0] / r[3], r[1] / r[3], r[2] / r[3]], axis=1)


def concatenation(clouds, mask):
    parts = [np.asarray(clouds[j // 4][j % 4], np.float64).reshape(-1, 3) for j in range(8) if (mask >> j) & 1]
    return np.concatenate(parts) if parts else np.zeros((0, 3))


def build_map(poses, clouds, mask=0xF0, voxel=1.0, origin=(0.0, 0.0, 0.0)):
    """the closed map of section 19: each adding keyframe's transformed concatenation, keyframes ascending"""
    V = VN.VoxelMapNP(voxel, origin)
    for P, c in zip(poses, clouds):
        cat = concatenation(c, mask)
        if len(cat):
            V.add_frame(transform(P, cat))
    return V


def rays(poses, clouds, mask):
    """(O (n, 3), E (n, 3)) of every ray in the contract's order"""
    Os, Es = [np.zeros((0, 3))], [np.zeros((0, 3))]
    for P, c in zip(poses, clouds):
        cat = concatenation(c, mask)
        P = np.asarray(P, np.float64)
        Es.append(transform(P, cat))
        Os.append(np.broadcast_to(P[:3, 3], (len(cat), 3)))
    return np.concatenate(Os), np.concatenate(Es)


class Walk:
    """The walk of every ray at once, from grid coordinates s0 to s1 ((m, 3), cells within the grid).  Iterating yields, per
    step index, (rows still walking, their current cells (k, 3) int64) before the step is taken; afterwards `c` holds the cells
    the walks ended in and `n` the steps each took."""

    def __init__(self, s0, s1):
        s0, s1 = np.asarray(s0, np.float64).reshape(-1, 3), np.asarray(s1, np.float64).reshape(-1, 3)
        f = np.floor(s0)
        self.c, self.ce = f.astype(np.int64), np.floor(s1).astype(np.int64)
        d = s1 - s0
        self.step = np.sign(d).astype(np.int64)
        with np.errstate(all="ignore"):
            self.tmax = np.where(d > 0.0, ((f + 1.0) - s0) / d, np.where(d < 0.0, (f - s0) / d, np.inf))
            self.tdelta = self.step / d
        self.tmax[self.c == self.ce] = np.inf
        self.n = np.abs(self.ce - self.c).sum(axis=1)

    def __iter__(self):
        c, ce, tmax = self.c, self.ce, self.tmax
        rows, k = np.flatnonzero(self.n > 0), 0
        while len(rows):
            yield rows, c[rows]
            t = tmax[rows]
            r = np.arange(len(rows))
            a = np.zeros(len(rows), np.int64)
            a[t[:, 1] < t[:, 0]] = 1
            a[t[:, 2] < t[r, a]] = 2
            c[rows, a] += self.step[rows, a]
            tmax[rows, a] = np.where(c[rows, a] == ce[rows, a], np.inf, t[r, a] + self.tdelta[rows, a])
            k += 1
            rows = rows[self.n[rows] > k]


def walk(s0, s1):
    """one ray: (the cells visited in order (n, 3), the cell the n steps end in)"""
    W = Walk(np.reshape(s0, (1, 3)), np.reshape(s1, (1, 3)))
    cells = [c[0] for _, c in W]
    return np.array(cells, np.int64).reshape(-1, 3), W.c[0].copy()


def carve(V, poses, clouds, mask, max_range=60.0, end_margin=1.0, radius=0.25):
    """-> (M (n_voxels,) int64 in id order, the info the device reports without `launches`)"""
    v, o = float(V.voxel), np.asarray(V.origin, np.float64)
    O, E = rays(poses, clouds, mask)
    with np.errstate(all="ignore"):
        D = E - O
        DD = dot(D, D)
        L = np.sqrt(DD)
        s0, s1 = (O - o) / v, (E - o) / v
        inside = (np.abs(np.floor(s0)) < VN.LIMIT).all(axis=1) & (np.abs(np.floor(s1)) < VN.LIMIT).all(axis=1)
        ok = np.isfinite(E).all(axis=1) & ~(L > max_range) & ~(L == 0.0) & inside
        tlim = 1.0 - end_margin / L
    take = np.flatnonzero(ok)
    O, D, DD, tlim = O[take], D[take], DD[take], tlim[take]
    order = np.argsort(V.keys, kind="stable")
    skeys = V.keys[order]
    C = V.centroids()
    r2 = np.float64(radius) * np.float64(radius)
    M = np.zeros(len(V.keys), np.int64)
    steps = tested = 0
    for rows, cells in Walk(s0[take], s1[take]):
        steps += len(rows)
        if not len(skeys):
            continue
        key = VN.pack(cells)
        pos = np.minimum(np.searchsorted(skeys, key), len(skeys) - 1)
        hit = skeys[pos] == key
        rows, ids = rows[hit], order[pos[hit]]
        tested += len(rows)
        u = C[ids] - O[rows]
        tt = dot(u, D[rows]) / DD[rows]
        w = u - tt[:, None] * D[rows]
        miss = (0.0 <= tt) & (tt < tlim[rows]) & (dot(w, w) <= r2)
        np.add.at(M, ids[miss], 1)
    info = dict(n_keyframes=len(poses), n_rays=len(ok), skipped_rays=int(len(ok) - len(take)), steps=int(steps),
                tested=int(tested), misses=int(M.sum()), voxels_missed=int((M > 0).sum()))
    return M, info


def read_carved(V, M, lo=None, hi=None, min_count=1, min_miss=3, miss_ratio=1.0):
    """ids, in id order, of read_box's voxels (lo and hi None: the whole map) that are not left out as seen through"""
    c = V.centroids()
    sel = V.N >= min_count
    if lo is not None:
        sel &= (c >= np.asarray(lo, np.float64)).all(axis=1) & (c <= np.asarray(hi, np.float64)).all(axis=1)
    gone = (M >= min_miss) & (M.astype(np.float64) > np.float64(miss_ratio) * V.N.astype(np.float64))
    return np.flatnonzero(sel & ~gone)
