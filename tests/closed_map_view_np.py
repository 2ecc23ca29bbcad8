"""The view gain of the closed map restated in int64 / fp64 numpy: the contract the device is checked
against bit for bit.  It sits on the frontier field's label array (tests/closed_map_frontier_np.py's FrontierNP.label: the
dense state array of the box) and on tests/closed_map_carve_np.py's Walk, the end cell visited as ClearNP.segments does.

A view is a pose and the shared segment ends in the sensor frame.  Ray r runs from O = pose[:3, 3] to E = transform(pose, p_r);
the skip rule is the carve's under max_range.  Visited are the start cell, then every cell stepped into, the end cell included;
per visited cell the first rule that applies decides: outside the box -- the ray ends (rays_left_box); OCCUPIED -- the ray ends
(rays_occupied); UNKNOWN -- its bit is set in the view's window, unknown_visits + 1, the walk goes on; free or a frontier label
-- free_visits + 1, the walk goes on.  A ray that passes its end cell: rays_ended.  The window: W = int(ceil(max_range / v)) + 1,
S = 2 W + 1, bit ((dz * S) + dy) * S + dx with d = c - c_O + W, c_O = floor((O - o) / v)."""
from __future__ import annotations

import math

import numpy as np

import closed_map_carve_np as CN
import closed_map_frontier_np as QN
import voxel_map_np as VN

DEFAULTS = dict(max_range=20.0, max_bytes=256 << 20, lds_bytes=131072, form=0)
DIAGNOSTICS = ("chunks", "form", "blocks_per_view", "launches", "waits")
GAIN = np.dtype([("unknown_cells", "<i8"), ("unknown_visits", "<i8"), ("free_visits", "<i8"), ("steps", "<i8"),
                 ("rays_skipped", "<i4"), ("rays_occupied", "<i4"), ("rays_left_box", "<i4"), ("rays_ended", "<i4"),
                 ("origin_label", "<u4"), ("reserved0", "<u4"), ("reserved1", "<i8")])
assert GAIN.itemsize == 64


def window(max_range, voxel):
    """-> (W, S, words, bytes)"""
    W = int(math.ceil(np.float64(max_range) / np.float64(voxel))) + 1
    S = 2 * W + 1
    words = (S ** 3 + 31) // 32
    return W, S, words, 4 * words


class ViewNP:
    """the view gain over a label array `label` (nz, ny, nx) uint32 whose lowest cell is `lo`, on the grid (o, v)"""

    def __init__(self, label, lo, o, v, max_range=DEFAULTS["max_range"]):
        self.label = np.asarray(label).astype(np.int64)
        self.lo = np.asarray(lo, np.int64)
        self.n = np.array(self.label.shape[::-1], np.int64)
        self.o, self.v = np.asarray(o, np.float64), np.float64(v)
        self.max_range = np.float64(max_range)
        self.W, self.S, self.words, self.bytes = window(max_range, v)

    @classmethod
    def of(cls, N, max_range=DEFAULTS["max_range"]):
        """over a built FrontierNP"""
        return cls(N.label, N.lo, N.G.o, N.G.v, max_range)

    def value(self, cells):
        """the field at absolute cells (k, 3) -> (k,) int64, QN.OUTSIDE outside the box"""
        c = np.asarray(cells, np.int64).reshape(-1, 3) - self.lo
        inside = ((c >= 0) & (c < self.n)).all(axis=1)
        c = np.where(inside[:, None], c, 0)
        return np.where(inside, self.label[c[:, 2], c[:, 1], c[:, 0]], QN.OUTSIDE)

    def view(self, pose, ends):
        """one view -> (record (GAIN scalar as a (1,) array), bits: the distinct window bit indices ascending (m,) int64,
        beyond: visited cells beyond the window, c_O or None)"""
        pose = np.asarray(pose, np.float64)
        P = np.asarray(ends, np.float64).reshape(-1, 3)
        O = pose[:3, 3]
        rec = np.zeros(1, GAIN)
        with np.errstate(all="ignore"):
            E = CN.transform(pose, P)
            D = E - O
            L = np.sqrt(CN.dot(D, D))
            s0 = np.broadcast_to((O - self.o) / self.v, E.shape)
            s1 = (E - self.o) / self.v
            f0 = np.floor(s0[:1])
            origin_ok = bool((np.abs(f0) < VN.LIMIT).all())
            inside = (np.abs(np.floor(s0)) < VN.LIMIT).all(axis=1) & (np.abs(np.floor(s1)) < VN.LIMIT).all(axis=1)
            ok = np.isfinite(E).all(axis=1) & ~(L > self.max_range) & ~(L == 0.0) & inside
        cO = f0[0].astype(np.int64) if origin_ok else None
        rec["origin_label"] = int(self.value(cO)[0]) if origin_ok else QN.OUTSIDE
        rec["rays_skipped"] = int((~ok).sum())
        take = np.flatnonzero(ok)
        bits, count = [], dict(unknown_visits=0, free_visits=0, steps=0, rays_occupied=0, rays_left_box=0, rays_ended=0, beyond=0)
        if len(take):
            Wk = CN.Walk(s0[take], s1[take])
            alive = np.ones(len(take), bool)

            def visit(rows, cells):
                live = alive[rows]
                rows, cells = rows[live], cells[live]
                val = self.value(cells)
                count["steps"] += len(rows)
                out, occ = val == QN.OUTSIDE, val == QN.OCCUPIED
                count["rays_left_box"] += int(out.sum())
                count["rays_occupied"] += int(occ.sum())
                alive[rows[out | occ]] = False
                unk = val == QN.UNKNOWN
                count["unknown_visits"] += int(unk.sum())
                count["free_visits"] += int((~(out | occ | unk)).sum())
                d = cells[unk] - cO + self.W
                within = ((d >= 0) & (d < self.S)).all(axis=1)
                count["beyond"] += int((~within).sum())
                d = d[within]
                bits.append((d[:, 2] * self.S + d[:, 1]) * self.S + d[:, 0])

            for rows, cells in Wk:
                visit(rows, cells)
            visit(np.arange(len(take)), Wk.c)                   # the end cells (of a ray with n = 0: its only cell)
            count["rays_ended"] = int(alive.sum())
        bits = np.unique(np.concatenate(bits)) if bits else np.zeros(0, np.int64)
        for k in ("unknown_visits", "free_visits", "steps", "rays_occupied", "rays_left_box", "rays_ended"):
            rec[k] = count[k]
        rec["unknown_cells"] = len(bits)
        return rec, bits.astype(np.int64), count["beyond"], cO

    def centres(self, bits, cO):
        """the centres o + (c + 0.5) * v of the window bits `bits` of a view whose origin cell is cO"""
        if not len(bits):
            return np.zeros((0, 3), np.float64)
        row, dx = np.divmod(bits, self.S)
        dz, dy = np.divmod(row, self.S)
        c = np.stack([dx, dy, dz], axis=1) - self.W + cO
        return (self.o + (c.astype(np.float64) + 0.5) * self.v).reshape(-1, 3)

    def gain(self, poses, ends):
        """-> (records (v,) GAIN, info dict without the DIAGNOSTICS)"""
        poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
        got = [self.view(P, ends) for P in poses]
        rec = np.concatenate([g[0] for g in got])
        info = dict(views=len(poses), rays=len(np.asarray(ends).reshape(-1, 3)), window_side=self.S, window_bytes=self.bytes,
                    steps=int(rec["steps"].sum()), unknown_visits=int(rec["unknown_visits"].sum()),
                    unknown_cells=int(rec["unknown_cells"].sum()), beyond_window=int(sum(g[2] for g in got)))
        return rec, info

    def cells(self, pose, ends):
        """one view -> (centres (m, 3) ascending in bit index, record (1,))"""
        rec, bits, _, cO = self.view(pose, ends)
        return self.centres(bits, cO), rec


def cells_by_loop(V, pose, ends):
    """the set of UNKNOWN cells one view sees, by a plain Python loop over each ray's cells (CN.walk): small boxes only"""
    pose = np.asarray(pose, np.float64)
    O = pose[:3, 3]
    seen = set()
    for p in np.asarray(ends, np.float64).reshape(-1, 3):
        E = CN.transform(pose, p.reshape(1, 3))[0]
        D = E - O
        L = float(np.sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]))
        if not np.isfinite(E).all() or L > float(V.max_range) or L == 0.0:
            continue
        cells, last = CN.walk((O - V.o) / V.v, (E - V.o) / V.v)
        for c in list(cells) + [last]:
            val = int(V.value(np.reshape(c, (1, 3)))[0])
            if val in (QN.OUTSIDE, QN.OCCUPIED):
                break
            if val == QN.UNKNOWN:
                seen.add(tuple(int(x) for x in c))
    return seen
