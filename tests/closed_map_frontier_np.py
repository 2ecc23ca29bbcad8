"""The frontiers of the closed map restated in int64 / fp64 numpy: the contract the device is checked
against bit for bit.  It sits on tests/closed_map_free_np.py's FreeNP (the grid, its box, the map's counting voxels); the pure
functions below take a dense array of states, so the CPU tests drive them over hand-made arrays.

The field: one uint32 per cell of the grid's box, [z][y][x].  A frontier cell is a FREE cell with at least one of its six face
neighbours inside the box UNKNOWN; the clusters are the 26-connected components of the frontier cells, and a frontier cell holds
its cluster's root, the least linear index (z * ny + y) * nx + x among the cluster's cells; every other cell holds its state's
sentinel.  The labels are computed here by sweeps of 26 shifted-array minima to the fixpoint (closed_map_route_np.relax's form),
which is unique: every cell ends at the minimum over its component."""
from __future__ import annotations

import numpy as np

import closed_map_carve_np as CN
import closed_map_free_np as FN
import closed_map_route_np as RN
import voxel_map_np as VN

FREE, UNKNOWN, OCCUPIED, OUTSIDE, ALL = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC, 0xFFFFFFFF
DEFAULTS = dict(max_bytes=1 << 30, min_cells=8, reach=2, max_rounds=65536, rounds_per_wait=16)
DIAGNOSTICS = ("tile_updates", "rounds", "launches", "waits")
CLUSTER_BYTES = 136                                   # a component's share of the table on the device
CLUSTER = np.dtype([("sum", "<i8", 3), ("lo", "<i4", 3), ("hi", "<i4", 3), ("root", "<u4"), ("cells", "<u4"),
                    ("unknown_faces", "<u4"), ("reserved", "<u4")])
assert CLUSTER.itemsize == 64
FAR = np.int64(1) << 40
STEPS = RN.STEPS
FACES = [(0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0)]   # (dz, dy, dx)

field_bytes = RN.field_bytes                          # 4 bytes a cell, 8 bytes a tile of 32 x 8 x 4: the route's


def unknown_faces(state):
    """state (nz, ny, nx) of FN.* -> (nz, ny, nx) int64: the face neighbours inside the box that are UNKNOWN"""
    nz, ny, nx = state.shape
    u = np.pad(state == FN.UNKNOWN, 1, constant_values=False).astype(np.int64)
    out = np.zeros(state.shape, np.int64)
    for dz, dy, dx in FACES:
        out += u[1 + dz:nz + 1 + dz, 1 + dy:ny + 1 + dy, 1 + dx:nx + 1 + dx]
    return out


def propagate(front):
    """front (nz, ny, nx) bool -> (labels (nz, ny, nx) int64: the least linear index of each frontier cell's 26-connected
    component, FAR elsewhere; sweeps).  The sweeps run over the frontier cells' bounding box: nothing outside it takes part."""
    nz, ny, nx = front.shape
    out = np.full(front.shape, FAR, np.int64)
    if not front.any():
        return out, 0
    zs, ys, xs = np.nonzero(front)
    box = (slice(zs.min(), zs.max() + 1), slice(ys.min(), ys.max() + 1), slice(xs.min(), xs.max() + 1))
    index = np.arange(nz * ny * nx, dtype=np.int64).reshape(nz, ny, nx)[box]
    f = front[box]
    mz, my, mx = f.shape
    c = np.full((mz + 2, my + 2, mx + 2), FAR, np.int64)       # a ring of FAR: nothing outside takes part
    inner = c[1:-1, 1:-1, 1:-1]
    inner[f] = index[f]
    sweeps = 0
    while True:
        sweeps += 1
        best = inner.copy()
        for dz, dy, dx in STEPS:
            np.minimum(best, c[1 + dz:mz + 1 + dz, 1 + dy:my + 1 + dy, 1 + dx:mx + 1 + dx], out=best)
        best[~f] = FAR
        if (best == inner).all():
            break
        inner[...] = best
    out[box] = inner
    return out, sweeps


def solve(state, lo, min_cells):
    """state (nz, ny, nx) of FN.* over the box whose lowest cell is lo -> (field (nz, ny, nx) uint32, records of all components
    ascending in root, kept records, kept_of (per component: its index in the kept list or -1), counts dict)"""
    state = np.asarray(state)
    nz, ny, nx = state.shape
    faces = unknown_faces(state)
    front = (state == FN.FREE) & (faces > 0)
    lab, sweeps = propagate(front)
    field = np.where(state == FN.OCCUPIED, OCCUPIED, np.where(state == FN.FREE, FREE, UNKNOWN)).astype(np.int64)
    field[front] = lab[front]
    z, y, x = np.nonzero(front)                               # ascending in linear index
    L = lab[front]
    roots, inv = np.unique(L, return_inverse=True)
    rec = np.zeros(len(roots), CLUSTER)
    rec["root"] = roots
    rec["cells"] = np.bincount(inv, minlength=len(roots))
    rec["unknown_faces"] = np.bincount(inv, weights=faces[front], minlength=len(roots)).astype(np.int64)
    for a, v in enumerate((x, y, z)):
        s = np.zeros(len(roots), np.int64)
        np.add.at(s, inv, v)
        rec["sum"][:, a] = s
        low, high = np.full(len(roots), np.iinfo(np.int64).max), np.full(len(roots), np.iinfo(np.int64).min)
        np.minimum.at(low, inv, v)
        np.maximum.at(high, inv, v)
        rec["lo"][:, a] = low + int(lo[a])
        rec["hi"][:, a] = high + int(lo[a])
    keep = rec["cells"] >= min_cells
    kept_of = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)
    counts = dict(free_cells=int((state == FN.FREE).sum()), unknown_cells=int((state == FN.UNKNOWN).sum()),
                  occupied_cells=int((state == FN.OCCUPIED).sum()), frontier_cells=int(front.sum()), clusters=int(len(roots)),
                  clusters_kept=int(keep.sum()), cells_kept=int(rec["cells"][keep].astype(np.int64).sum()),
                  largest=int(rec["cells"].max()) if len(rec) else 0, unknown_faces=int(faces[front].sum()), reserved0=0)
    return field.astype(np.uint32), rec, rec[keep], kept_of, counts, sweeps


def centroids(rec, box_lo, o, v):
    """o + (lo_cells + sum / cells + 0.5) * v per axis, in double, in that order; lo_cells the BOX's lowest cell"""
    rec = np.asarray(rec)
    mean = rec["sum"].astype(np.float64) / rec["cells"].astype(np.float64)[:, None]
    return np.asarray(o, np.float64) + ((np.asarray(box_lo, np.int64).astype(np.float64) + mean) + 0.5) * np.float64(v)


def cost_join(field, kept, route, reach, box_lo, o, v):
    """field, route (nz, ny, nx) uint32 over one box, kept: the kept records -> (cost (k,) uint32, approach (k, 3) float64): per
    kept cluster the least key (cost(u) << 32) | linear(u) over its cells c and the cells u of the box with max |u - c| <= reach
    whose route value is a cost; RN.UNREACHED and NaN without one"""
    nz, ny, nx = field.shape
    f = field.astype(np.int64)
    r = route.astype(np.int64)
    k = len(kept)
    key_none = np.iinfo(np.int64).max                          # none (a key is below 2^63: a cost is below 2^31 here, asserted)
    best = np.full(k, key_none, np.int64)
    if k:
        z, y, x = np.nonzero(f < OUTSIDE)
        L = f[z, y, x]
        pos = np.minimum(np.searchsorted(kept["root"].astype(np.int64), L), k - 1)
        mine = kept["root"].astype(np.int64)[pos] == L
        z, y, x, pos = z[mine], y[mine], x[mine], pos[mine]
        for dz in range(-reach, reach + 1):
            for dy in range(-reach, reach + 1):
                for dx in range(-reach, reach + 1):
                    uz, uy, ux = z + dz, y + dy, x + dx
                    ok = (uz >= 0) & (uz < nz) & (uy >= 0) & (uy < ny) & (ux >= 0) & (ux < nx)
                    c = r[np.where(ok, uz, 0), np.where(ok, uy, 0), np.where(ok, ux, 0)]
                    ok &= c < RN.OUTSIDE
                    assert (c[ok] < (1 << 31)).all()
                    key = (c[ok] << 32) | ((uz[ok] * ny + uy[ok]) * nx + ux[ok])
                    np.minimum.at(best, pos[ok], key)
    none = best == key_none
    cost = np.where(none, RN.UNREACHED, best >> 32).astype(np.uint32)
    lin = np.where(none, 0, best & 0xFFFFFFFF)
    row, ux = np.divmod(lin, nx)
    uz, uy = np.divmod(row, ny)
    cells = np.stack([ux, uy, uz], axis=1) + np.asarray(box_lo, np.int64)
    approach = np.asarray(o, np.float64) + (cells.astype(np.float64) + 0.5) * np.float64(v)
    approach[none] = np.nan
    return cost, approach.reshape(-1, 3)


class FrontierNP:
    """the frontiers over the restated grid G (tests/closed_map_free_np.py's FreeNP, reset and filled)"""

    def __init__(self, G, **cfg):
        assert set(cfg) <= set(DEFAULTS)
        self.G, self.cfg = G, dict(DEFAULTS, **cfg)
        self.label = None

    def box_cells(self):
        """the box's cells (nz * ny * nx, 3) in the field's order, x fastest"""
        G = self.G
        n, lo = 4 * G.nb, 4 * G.blo
        z, y, x = np.meshgrid(lo[2] + np.arange(n[2]), lo[1] + np.arange(n[1]), lo[0] + np.arange(n[0]), indexing="ij")
        return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)

    def _run(self, state, lo):
        """-> (field, kept records, kept_of, roots, info without the diagnostics); False: refused; None: the table does not fit"""
        nz, ny, nx = state.shape
        if nx * ny * nz >= OUTSIDE or field_bytes((nx, ny, nz)) > self.cfg["max_bytes"]:
            return False
        field, rec, kept, kept_of, counts, self.sweeps = solve(state, lo, self.cfg["min_cells"])
        if field_bytes((nx, ny, nz)) + CLUSTER_BYTES * len(rec) > self.cfg["max_bytes"]:
            return None
        info = dict(lo_cells=tuple(int(v) for v in lo), n_cells=(nx, ny, nz), bytes=field_bytes((nx, ny, nz)), **counts)
        return field, kept, kept_of, rec["root"].astype(np.int64), info

    def build(self, misses=None):
        """True; False (and nothing changed): a refused build; None: the cluster table does not fit (the device drops the field)"""
        G = self.G
        n = 4 * G.nb
        state, _ = G.cell_states(self.box_cells(), misses)
        got = self._run(state.reshape(n[2], n[1], n[0]), 4 * G.blo)
        if not got:
            if got is None:
                self.label = None
            return got
        self.lo, self.n = 4 * G.blo, n
        self.label, self.kept, self.kept_of, self.roots, self._info = got
        return True

    def info(self):
        """the device's info without its DIAGNOSTICS"""
        return dict(self._info)

    def clusters(self):
        """-> (kept records, centroids (k, 3))"""
        return self.kept, centroids(self.kept, self.lo, self.G.o, self.G.v)

    def cells(self, root=ALL):
        """-> (centres (m, 3) float64 ascending in linear index, roots (m,) uint32)"""
        f = self.label.astype(np.int64)
        if root == ALL:
            want = np.isin(f, self.kept["root"].astype(np.int64)) & (f < OUTSIDE)
        else:
            want = (f == root) & bool((self.kept["root"] == root).any())
        z, y, x = np.nonzero(want)
        cells = np.stack([x, y, z], axis=1) + self.lo
        return (self.G.o + (cells.astype(np.float64) + 0.5) * self.G.v).reshape(-1, 3), self.label[z, y, x]

    def points(self, pts, pose=None):
        """-> (label (n,) uint32, cluster (n,) int32, counts (5,) int64: frontier, free, unknown, occupied, outside)"""
        G = self.G
        P = np.asarray(pts, np.float64).reshape(-1, 3)
        if pose is not None:
            P = CN.transform(pose, P)
        with np.errstate(all="ignore"):
            fl = np.floor((P - G.o) / G.v)
            ok = np.isfinite(P).all(axis=1) & (np.abs(fl) < VN.LIMIT).all(axis=1)
        c = np.where(ok[:, None], fl, 0).astype(np.int64) - self.lo
        inside = ok & ((c >= 0) & (c < self.n)).all(axis=1)
        c = np.where(inside[:, None], c, 0)
        v = np.where(inside, self.label[c[:, 2], c[:, 1], c[:, 0]].astype(np.int64), OUTSIDE)
        cluster = np.full(len(v), -1, np.int64)
        if len(self.roots):
            pos = np.minimum(np.searchsorted(self.roots, v), len(self.roots) - 1)
            hit = (v < OUTSIDE) & (self.roots[pos] == v)
            cluster[hit] = self.kept_of[pos[hit]]
        kind = np.where(v < OUTSIDE, 0, np.where(v == FREE, 1, np.where(v == UNKNOWN, 2, np.where(v == OCCUPIED, 3, 4))))
        return v.astype(np.uint32), cluster.astype(np.int32), np.bincount(kind, minlength=5).astype(np.int64)

    def costs(self, route):
        """route: the route field (nz, ny, nx) uint32 over the same box -> (cost (k,) uint32, approach (k, 3) float64)"""
        assert route.shape == self.label.shape
        return cost_join(self.label, self.kept, route, self.cfg["reach"], self.lo, self.G.o, self.G.v)

    def columns(self, z_lo, z_hi, min_free=1, misses=None):
        """-> (label (ny, nx) uint32, kept records, info); False: refused; None: the table does not fit"""
        G = self.G
        state = G.columns(z_lo, z_hi, min_free, misses)
        got = self._run(state[None], 4 * G.blo)
        if not got:
            return got
        return got[0][0], got[1], got[4]
