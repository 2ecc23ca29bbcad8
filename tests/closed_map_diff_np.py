"""A scan diffed against the closed map restated in int64 / fp64 numpy: the contract tl_diff.hip is checked
against bit for bit.  No operation here is contracted.  The association is tests/closed_map_localise_np.py's (associate, over
the localiser's Target) and the ray walk tests/closed_map_carve_np.py's (Walk); neither is copied.

Input: the restated closed map V (tests/voxel_map_np.py), the localiser's view of it T (closed_map_localise_np.Target: per
voxel the record {c, n, eligible} under the current localise configuration), the carve's misses when the gate is on, a scan
(n, 3) in the sensor frame, a pose matrix M (4 x 4, used as it stands) and a config (DEFAULTS).
O = M[:3, 3], E = map_transform_point(M, p).
Point side.  INVALID: E is not finite or its cell has |i| >= 2^20 on an axis.  Otherwise, over the 27 cells in the localiser's
order, a voxel counts unless carve_gate is set and Mv >= min_miss and (double) Mv > miss_ratio * (double) N; the nearest eligible
voxel that counts and the nearest voxel that counts, each under a strict <.  SURFACE: an eligible voxel was found and
fabs(r) <= plane_tol, r = (n_x*d_x + n_y*d_y) + n_z*d_z; OCCUPIED: not SURFACE and the nearest voxel has D <= near * near; NEW:
every other valid point.  ids: the voxel that explained the point, -1 for INVALID and NEW.  hits: a valid point whose own cell is
a voxel adds 1 to it, ungated.
Map side.  The rays are the scan's points in order from O to E; skip rule, walk and miss test are closed_map_carve_np's with
this config's max_range, end_margin and radius; a miss adds 1 to the voxel's through."""
from __future__ import annotations

import copy

import numpy as np

import closed_map_carve_np as CN
import closed_map_localise_np as LN
import voxel_map_np as VN

DEFAULTS = dict(max_range=60.0, end_margin=1.0, radius=0.25, plane_tol=0.1, near=0.5, min_miss=3, miss_ratio=1.0, carve_gate=0)
GONE_DEFAULTS = dict(min_through=3, gone_ratio=1.0)
INVALID, SURFACE, OCCUPIED, NEW = 0, 1, 2, 3


def counting(V, cfg, misses):
    """the voxels that explain points: all of them, or with the gate on those the carved read keeps"""
    if not cfg["carve_gate"]:
        return np.ones(len(V.keys), bool)
    Mv = np.asarray(misses, np.int64)
    return ~((Mv >= cfg["min_miss"]) & (Mv.astype(np.float64) > np.float64(cfg["miss_ratio"]) * V.N.astype(np.float64)))


def with_candidates(T, mask):
    """T with `mask` as what LN.associate takes for its candidates"""
    view = copy.copy(T)
    view.eligible = np.asarray(mask, bool)
    return view


def labels_of(T, V, E, cfg, misses=None):
    """-> (labels (n,) uint8, ids (n,) int32, valid (n,) bool, own (n,) int64: the voxel of the point's own cell or -1)"""
    E = np.asarray(E, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        f = np.floor((E - T.origin) / T.voxel)
        valid = np.isfinite(E).all(axis=1) & (np.abs(f) < VN.LIMIT).all(axis=1)
    counts = counting(V, cfg, misses)
    ide, de = LN.associate(with_candidates(T, T.eligible & counts), E)
    ida, da = LN.associate(with_candidates(T, counts), E)
    ne = np.zeros((len(E), 3))
    ne[ide >= 0] = T.n[ide[ide >= 0]]
    r = (ne[:, 0] * de[:, 0] + ne[:, 1] * de[:, 1]) + ne[:, 2] * de[:, 2]
    Da = (da[:, 0] * da[:, 0] + da[:, 1] * da[:, 1]) + da[:, 2] * da[:, 2]
    surface = valid & (ide >= 0) & (np.fabs(r) <= np.float64(cfg["plane_tol"]))
    occupied = valid & ~surface & (ida >= 0) & (Da <= np.float64(cfg["near"]) * np.float64(cfg["near"]))
    labels = np.full(len(E), NEW, np.uint8)
    labels[~valid] = INVALID
    labels[surface] = SURFACE
    labels[occupied] = OCCUPIED
    ids = np.full(len(E), -1, np.int32)
    ids[surface] = ide[surface]
    ids[occupied] = ida[occupied]
    own = np.full(len(E), -1, np.int64)
    rows = np.flatnonzero(valid)
    if len(rows):
        own[rows] = T.find(f[rows].astype(np.int64))
    return labels, ids, valid, own


def through_of(V, O, E, cfg):
    """-> (through (n_voxels,) int64 of these rays, skipped, steps, tested)"""
    v, o = float(V.voxel), np.asarray(V.origin, np.float64)
    E = np.asarray(E, np.float64).reshape(-1, 3)
    O = np.broadcast_to(np.asarray(O, np.float64), E.shape)
    with np.errstate(all="ignore"):
        D = E - O
        DD = CN.dot(D, D)
        L = np.sqrt(DD)
        s0, s1 = (O - o) / v, (E - o) / v
        inside = (np.abs(np.floor(s0)) < VN.LIMIT).all(axis=1) & (np.abs(np.floor(s1)) < VN.LIMIT).all(axis=1)
        ok = np.isfinite(E).all(axis=1) & ~(L > cfg["max_range"]) & ~(L == 0.0) & inside
        tlim = 1.0 - cfg["end_margin"] / L
    take = np.flatnonzero(ok)
    O, D, DD, tlim = O[take], D[take], DD[take], tlim[take]
    order = np.argsort(V.keys, kind="stable")
    skeys = V.keys[order]
    C = V.centroids()
    r2 = np.float64(cfg["radius"]) * np.float64(cfg["radius"])
    through = np.zeros(len(V.keys), np.int64)
    steps = tested = 0
    for rows, cells in CN.Walk(s0[take], s1[take]):
        steps += len(rows)
        if not len(skeys):
            continue
        key = VN.pack(cells)
        pos = np.minimum(np.searchsorted(skeys, key), len(skeys) - 1)
        hit = skeys[pos] == key
        rows, ids = rows[hit], order[pos[hit]]
        tested += len(rows)
        u = C[ids] - O[rows]
        tt = CN.dot(u, D[rows]) / DD[rows]
        w = u - tt[:, None] * D[rows]
        miss = (0.0 <= tt) & (tt < tlim[rows]) & (CN.dot(w, w) <= r2)
        np.add.at(through, ids[miss], 1)
    return through, int(len(ok) - len(take)), int(steps), int(tested)


def diff(T, V, points, M, cfg=None, misses=None, state=None):
    """One call.  state: None (the counts are cleared first) or the dict a previous call returned (TLOAM_DIFF_ACCUMULATE).
    -> dict(labels, ids, through, hits, info); info holds what the device reports without launches, prepared and cleared"""
    cfg = dict(DEFAULTS, **(cfg or {}))
    M = np.asarray(M, np.float64).reshape(4, 4)
    E = CN.transform(M, points)
    labels, ids, valid, own = labels_of(T, V, E, cfg, misses)
    hits = np.zeros(len(V.keys), np.int64)
    np.add.at(hits, own[own >= 0], 1)
    through, skipped, steps, tested = through_of(V, M[:3, 3], E, cfg)
    scans = 1
    if state is not None:
        through, hits, scans = through + state["through"], hits + state["hits"], state["info"]["scans"] + 1
    info = dict(n_points=len(E), n_invalid=int((labels == INVALID).sum()), n_surface=int((labels == SURFACE).sum()),
                n_occupied=int((labels == OCCUPIED).sum()), n_new=int((labels == NEW).sum()), rays=len(E), skipped_rays=skipped,
                steps=steps, tested=tested, through=int(through.sum()), voxels_through=int((through > 0).sum()),
                voxels_hit=int((hits > 0).sum()), scans=scans)
    return dict(labels=labels, ids=ids, through=through, hits=hits, info=info)


def read_gone(V, through, hits, lo=None, hi=None, min_through=3, gone_ratio=1.0):
    """ids, in id order, of the voxels (lo and hi None: of the whole map) with through >= min_through and
    (double) through > gone_ratio * (double) hits"""
    sel = np.ones(len(V.keys), bool)
    if lo is not None:
        c = V.centroids()
        sel &= (c >= np.asarray(lo, np.float64)).all(axis=1) & (c <= np.asarray(hi, np.float64)).all(axis=1)
    gone = (through >= min_through) & (through.astype(np.float64) > np.float64(gone_ratio) * hits.astype(np.float64))
    return np.flatnonzero(sel & gone)
