"""The ray-cast of the closed map restated in int64 / fp64 numpy: the contract tl_raycast.hip is checked
against bit for bit.  No operation here is contracted, and every expression is written in the order tl_raycast.hip's header
states.  The walk is tests/closed_map_carve_np.py's (Walk), the voxel records tests/closed_map_localise_np.py's (Target) and the
transform CN.transform; none of them is copied.

Input: the restated closed map V (tests/voxel_map_np.py), the localiser's view of it T (per voxel the record {c, n, eligible}
under the current localise and surfel configuration), the carve's misses when the gate is on, segment ends (n, 3) in the sensor
frame, a pose matrix M (4 x 4, used as it stands) and a config (DEFAULTS).
A ray is the segment from O = M[:3, 3] to E = map_transform_point(M, p).  Skip rule, set-up and stepping are the carve's with
this config's max_range; a skipped ray has status SKIPPED, range -1.0, id -1.
Visited: the start cell, then every cell stepped into, the end cell included (n + 1 cells for n steps).
A visited cell that is a voxel counts when N >= min_count and, with carve_gate set, not
(Mv >= min_miss and (double) Mv > miss_ratio * (double) N).
Per counting voxel with record R:  u = R.c - O,  tt = ((ux*Dx + uy*Dy) + uz*Dz) / DD,  w = u - tt * D.
Centroid test: a hit when 0 <= tt <= 1 and (wx*wx + wy*wy) + wz*wz <= radius2; t = tt.
Plane test, instead, when planes != 0 and R.eligible and den = (nx*Dx + ny*Dy) + nz*Dz != 0:
tp = ((nx*ux + ny*uy) + nz*uz) / den,  e = tp * D - u;  a hit when 0 <= tp <= 1 and (ex*ex + ey*ey) + ez*ez <= radius2; t = tp.
With planes == 2 a counting voxel that is not eligible or has den == 0 is passed through and is not `tested`.
radius = radius_cells * voxel, radius2 = radius * radius.  The first hit in visiting order ends the walk: HIT_CENTROID or
HIT_PLANE, range = t * L, id the voxel.  No hit by the end cell: MISS, -1.0, -1."""
from __future__ import annotations

import numpy as np

import closed_map_carve_np as CN
import voxel_map_np as VN

DEFAULTS = dict(max_range=120.0, radius_cells=0.75, planes=1, min_count=1, min_miss=3, miss_ratio=1.0, carve_gate=0)
SKIPPED, MISS, HIT_CENTROID, HIT_PLANE = 0, 1, 2, 3


def counting(V, cfg, misses):
    """the voxels a ray can hit"""
    keep = V.N >= cfg["min_count"]
    if cfg["carve_gate"]:
        Mv = np.asarray(misses, np.int64)
        keep &= ~((Mv >= cfg["min_miss"]) & (Mv.astype(np.float64) > np.float64(cfg["miss_ratio"]) * V.N.astype(np.float64)))
    return keep


def cast(T, V, ends, M, cfg=None, misses=None):
    """One call -> dict(status (n,) uint8, ranges (n,) float64, ids (n,) int32, info: what the device reports without launches
    and prepared)"""
    cfg = dict(DEFAULTS, **(cfg or {}))
    M = np.asarray(M, np.float64).reshape(4, 4)
    v, o = float(V.voxel), np.asarray(V.origin, np.float64)
    E = CN.transform(M, ends)
    O = np.broadcast_to(M[:3, 3], E.shape)
    with np.errstate(all="ignore"):
        D = E - O
        DD = CN.dot(D, D)
        L = np.sqrt(DD)
        s0, s1 = (O - o) / v, (E - o) / v
        inside = (np.abs(np.floor(s0)) < VN.LIMIT).all(axis=1) & (np.abs(np.floor(s1)) < VN.LIMIT).all(axis=1)
        ok = np.isfinite(E).all(axis=1) & ~(L > cfg["max_range"]) & ~(L == 0.0) & inside
    take = np.flatnonzero(ok)
    O, D, DD, L = O[take], D[take], DD[take], L[take]
    radius = np.float64(cfg["radius_cells"]) * np.float64(v)
    r2 = radius * radius
    counts = counting(V, cfg, misses) if len(V.keys) else np.zeros(0, bool)
    planes = int(cfg["planes"])
    status = np.full(len(take), MISS, np.uint8)
    rng = np.full(len(take), -1.0)
    ids = np.full(len(take), -1, np.int32)
    alive = np.ones(len(take), bool)
    tally = dict(steps=0, tested=0)

    def visit(rows, cells):
        on = alive[rows]
        rows, cells = rows[on], cells[on]
        tally["steps"] += len(rows)
        vid = T.find(cells)
        has = vid >= 0
        has[has] = counts[vid[has]]
        rows, vid = rows[has], vid[has]
        if not len(rows):
            return
        Dr = D[rows]
        u = T.c[vid] - O[rows]
        nrm = T.n[vid]
        with np.errstate(all="ignore"):
            tt = CN.dot(u, Dr) / DD[rows]
            w = u - tt[:, None] * Dr
            hit_c = (0.0 <= tt) & (tt <= 1.0) & (CN.dot(w, w) <= r2)
            den = CN.dot(nrm, Dr)
            tp = CN.dot(nrm, u) / den
            e = tp[:, None] * Dr - u
            hit_p = (0.0 <= tp) & (tp <= 1.0) & (CN.dot(e, e) <= r2)
            plane = (planes != 0) & T.eligible[vid] & (den != 0.0)
        tested = plane | (planes != 2)
        hit = np.where(plane, hit_p, hit_c) & tested
        tally["tested"] += int(tested.sum())
        t = np.where(plane, tp, tt)
        rows, vid, plane, t = rows[hit], vid[hit], plane[hit], t[hit]
        status[rows] = np.where(plane, HIT_PLANE, HIT_CENTROID)
        rng[rows] = t * L[rows]
        ids[rows] = vid
        alive[rows] = False

    W = CN.Walk(s0[take], s1[take])
    for rows, cells in W:
        visit(rows, cells)
    rows = np.flatnonzero(alive)
    visit(rows, W.c[rows])

    out_s = np.full(len(E), SKIPPED, np.uint8)
    out_r = np.full(len(E), -1.0)
    out_i = np.full(len(E), -1, np.int32)
    out_s[take], out_r[take], out_i[take] = status, rng, ids
    info = dict(rays=len(E), skipped=int(len(E) - len(take)), missed=int((out_s == MISS).sum()),
                hits_centroid=int((out_s == HIT_CENTROID).sum()), hits_plane=int((out_s == HIT_PLANE).sum()),
                steps=int(tally["steps"]), tested=int(tally["tested"]))
    return dict(status=out_s, ranges=out_r, ids=out_i, info=info)


class Handle:
    """the restatement behind the device handle's closed_map_raycast, for host-side helpers that take a handle
    (tloam_amd.raycast.scan_check)"""

    def __init__(self, T, V, cfg=None, misses=None):
        self.T, self.V, self.cfg, self.misses = T, V, cfg, misses

    def closed_map_raycast(self, ends, pose, want_ids=False):
        R = cast(self.T, self.V, ends, pose, self.cfg, self.misses)
        return R["status"], R["ranges"], (R["ids"] if want_ids else None), R["info"]
