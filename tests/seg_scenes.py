"""Named small scans for the segmentation node: one per branch family of tl_seg.hip that a street scan
reaches only by accident.  tests/test_seg_scenes.py checks every scene on the CPU (empty margin report, witness, status);
tests/test_gpu_segmentation_edges.py runs every scene on the device against the restatement.

A scene is (name, xyz, SegCfg overrides, first_frame, witness, status): xyz is float32-rounded float64, at most 20 k returns;
witness(xyz, cfg, first_frame, out) is a predicate on the restatement's output / intermediates that proves the scene reaches
the branch it is named for; status is what the node answers.

Hand-made scenes put a flat ground patch (second world quadrant, beyond the last section bound) in front of their object
points: it pulls the z mean down, so every object point lies above the height split and object_scan is the hand-made list
in scan order."""
from __future__ import annotations

import dataclasses
import functools
from typing import Callable, NamedTuple

import numpy as np

import segmentation_np as S
from tloam_amd import synth_hdl64 as G

MAX_RETURNS = 20000
FRONT_THREADS = 1024      # k_seg_front's block: one contiguous chunk of ceil(n / 1024) returns per thread


class Scene(NamedTuple):
    name: str
    xyz: np.ndarray
    over: dict
    first_frame: bool
    witness: Callable
    status: int = S.STATUS_OK


def cfg_of(over) -> S.SegCfg:
    return dataclasses.replace(S.SegCfg(), **over)


def seg_config(reg, cfg: S.SegCfg):
    """SegCfg -> the binding's SegConfig, field by field"""
    return reg.default_seg_config(
        sensor_model=cfg.sensorModel, scan_period=cfg.scanPeriod, sensor_height=cfg.sensorHeight,
        vertical_res=cfg.verticalRes, init_angle=cfg.initAngle, sensor_min_range=cfg.sensorMinRange,
        sensor_max_range=cfg.sensorMaxRange, near_dis=cfg.near_dis, quadrant=cfg.quadrant, num_sec=cfg.numSec, dis=cfg.dis,
        max_iter=cfg.maxIter, ground_seed_num=cfg.ground_seed_num, ring_min_num=cfg.ringMinNum, start_r=cfg.startR,
        delta_r=cfg.deltaR, delta_p=cfg.deltaP, delta_a=cfg.deltaA, min_seg=cfg.minSeg)


def f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, 3).astype(np.float32).astype(np.float64))


# ---- intermediates of the restatement, for the witnesses ------------------------------------------------
def regions(xyz, cfg):
    """current_scan split as ground_stage splits it -> (cur, region per entry, section bounds)"""
    kept, _ = S.near_filter(xyz, cfg)
    P = xyz[kept]
    s = 0.0
    for v in P[:, 2]:
        s += v
    mean = (s / float(len(P)) if len(P) else 1.0) + 0.5
    cur = kept[~(P[:, 2] > mean)]
    bounds = S.section_bounds(cfg)
    reg, _ = S.region_of(xyz[cur], bounds, cfg)
    return cur, reg, bounds


def subsample(P, cfg):
    """one region's points -> (region-local ids of the subsample sorted by (z, k), ids of the seeds)"""
    k = np.arange(len(P))
    r3 = np.sqrt((P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1]) + P[:, 2] * P[:, 2])
    sub = (k % 10 == 0) & (P[:, 2] >= -1.5 * cfg.sensorHeight) & (r3 >= cfg.sensorMinRange) & (r3 <= cfg.sensorMaxRange)
    si = k[sub]
    order = si[np.lexsort((si, P[si, 2]))]
    low = P[order[: cfg.ground_seed_num], 2]
    av = float(np.sum(low)) / len(low) if len(low) else 0.0
    return order, order[P[order, 2] < av + cfg.dis]


def object_voxels(xyz, cfg, first_frame, out):
    return S.polar_voxels(xyz[out["object"]], cfg, first_frame)


def components_plain(V):
    """the declared partition with no shortcut: every point's own searchKNN edges, taken as undirected"""
    vm = S._voxel_map(V)
    n = len(V["pol"])
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i in range(n):
        for j in S._neighbours(i, V, vm):
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], np.int64)


def hash_home(key, mask):
    return ((int(key) * 2654435761) & 0xFFFFFFFF) & mask


def transitions(xyz, cfg):
    kept, _ = S.near_filter(xyz, cfg)
    q = S.quadrant_code(xyz[kept, 0], xyz[kept, 1])
    return int(((q[1:] == 1) & (q[:-1] == 4)).sum())


def ring_entries(xyz, cfg, out, ring):
    """the segmented points of one ring in segmented order -> (input indices, sector ranges [(s0, s1)], curvature)"""
    seg = out["segmented"]
    ids = seg[out["ring"][seg] == ring]
    if len(ids) < max(cfg.ringMinNum, 11):
        return ids, [], np.zeros(0)
    tp = len(ids) - 10
    L = tp // 6
    sec = [(L * j, L * (j + 1) - 1 if j != 5 else tp - 1) for j in range(6)]
    return ids, sec, S.curvature(xyz[ids])


# ---- building blocks ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def street(seed=0, n_az=256, extra=()):
    rings = np.concatenate([np.arange(64), np.asarray(extra, np.int64)]) if extra else None
    W = G.make_street(seed)
    return G.scan(W, G.trajectory(1)[0], seed=seed, n_az=n_az, rings=rings)


def patch(n, seed):
    """flat ground, one region (x < 0 < y, beyond the last section bound): all of it comes out as ground"""
    r = np.random.default_rng(9000 + seed)
    return np.column_stack([-r.uniform(15.0, 40.0, n), r.uniform(2.0, 25.0, n), -1.73 + r.normal(0.0, 0.01, n)])


def polar(rho, pitch_deg, az_deg):
    rho, p, a = np.broadcast_arrays(np.asarray(rho, np.float64), np.deg2rad(np.asarray(pitch_deg, np.float64)),
                                    np.deg2rad(np.asarray(az_deg, np.float64)))
    return np.column_stack([(rho * np.cos(p) * np.cos(a)).ravel(), (rho * np.cos(p) * np.sin(a)).ravel(),
                            (rho * np.sin(p)).ravel()])


def over_ground(objs, seed, ratio=3):
    """ground patch, then the object points: object_scan is `objs` in its order (checked by the witness helper `objects_are`)"""
    objs = np.asarray(objs, np.float64).reshape(-1, 3)
    g = patch(max(200, ratio * len(objs)), seed)
    return f32(np.concatenate([g, objs])), len(g)


def objects_are(out, n_ground, n):
    return np.array_equal(out["object"], np.arange(n_ground, n)) and len(out["ground"]) == n_ground


# ---- front ---------------------------------------------------------------------------------------------------
def _front_70_sweeps():
    xyz, _ = street(3, 180, tuple(range(30, 64)))     # the lowest sweeps fall to the near filter

    def w(xyz, cfg, ff, out):
        return transitions(xyz, cfg) >= 64 and out["ring"].max() == 63 and (out["ring"] == 63).sum() > 2 * 180
    return Scene("front_70_sweeps", xyz, dict(minSeg=5), True, w)


_ANGLE_360 = f32([[20.0, 1e-6, -1.7], [35.0, 2e-6, -1.9], [50.0, 1e-6, -2.0]])


def _front_angle_360():
    base, ring = street(4)
    cut = [int(np.searchsorted(ring, r)) for r in (8, 20, 33)]      # each goes in front of a sweep: q1 after q4
    xyz = np.insert(base, cut, _ANGLE_360, axis=0)
    at = np.asarray(cut) + np.arange(3)

    def w(xyz, cfg, ff, out):
        cur, reg, _ = regions(xyz, cfg)
        pos = np.searchsorted(cur, at)
        used = set(out["ground"].tolist()) | set(out["object"].tolist())
        return (np.array_equal(cur[pos], at) and (reg[pos] == -1).all() and (out["ring"][at] >= 0).all()
                and not (set(at.tolist()) & used)
                and (S.fast_atan2(-xyz[at, 1], xyz[at, 0]) == np.float32(360.0)).all())
    return Scene("front_angle_360", xyz, dict(minSeg=5), True, w)


def _front_nan_run():
    base, ring = street(5)
    cut = int(np.searchsorted(ring, 40))
    run = np.full((64, 3), np.nan)
    run[1::2, 0] = np.inf
    run[::4, 2] = -np.inf
    run[::2, 1] = 7.0
    xyz = np.insert(base, [cut] * 64, run, axis=0)

    def w(xyz, cfg, ff, out):
        chunk = -(-len(xyz) // FRONT_THREADS)
        a, b = xyz[cut - 1], xyz[cut + 64]
        return (64 > 2 * chunk + chunk and (out["ring"][cut:cut + 64] == -1).all()
                and S.quadrant_code(a[:1], a[1:2])[0] == 4 and S.quadrant_code(b[:1], b[1:2])[0] == 1
                and out["ring"][cut - 1] >= 0 and out["ring"][cut + 64] == out["ring"][cut - 1] + 1)
    return Scene("front_nan_run", xyz, dict(minSeg=5), True, w)


def _front_n(n):
    base, ring = street(6)
    lo = int(np.searchsorted(ring, 44)) - 3       # starts three returns before a sweep's end
    xyz = base[lo:lo + n]
    return Scene(f"front_n_{n}", xyz, dict(minSeg=0, ringMinNum=16), True, lambda xyz, cfg, ff, out: len(xyz) == n,
                 S.STATUS_TOO_FEW if n == 1 else S.STATUS_OK)


# ---- ground --------------------------------------------------------------------------------------------------
def _ground_regions():
    r = np.random.default_rng(11)
    A = np.column_stack([r.uniform(16, 30, 30), -r.uniform(2, 20, 30), -1.73 + r.normal(0, 0.01, 30)])     # 3 seeds
    B = np.column_stack([-r.uniform(16, 30, 31), -r.uniform(2, 20, 31), -1.73 + r.normal(0, 0.01, 31)])    # 4 seeds
    # the skipped tail: seeds 0, 10, 20 on z = -1.9 and seed 30 at the triangle's centroid 0.5 m below; the plane settles
    # 0.125 m under the triangle, seed 30 is 0.375 m off it, every other k % 5 == 0 point 0.6 m: the fit set falls to 3
    C = np.column_stack([-r.uniform(18, 32, 36), r.uniform(4, 15, 36), np.full(36, -1.9)])
    C[[0, 10, 20]] = [[-20.0, 5.0, -1.9], [-30.0, 5.0, -1.9], [-25.0, 14.0, -1.9]]
    C[30] = [-25.0, 8.0, -2.4]
    C[[5, 15, 25, 35], 2] = -1.4
    D = np.tile([[16.0, 4.0, -1.75]], (31, 1))                                                              # zero normal
    a, z = np.meshgrid(np.arange(5.0, 6.0, 0.1), np.arange(1.0, 3.0, 0.2), indexing="ij")
    wall = np.column_stack([np.full(a.size, 20.0), a.ravel(), z.ravel()])
    xyz = f32(np.concatenate([A, B, C, D, wall]))
    iA, iB, iC, iD = np.arange(0, 30), np.arange(30, 61), np.arange(61, 97), np.arange(97, 128)

    def w(xyz, cfg, ff, out):
        cur, reg, _ = regions(xyz, cfg)
        mem = {int(q): cur[reg == q * cfg.numSec + 2] for q in range(4)}
        if not all(np.array_equal(mem[q], i) for q, i in ((0, iA), (1, iB), (2, iC), (3, iD))):
            return False
        g, o = set(out["ground"].tolist()), set(out["object"].tolist())
        seeds = {q: subsample(xyz[mem[q]], cfg)[1] for q in range(4)}
        ok = len(seeds[0]) == 3 and not (set(iA.tolist()) & (g | o))
        ok &= len(seeds[1]) == 4 and len(set(iB.tolist()) & g) > 4
        ok &= len(seeds[2]) == 4 and (set(iC.tolist()) & g) == set(iC[[0, 10, 20]].tolist()) and not (set(iC.tolist()) & o)
        pl = S.find_best_plane(xyz[iD][seeds[3]])
        ok &= len(seeds[3]) == 4 and bool((pl == 0).all()) and set(iD.tolist()) <= g
        return bool(ok)
    return Scene("ground_regions", xyz, dict(minSeg=5), True, w)


def _ground_region_sizes():
    r = np.random.default_rng(12)
    big = np.column_stack([-r.uniform(15, 60, 10300), r.uniform(2, 40, 10300), -1.73 + r.normal(0, 0.01, 10300)])
    y, z = np.meshgrid(np.arange(10.0, 14.0, 0.1), np.arange(-1.6, 2.0, 0.15), indexing="ij")
    wall = np.column_stack([np.full(y.size, -30.0), y.ravel(), z.ravel()])
    one = [[20.0, -5.0, -1.73]]
    ten = np.column_stack([-r.uniform(16, 30, 10), -r.uniform(2, 20, 10), np.full(10, -1.73)])
    eleven = np.column_stack([r.uniform(16, 30, 11), r.uniform(2, 20, 11), np.full(11, -1.73)])
    xyz = f32(np.concatenate([big[:5000], wall, one, big[5000:], ten, eleven]))

    def w(xyz, cfg, ff, out):
        cur, reg, _ = regions(xyz, cfg)
        sizes = np.bincount(reg[reg >= 0], minlength=12)
        return {1, 10, 11} <= set(sizes.tolist()) and sizes.max() > 10240 and len(out["boxes"]) >= 1
    return Scene("ground_region_sizes", xyz, dict(minSeg=5), True, w)


def _street_cfg(name, seed, over, w):
    return Scene(name, street(seed)[0], dict(minSeg=5, **over), True, w)


def _ground_max_iter(it):
    def w(xyz, cfg, ff, out):
        return cfg.maxIter == it and len(out["ground"]) > 1000 and len(out["object"]) > 1000
    return _street_cfg(f"ground_max_iter_{it}", 7, dict(maxIter=it), w)


def _ground_seed_num(num):
    def w(xyz, cfg, ff, out):
        cur, reg, _ = regions(xyz, cfg)
        subs = [len(subsample(xyz[cur[reg == r]], cfg)[0]) for r in range(4 * cfg.numSec)]
        return cfg.ground_seed_num == num and 3 < max(subs) < 1024 and len(out["ground"]) > 0
    return _street_cfg(f"ground_seed_num_{num}", 8, dict(ground_seed_num=num), w)


def _ground_seed_ties():
    xyz = street(9)[0].copy()
    low = xyz[:, 2] < -1.0
    xyz[low, 2] = np.round(xyz[low, 2] * 64.0) / 64.0

    def w(xyz, cfg, ff, out):
        cur, reg, _ = regions(xyz, cfg)
        tied = 0
        for r in range(4 * cfg.numSec):
            P = xyz[cur[reg == r]]
            order, seeds = subsample(P, cfg)
            z = P[order[: cfg.ground_seed_num], 2]
            tied += len(seeds) > 3 and len(z) > 1 and bool((np.diff(z) == 0).any())
        return tied >= 2
    return Scene("ground_seed_ties", xyz, dict(minSeg=5), True, w)


def _ground_num_sec(ns):
    # (the bounds of 16 sections end at 5 m: only returns far below the sensor are inside them and past the near filter)
    r = np.random.default_rng(14)
    deep = f32(polar(r.uniform(9.2, 9.8, 60), -r.uniform(58.0, 68.0, 60), r.uniform(0.0, 360.0, 60)))

    def w(xyz, cfg, ff, out):
        cur, reg, bounds = regions(xyz, cfg)
        if ns == 1:
            return len(bounds) <= 1 and set(reg[reg >= 0].tolist()) <= {0, 1, 2, 3} and len(out["ground"]) > 0
        rad = np.hypot(xyz[cur, 0], xyz[cur, 1])
        beyond = rad >= bounds[-1]
        return (len(bounds) < ns and beyond.any() and ((reg[beyond] % ns == ns - 1) | (reg[beyond] < 0)).all()
                and len(np.unique(reg)) > 12)
    sc = _street_cfg(f"ground_num_sec_{ns}", 10, dict(numSec=ns), w)
    return sc._replace(xyz=np.concatenate([sc.xyz, deep]))


def _ground_sensor_geometry():
    def w(xyz, cfg, ff, out):
        return S.section_bounds(cfg) != S.section_bounds(S.SegCfg()) and len(out["ground"]) > 1000
    return _street_cfg("ground_sensor_geometry", 11, dict(sensorHeight=2.0, initAngle=-20.0, verticalRes=0.5), w)


# ---- polar and voxels ------------------------------------------------------------------------------------
def _polar_straddle_x():
    y, z = np.meshgrid(np.arange(-1.0, 1.01, 0.1), np.arange(0.5, 2.5, 0.2), indexing="ij")
    objs = np.column_stack([np.full(y.size, 20.0), y.ravel() + 0.013, z.ravel()])
    xyz, ng = over_ground(objs, 1)

    def w(xyz, cfg, ff, out):
        V = object_voxels(xyz, cfg, ff, out)
        loc = {int(o): i for i, o in enumerate(out["object"])}
        first = [loc[int(s)] for s in out["segmented"][out["label"] == 1]]
        az = set(V["az"][first].tolist())
        return objects_are(out, ng, len(xyz)) and {0, 300} <= az and len(out["boxes"]) == 1
    return Scene("polar_straddle_x", xyz, dict(minSeg=5), True, w)


def _polar_delta_a_06():
    # column 300 (azimuth 180 deg) and, at the same range and pitch, a patch at 250 deg: only the clamp joins the two.  A second
    # patch at 300 deg stands alone at its range: its points see column 300 and never their own voxel, so each is its own node.
    at180 = polar(20.0, *np.meshgrid([2.5, 2.8], np.arange(179.8, 180.21, 0.1), indexing="ij"))
    at250 = polar(20.0, *np.meshgrid([2.5, 2.8], np.arange(249.8, 250.21, 0.1), indexing="ij"))
    alone = polar(30.0, *np.meshgrid([2.5, 2.8], np.arange(299.8, 300.21, 0.1), indexing="ij"))
    objs = np.concatenate([at180, at250, alone])
    xyz, ng = over_ground(objs, 2)
    n180, n250 = len(at180), len(at250)

    def w(xyz, cfg, ff, out):
        V = object_voxels(xyz, cfg, ff, out)
        lab = S.canonical(S.dcvc_components(V))
        a, b, c = lab[:n180], lab[n180:n180 + n250], lab[n180 + n250:]
        return (objects_are(out, ng, len(xyz)) and V["width"] == 601 and (V["az"] > 301).sum() >= len(b) + len(c)
                and (V["az"][:n180] == 300).any() and len(set(a.tolist()) | set(b.tolist())) == 1
                and len(set(c.tolist())) == len(c) and len(np.unique(S.voxel_key(V["pol"], V["pit"], V["az"], V)[-len(c):])) < len(c))
    return Scene("polar_delta_a_06", xyz, dict(minSeg=0, deltaA=0.6), True, w)


def _polar_delta_a_street(da, seed):
    def w(xyz, cfg, ff, out):
        V = object_voxels(xyz, cfg, ff, out)
        return V["width"] == int(round(360.0 / da)) + 1 and (V["az"].max() > 301) == (da < 1.2) and len(out["boxes"]) > 3
    return _street_cfg(f"polar_delta_a_{str(da).replace('.', '')}_street", seed, dict(deltaA=da), w)


def _polar_top_row():
    # pitches from 0 up to 3.24 deg = 2.7 deltaP: height is 2, the points above 3.0 deg round to row 3
    body = polar(20.0, *np.meshgrid([0.1, 1.3, 2.5], np.arange(40.0, 43.0, 0.3), indexing="ij"))
    top = polar(20.0, [3.1, 3.15, 3.2, 3.24], [41.0, 41.1, 40.9, 41.0])             # one voxel, over the body
    lone = polar(20.0, [3.1, 3.2, 3.24], [100.0, 100.1, 99.9])                      # one voxel, nothing under it
    under = polar(20.0, [0.1] * 3, [99.9, 100.0, 100.1])
    objs = np.concatenate([body, top, lone, under])
    xyz, ng = over_ground(objs, 3)
    nb = len(body)

    def w(xyz, cfg, ff, out):
        V = object_voxels(xyz, cfg, ff, out)
        lab = S.canonical(S.dcvc_components(V))
        key = S.voxel_key(V["pol"], V["pit"], V["az"], V)
        t, l = slice(nb, nb + 4), slice(nb + 4, nb + 7)
        return (objects_are(out, ng, len(xyz)) and V["height"] == 2 and (V["pit"][t] == 3).all() and (V["pit"][l] == 3).all()
                and len(set(key[t].tolist())) == 1 and len(set(key[l].tolist())) == 1
                and (lab[t] == lab[0]).all() and len(set(lab[l].tolist())) == 3)
    return Scene("polar_top_row", xyz, dict(minSeg=0), True, w)


def _polar_all_far():
    objs = polar(np.linspace(121.0, 140.0, 60), np.linspace(0.2, 1.5, 60), np.linspace(10.0, 350.0, 60))
    xyz, ng = over_ground(objs, 4)

    def w(xyz, cfg, ff, out):
        V = object_voxels(xyz, cfg, ff, out)
        return (objects_are(out, ng, len(xyz)) and (np.linalg.norm(xyz[out["object"]], axis=1) > cfg.sensorMaxRange).all()
                and V["polarNum"] == 1 and not V["pol"].any() and not V["az"].any() and len(out["boxes"]) == 1
                and len(out["segmented"]) == 60)
    return Scene("polar_all_far", xyz, dict(minSeg=5), False, w)


def _polar_hash_16():
    # three low returns (their region is dropped: neither ground nor object) and five object points; among candidate
    # azimuths, those whose voxel key starts its probe in the table's last slot: the third and fourth insert wrap to slot 0
    low = [[-20.0, 5.0, -1.7], [-21.0, 6.0, -1.7], [-22.0, 7.0, -1.7]]
    cfg = cfg_of(dict(minSeg=0))
    anchor = polar(20.0, [2.6], [10.0])
    V0 = S.polar_voxels(f32(np.concatenate([anchor, anchor])), cfg, True)
    home, last = [], 10.0
    for a in np.arange(15.0, 340.0, 1.2):
        p = f32(polar(20.0, [2.6], [a]))
        V = S.polar_voxels(np.concatenate([f32(anchor), p]), cfg, True)
        assert V["polarNum"] == V0["polarNum"]
        if hash_home(S.voxel_key(V["pol"], V["pit"], V["az"], V)[1], 15) == 15 and a - last > 4.0:
            home.append(p[0])
            last = a
    objs = np.concatenate([anchor, np.asarray(home[:4])])
    xyz = f32(np.concatenate([low, objs]))
    assert len(xyz) == 8

    def w(xyz, cfg, ff, out):
        V = object_voxels(xyz, cfg, ff, out)
        keys = np.unique(S.voxel_key(V["pol"], V["pit"], V["az"], V))
        return (len(xyz) <= 8 and np.array_equal(out["object"], np.arange(3, 8)) and len(out["ground"]) == 0
                and sum(hash_home(k, 15) == 15 for k in keys) >= 3 and len(out["boxes"]) == 5)
    return Scene("polar_hash_16", xyz, dict(minSeg=0), True, w)


def _chain():
    # a wall one voxel wide around the whole azimuth, and a comb: a spine along the azimuth with a radial tooth every 6 deg
    az = np.arange(0.23, 360.0, 0.4)
    wall = polar(20.0, 2.6, az)
    spine = polar(40.0, 2.6, np.arange(30.13, 150.0, 0.4))
    teeth = np.concatenate([polar(np.arange(40.15, 50.0, 0.15), 2.6, a) for a in np.arange(33.13, 150.0, 6.0)])
    objs = np.concatenate([wall, spine, teeth])
    xyz, ng = over_ground(objs, 5)

    def w(xyz, cfg, ff, out):
        V = object_voxels(xyz, cfg, ff, out)
        sizes = sorted(np.bincount(out["label"])[1:].tolist())
        return (objects_are(out, ng, len(xyz)) and sizes == sorted([len(wall), len(spine) + len(teeth)])
                and len(set(V["pit"][: len(wall)].tolist())) == 1 and len(set(V["az"][: len(wall)].tolist())) == 301)
    return Scene("chain", xyz, dict(minSeg=5), True, w)


# ---- clusters ------------------------------------------------------------------------------------------------
def _isolated(n_az, radii, seed):
    """single returns and pairs, each alone in its voxel neighbourhood (4 deg and 1.5 m apart), in a shuffled order"""
    r = np.random.default_rng(seed)
    A, R = np.meshgrid(2.0 + 4.0 * np.arange(n_az), radii, indexing="ij")
    one = polar(R.ravel(), 2.6, A.ravel())
    pair = r.uniform(size=len(one)) < 0.3
    two = polar(R.ravel()[pair] + 0.01, 2.6, A.ravel()[pair] + 0.01)
    objs = np.concatenate([one, two])
    return objs[r.permutation(len(objs))], len(one), int(pair.sum())


def _clusters_many(name, n_az, radii, lo, hi):
    objs, n_one, n_pair = _isolated(n_az, radii, len(radii))
    xyz, ng = over_ground(objs, 6)

    def w(xyz, cfg, ff, out):
        K = len(out["boxes"])
        size = np.bincount(out["label"])[1:]
        single = size == 1
        return (objects_are(out, ng, len(xyz)) and lo <= K <= hi and K == n_one and (size == 2).sum() == n_pair
                and single.sum() > 1 and not out["boxes"][single, 3:].any() and out["boxes"][~single, 3:].any())
    return Scene(name, xyz, dict(minSeg=0), True, w)


def _blob(rho, az, n):
    """n returns inside one voxel"""
    return polar(rho, 2.6 + 0.01 * np.arange(n), az + 0.01 * np.arange(n))


def _clusters_min_seg_edge():
    sizes = [5, 6, 4, 8, 6, 8, 5, 7]
    objs = np.concatenate([_blob(20.0, 10.0 + 6.0 * i, m) for i, m in enumerate(sizes)])
    xyz, ng = over_ground(objs, 7)

    def w(xyz, cfg, ff, out):
        V = object_voxels(xyz, cfg, ff, out)
        comp = np.bincount(np.unique(S.canonical(S.dcvc_components(V)), return_inverse=True)[1])
        kept = np.bincount(out["label"])[1:].tolist()
        return (objects_are(out, ng, len(xyz)) and sorted(comp.tolist()) == sorted(sizes) and kept == [8, 8, 7, 6, 6]
                and cfg.minSeg == 5)
    return Scene("clusters_min_seg_edge", xyz, dict(minSeg=5), True, w)


def _clusters_none_kept():
    objs = np.concatenate([_blob(20.0, 10.0 + 6.0 * i, 20) for i in range(5)])
    xyz, ng = over_ground(objs, 8)

    def w(xyz, cfg, ff, out):
        return (objects_are(out, ng, len(xyz)) and len(out["segmented"]) == 0 and len(out["boxes"]) == 0
                and (out["ring"] >= 0).all())
    return Scene("clusters_none_kept", xyz, {}, True, w, S.STATUS_TOO_FEW)


# ---- edges ---------------------------------------------------------------------------------------------------
EDGE_RINGS = (640, 15, 640, 16, 320, 17, 640)      # returns per sweep; the sparse sweeps hang on the dense ones around them


def _edges_cylinder():
    """a cylinder of radius 20 m, one pitch row per sweep, all one cluster: segmented order is scan order"""
    rings = []
    for k, m in enumerate(EDGE_RINGS):
        az = (np.arange(m) + 0.5) * (360.0 / m)
        rho = np.full(m, 20.0)
        if k == 0:                      # smooth, a few bumps of 6 cm: single picks with full +-5 marks, then cv <= 0.1 stops
            rho[[50, 200, 330, 331, 480]] += 0.06
        if k == 6:
            rho[[108, 111]] += 0.06     # either side of the first sector boundary (entries 104 | 105 are points 109 | 110)
            rho[260] += 0.1             # a pick whose walk meets the 0.25 m step at 263 after two marks
            rho[263] += 0.25
        R = polar(rho, 1.2 * k + 1.4, az)
        if k == 2:                      # a facet on a dyadic lattice with two equal spikes: exact curvature ties above 0.1
            z = float(np.float32(R[0, 2]))
            i0 = int(np.argmin(np.abs(az - 90.0))) - 16
            x = 3.0 - 0.1875 * np.arange(33)
            F = np.column_stack([x, np.full(33, 20.0), np.full(33, z)])
            F[[8, 24], 1] += 0.5
            R[i0:i0 + 33] = F
        if k == 6:                      # fourteen returns of one point: exact ties at curvature 0
            R[400:414] = R[400]
        rings.append(R)
    objs = np.concatenate(rings)
    xyz, ng = over_ground(objs, 9, ratio=3)
    start = ng + np.concatenate([[0], np.cumsum(EDGE_RINGS)])

    def w(xyz, cfg, ff, out):
        if not (objects_are(out, ng, len(xyz)) and len(out["boxes"]) == 1 and np.array_equal(out["segmented"], out["object"])):
            return False
        cnt = np.bincount(out["ring"][out["segmented"]], minlength=7)[:7]
        edge, gen = set(out["edge"].tolist()), set(out["general"].tolist())
        ok = cnt.tolist() == list(EDGE_RINGS) and cfg.ringMinNum == 16
        ok &= not any(start[k] <= e < start[k + 1] for k in (1, 3) for e in edge | gen)      # 15 and 16: nothing
        ok &= len([e for e in edge | gen if start[5] <= e < start[6]]) == 1                    # 17: one entry
        # a sector with more than 20 picks: 20 edges, and fewer general entries than the rest (the 21st is in neither)
        ids, sec, cv = ring_entries(xyz, cfg, out, 4)
        s0, s1 = sec[0]
        ent = ids[5 + s0:5 + s1]
        n_e, n_g = len(set(ent.tolist()) & edge), len(set(ent.tolist()) & gen)
        ok &= (cv[s0:s1] > 0.1).sum() > 21 and n_e == 20 and n_g == len(ent) - 21
        twenty_first = ent[np.lexsort((np.arange(len(ent)), cv[s0:s1]))[::-1][20]]
        ok &= int(twenty_first) not in edge | gen
        # a sector that stops at cv <= 0.1
        ids, sec, cv = ring_entries(xyz, cfg, out, 0)
        s0, s1 = sec[0]
        ent = ids[5 + s0:5 + s1]
        ok &= 0 < len(set(ent.tolist()) & edge) < 20 and (cv[s0:s1] <= 0.1).any() and int(start[0] + 50) in edge
        ok &= not ({int(start[0] + 50 + d) for d in range(-5, 6) if d} & (edge | gen))         # its +-5 marks
        # picks whose +-5 neighbours cross the sector boundary, the gate broken inside the walk, ties
        ids, sec, cv = ring_entries(xyz, cfg, out, 6)
        ok &= sec[0][1] == 104 and {int(start[6] + 108), int(start[6] + 111), int(start[6] + 260)} <= edge
        ok &= int(start[6] + 109) not in edge | gen                                             # the sector's last entry
        ok &= int(start[6] + 262) not in gen and int(start[6] + 264) in edge | gen            # marked up to the step only
        ok &= int((cv[395:410] == 0.0).sum()) >= 3
        ids, sec, cv = ring_entries(xyz, cfg, out, 2)
        big = cv[cv > 0.1]
        ok &= len(big) - len(np.unique(big)) >= 10
        return bool(ok)
    return Scene("edges_cylinder", xyz, dict(ringMinNum=16), True, w)


_BUILDERS = {
    "front_70_sweeps": _front_70_sweeps, "front_angle_360": _front_angle_360, "front_nan_run": _front_nan_run,
    **{f"front_n_{n}": functools.partial(_front_n, n) for n in (1, 1023, 1024, 1025, 2049)},
    "ground_regions": _ground_regions, "ground_region_sizes": _ground_region_sizes,
    "ground_max_iter_1": functools.partial(_ground_max_iter, 1), "ground_max_iter_5": functools.partial(_ground_max_iter, 5),
    "ground_seed_num_0": functools.partial(_ground_seed_num, 0),
    "ground_seed_num_1024": functools.partial(_ground_seed_num, 1024), "ground_seed_ties": _ground_seed_ties,
    "ground_num_sec_1": functools.partial(_ground_num_sec, 1), "ground_num_sec_16": functools.partial(_ground_num_sec, 16),
    "ground_sensor_geometry": _ground_sensor_geometry,
    "polar_straddle_x": _polar_straddle_x, "polar_delta_a_06": _polar_delta_a_06,
    "polar_delta_a_06_street": functools.partial(_polar_delta_a_street, 0.6, 12),
    "polar_delta_a_24_street": functools.partial(_polar_delta_a_street, 2.4, 13),
    "polar_top_row": _polar_top_row, "polar_all_far": _polar_all_far, "polar_hash_16": _polar_hash_16, "chain": _chain,
    "clusters_k_above_1024": functools.partial(_clusters_many, "clusters_k_above_1024", 88, 12.0 + 1.5 * np.arange(14), 1025, 4000),
    "clusters_k_257_to_1024": functools.partial(_clusters_many, "clusters_k_257_to_1024", 40, 12.0 + 1.5 * np.arange(10), 257, 1024),
    "clusters_min_seg_edge": _clusters_min_seg_edge, "clusters_none_kept": _clusters_none_kept,
    "edges_cylinder": _edges_cylinder,
}
NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def scene(name) -> Scene:
    sc = _BUILDERS[name]()
    assert sc.name == name and len(sc.xyz) <= MAX_RETURNS
    assert np.array_equal(sc.xyz, f32(sc.xyz), equal_nan=True)
    sc.xyz.setflags(write=False)
    return sc


@functools.lru_cache(maxsize=None)
def reference(name, first_frame=None):
    """the restatement's answer for a scene, computed once and shared (read-only) by the tests"""
    sc = scene(name)
    return S.segment(sc.xyz, cfg_of(sc.over), sc.first_frame if first_frame is None else first_frame)


# ---- polarBounds: what is refused, and the largest tables that are not -----------------------------------
BOUNDS_SCENE = "polar_straddle_x"       # object radii from 5 m (the first frame's seed) to a little over 20 m
MAX_BOUNDS = 4096                       # kSegMaxBounds (tl_seg.hpp): a declared limit, DESIGN.md section 11
BOUNDS_CASES = {
    # name: (overrides, what the restatement answers, what the device answers)
    "increment_runs_out": (dict(minSeg=5, deltaR=0.4), S.STATUS_INVALID, S.STATUS_INVALID),
    "above_the_cap": (dict(minSeg=5, startR=0.003, deltaR=0.0), S.STATUS_OK, S.STATUS_INVALID),
    "large_table": (dict(minSeg=5, startR=0.006, deltaR=0.0), S.STATUS_OK, S.STATUS_OK),
}


@functools.lru_cache(maxsize=None)
def bounds_reference(case, first_frame=True):
    return S.segment(scene(BOUNDS_SCENE).xyz, cfg_of(BOUNDS_CASES[case][0]), first_frame)


def bound_count(case, first_frame=True):
    sc = scene(BOUNDS_SCENE)
    cfg = cfg_of(BOUNDS_CASES[case][0])
    V = S.polar_voxels(sc.xyz[reference(BOUNDS_SCENE)["object"]], cfg, first_frame)
    return None if V is None else V["polarNum"]


REUSE_SCENES = ("polar_hash_16", "edges_cylinder", "clusters_k_above_1024")     # run after a 120 k-return scan, as later frames
DETERMINISM_SCENES = ("chain", "clusters_k_above_1024")
BOX_SCENE = "clusters_min_seg_edge"
NO_OBJECT_SCENE = "front_n_1"           # no object point: the node stops before convertToPolar, whatever startR / deltaR are
