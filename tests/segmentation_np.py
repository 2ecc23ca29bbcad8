"""Independent numpy restatement of the reference's segmentation node (Segmentation::spinOnce,
src/models/segmentation/segmentation.cpp:40-93) -- what `tloam_segment` (tloam_amd/csrc/tl_seg.hip) is tested against.

Every stage follows segmentation.cpp literally; the places where the reference's order is not defined are declared
 and implemented here the way the device implements them:
  * ground / object order of the four quadrant threads: the order of a std::launch::deferred run, (q, s) ascending;
  * ties of the unstable std::sort calls: by index;
  * DCVC: the device computes connected components over the neighbour edges taken as undirected.  The reference's
    per-point loop (`dcvc_literal`, `dcvc_literal_fast`) is restated too, and `partition_differs` reports the frames where
    the two partitions part.

`segment(xyz, cfg, first_frame)` -> dict of index lists into the caller's array plus `margins`: every point whose gate
(near filter, height split, section bound, seed height, plane distance, polar bound, round() of a voxel coordinate) lies
within 1e-9 of flipping.  A device result may legitimately part from this one only at such a point (its sums run in
another order, its asin / atan2 may differ by an ulp)."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

MARGIN = 1e-9


@dataclass
class SegCfg:
    """config/mapping/segmentation.yaml (the shipped values)"""
    sensorModel: int = 64
    scanPeriod: float = 0.1
    sensorHeight: float = 1.73
    verticalRes: float = 0.4
    initAngle: float = -24.9
    sensorMinRange: float = 1.0
    sensorMaxRange: float = 120.0
    near_dis: float = 3.0
    quadrant: int = 4
    numSec: int = 3
    dis: float = 0.3
    maxIter: int = 3
    ground_seed_num: int = 20
    ringMinNum: int = 131
    startR: float = 0.35
    deltaR: float = 0.0004
    deltaP: float = 1.2
    deltaA: float = 1.2
    minSeg: int = 80


# ---- :472-500 --------------------------------------------------------------------------------------
def near_filter(xyz, cfg: SegCfg):
    """kept original indices (in order) and the norms; the 3-D norm is compared with near_dis^2 (= 9 m)"""
    fin = np.isfinite(xyz).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        nrm = np.sqrt((xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1]) + xyz[:, 2] * xyz[:, 2])
        th = cfg.near_dis * cfg.near_dis
        keep = fin & (nrm >= th)
        near_margin = fin & (np.abs(nrm - th) < MARGIN)
    return np.nonzero(keep)[0], np.nonzero(near_margin)[0]


# ---- :346-361, :363-380 -----------------------------------------------------------------------------
def quadrant_code(x, y):
    q = np.full(len(x), 4, np.int32)
    q[(x <= 0) & (y > 0)] = 2
    q[(x < 0) & (y <= 0) & ~((x <= 0) & (y > 0))] = 3
    q[(x > 0) & (y >= 0)] = 1
    return q


def rings_literal(q, sensor_model=64):
    beam, prev, out = 0, 0, np.zeros(len(q), np.int32)
    for i, c in enumerate(q):
        if c == 1 and prev == 4 and beam < sensor_model - 1:
            beam += 1
        out[i] = beam
        prev = c
    return out


def rings(q, sensor_model=64):
    """the saturating prefix count of q4 -> q1 transitions (the device's form; equal to rings_literal)"""
    prev = np.concatenate([[0], q[:-1]]) if len(q) else q
    t = ((q == 1) & (prev == 4)).astype(np.int64)
    return np.minimum(np.cumsum(t), sensor_model - 1).astype(np.int32)


# ---- :174-223 / :230-237 ----------------------------------------------------------------------------
def section_bounds(cfg: SegCfg):
    """initSections' sectionBounds (float-rounded values stored as double)"""
    width = int(math.ceil(1.0 * cfg.sensorModel) / cfg.numSec)
    bidx = [width * (i + 1) - 1 for i in range(cfg.numSec)]
    prev, ang, out, sb = 0.0, cfg.initAngle, [], 0
    for i in range(cfg.sensorModel):
        if cfg.sensorModel == 64 and i == 31:
            ang += 1.7
        cur = cfg.sensorHeight / math.tan(abs(ang) / 180.0 * math.pi)
        cur = cur if cur < cfg.sensorMaxRange else cfg.sensorMaxRange
        if i >= 1:
            d = abs(cur - prev)
            if d >= 5.0 or d <= 0.0:
                continue
        if sb < len(bidx) and i == bidx[sb] and sb <= 3:
            theta = abs(ang / 180 * math.pi)
            if theta != 0 and i < cfg.sensorModel:
                out.append(float(np.float32(cfg.sensorHeight / math.tan(theta))))
            else:
                out.append(cfg.sensorMaxRange)
            sb += 1
        prev = cur
        ang += cfg.verticalRes
    return out


def get_section(r, bounds, num_sec):
    """a bound past the vector's end never matches (the reference reads sectionBounds[numSec-1] out of range)"""
    s = np.full(len(r), num_sec - 1, np.int32)
    for i in range(min(num_sec, len(bounds)) - 1, -1, -1):
        s[r < bounds[i]] = i
    return s


# ---- OpenCV 4 cv::fastAtan2 (atan_f32, modules/core/src/mathfuncs_core.simd.hpp), recalled -------------
_R2D = np.float32(180.0 / np.pi)
_P1 = np.float32(np.float32(0.9997878412794807) * _R2D)
_P3 = np.float32(np.float32(-0.3258083974640975) * _R2D)
_P5 = np.float32(np.float32(0.1555786518463281) * _R2D)
_P7 = np.float32(np.float32(-0.04432655554792128) * _R2D)
_EPS = np.float32(np.finfo(np.float64).eps)


def fast_atan2(y, x):
    y = np.asarray(y, np.float32)
    x = np.asarray(x, np.float32)
    ax, ay = np.abs(x), np.abs(y)
    big = ax >= ay
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(big, ay / (ax + _EPS), ax / (ay + _EPS)).astype(np.float32)
    c2 = (c * c).astype(np.float32)
    p = ((((_P7 * c2 + _P5) * c2 + _P3) * c2 + _P1) * c).astype(np.float32)
    a = np.where(big, p, np.float32(90.0) - p).astype(np.float32)
    a = np.where(x < 0, np.float32(180.0) - a, a).astype(np.float32)
    a = np.where(y < 0, np.float32(360.0) - a, a).astype(np.float32)
    return a


def region_of(P, bounds, cfg: SegCfg):
    """fillSectionIndex (:507-549): q * numSec + s, or -1 for an angle of 360.0f (in no region)"""
    x, y = P[:, 0], P[:, 1]
    r = np.sqrt(x * x + y * y)
    th = fast_atan2(-y, x)
    s = get_section(r, bounds, cfg.numSec)
    q = np.full(len(P), -1, np.int32)
    for k in range(4):
        q[(th >= 90.0 * k) & (th < 90.0 * (k + 1))] = k
    reg = np.where(q >= 0, q * cfg.numSec + s, -1)
    marg = np.zeros(len(P), bool)
    for b in bounds:
        marg |= np.abs(r - b) < MARGIN
    return reg.astype(np.int32), marg


# ---- :551-616 ---------------------------------------------------------------------------------------
def find_best_plane(F):
    """sequential sums in the given order"""
    cx = cy = cz = 0.0
    for p in F:
        cx += p[0]; cy += p[1]; cz += p[2]
    n = float(len(F))
    cx /= n; cy /= n; cz /= n
    xx = xy = xz = yy = yz = zz = 0.0
    for p in F:
        rx, ry, rz = p[0] - cx, p[1] - cy, p[2] - cz
        xx += rx * rx; xy += rx * ry; xz += rx * rz; yy += ry * ry; yz += ry * rz; zz += rz * rz
    xx /= n; xy /= n; xz /= n; yy /= n; yz /= n; zz /= n
    dets = [yy * zz - yz * yz, xx * zz - xz * xz, xx * yy - xy * xy]
    axes = [(dets[0], xz * yz - xy * zz, xy * yz - xz * yy),
            (xz * yz - xy * zz, dets[1], xy * xz - yz * xx),
            (xy * yz - xz * yy, xy * xz - yz * xx, dets[2])]
    wx = wy = wz = 0.0
    for d, a in zip(dets, axes):
        wgt = d * d
        if wx * a[0] + wy * a[1] + wz * a[2] < 0.0:
            wgt = -wgt
        wx += a[0] * wgt; wy += a[1] * wgt; wz += a[2] * wgt
    nrm = math.sqrt(wx * wx + wy * wy + wz * wz)
    if nrm > 0:            # Eigen >= 3.3 normalize(): a no-op on the zero vector (recalled)
        wx /= nrm; wy /= nrm; wz /= nrm
    d = -(wx * cx + wy * cy + wz * cz)
    return np.array([wx, wy, wz, d])


def plane_dist(P, pl):
    return np.abs(pl[0] * P[:, 0] + pl[1] * P[:, 1] + pl[2] * P[:, 2] + pl[3])


# ---- :626-731 ---------------------------------------------------------------------------------------
def ground_region(P, cfg: SegCfg):
    """one region's points (region order) -> (ground local idx, vertical local idx, margin local idx)"""
    m = len(P)
    marg = []
    if m == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), marg
    k = np.arange(m)
    r3 = np.sqrt((P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1]) + P[:, 2] * P[:, 2])
    sub = (k % 10 == 0) & (P[:, 2] >= -1.5 * cfg.sensorHeight) & (r3 >= cfg.sensorMinRange) & (r3 <= cfg.sensorMaxRange)
    si = k[sub]
    order = si[np.lexsort((si, P[si, 2]))]           # by z, ties by k
    low = P[order[: cfg.ground_seed_num], 2]
    s = 0.0
    for v in low:
        s += v
    av = s / len(low) if len(low) else 0.0
    gate = av + cfg.dis
    seeds = order[P[order, 2] < gate]
    marg += list(order[np.abs(P[order, 2] - gate) < MARGIN])
    if len(seeds) <= 3:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), marg
    fit = seeds
    ground = vert = np.zeros(0, np.int64)
    for it in range(cfg.maxIter):
        if len(fit) <= 3:
            continue
        pl = find_best_plane(P[fit])
        d = plane_dist(P, pl)
        marg += list(k[np.abs(d - cfg.dis) < MARGIN])
        if it < cfg.maxIter - 1:
            fit = k[(d < cfg.dis) & (k % 5 == 0)]
            vert = np.zeros(0, np.int64)
        else:
            fit = k[d < cfg.dis]
            vert = k[~(d < cfg.dis)]
    ground = fit
    return ground, vert, marg


def ground_stage(xyz, cfg: SegCfg):
    n = len(xyz)
    kept, near_m = near_filter(xyz, cfg)
    P = xyz[kept]
    ring_all = np.full(n, -1, np.int32)
    q = quadrant_code(P[:, 0], P[:, 1])
    rg = rings(q, cfg.sensorModel)
    ring_all[kept] = rg
    s = 0.0
    for v in P[:, 2]:
        s += v
    mean = (s / float(len(P)) if len(P) else 1.0) + 0.5     # estimateRingsAndTimes2 returns 1.0 on an empty cloud
    hi = P[:, 2] > mean
    margins = set(near_m.tolist()) | set(kept[np.abs(P[:, 2] - mean) < MARGIN].tolist())
    cur = kept[~hi]
    non_ground = kept[hi]
    bounds = section_bounds(cfg)
    reg, rmarg = region_of(xyz[cur], bounds, cfg)
    margins |= set(cur[rmarg].tolist())
    ground, obj = [], []
    for r in range(cfg.quadrant * cfg.numSec):
        members = cur[reg == r]
        g, v, mg = ground_region(xyz[members], cfg)
        ground.append(members[g]); obj.append(members[v])
        margins |= set(members[np.asarray(mg, np.int64)].tolist())
    obj.append(non_ground)
    return dict(ring=ring_all, ground=np.concatenate(ground).astype(np.int64) if ground else np.zeros(0, np.int64),
                object=np.concatenate(obj).astype(np.int64), margins=margins, mean_height=mean)


# ---- :791-870 ---------------------------------------------------------------------------------------
def std_round(v):
    t = np.trunc(v)
    return (t + np.sign(v) * (np.abs(v - t) >= 0.5)).astype(np.int64)


def polar_voxels(P, cfg: SegCfg, first_frame: bool):
    """convertToPolar + the voxel coordinates of createHashTable.  Returns None when the polarBounds loop would not end."""
    nrm = np.sqrt((P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1]) + P[:, 2] * P[:, 2])
    pitch = np.arcsin(P[:, 2] / nrm) * 180.0 / math.pi
    ang = np.arctan2(P[:, 1], P[:, 0])
    az = np.where(ang > 0.0, ang * 180 / math.pi, (ang + 2 * math.pi) * 180 / math.pi)
    ok = ~((nrm >= cfg.sensorMaxRange) | (nrm <= cfg.sensorMinRange))
    min_pitch = min(0.0, float(pitch[ok].min())) if ok.any() else 0.0
    max_pitch = max(0.0, float(pitch[ok].max())) if ok.any() else 0.0
    seed = 5.0 if first_frame else 0.0
    min_polar = min(seed, float(nrm[ok].min())) if ok.any() else seed
    max_polar = max(seed, float(nrm[ok].max())) if ok.any() else seed
    polar = np.where(ok, nrm, 0.0); pitch = np.where(ok, pitch, 0.0); az = np.where(ok, az, 0.0)
    width = int(std_round(np.array([360.0 / cfg.deltaA]))[0] + 1)
    height = int((max_pitch - min_pitch) / cfg.deltaP)
    rng, step, bounds = min_polar, 1, []
    while rng <= max_polar:
        inc = cfg.startR - step * cfg.deltaR
        if inc <= 0.0:
            return None
        rng += inc
        bounds.append(rng)
        step += 1
    bounds = np.array(bounds)
    P_n = len(bounds)
    pol = np.minimum(np.searchsorted(bounds, polar, side="right"), P_n - 1)
    vp, va = (pitch - min_pitch) / cfg.deltaP, az / cfg.deltaA
    pit, azi = std_round(vp), std_round(va)
    marg = (np.abs(np.abs(vp - np.trunc(vp)) - 0.5) < MARGIN) | (np.abs(np.abs(va - np.trunc(va)) - 0.5) < MARGIN)
    marg |= np.abs(nrm - cfg.sensorMaxRange) < MARGIN
    j = np.searchsorted(bounds, polar)
    for jj in (j - 1, j, j + 1):
        v = (jj >= 0) & (jj < P_n)
        marg[v] |= np.abs(polar[v] - bounds[jj[v]]) < MARGIN
    return dict(pol=pol, pit=pit, az=azi, polarNum=P_n, width=width, height=height, bounds=bounds, margin=marg,
                min_pitch=min_pitch, min_polar=min_polar, max_polar=max_polar)


def voxel_key(pol, pit, az, V):
    Pn, W = V["polarNum"], V["width"]
    return (az * (Pn + 1) + pol) + pit * (Pn + 1) * (W + 1)


def neighbour_keys(pol, pit, az, V):
    """searchKNN (:884-904), in its order"""
    out = []
    for z in (pit - 1, pit, pit + 1):
        if z < 0 or z > V["height"]:
            continue
        for y in (pol - 1, pol, pol + 1):
            if y < 0 or y > V["polarNum"]:
                continue
            for x in (az - 1, az, az + 1):
                ax = x
                if ax < 0:
                    ax = V["width"] - 1
                if ax > 300:
                    ax = 300
                out.append((ax * (V["polarNum"] + 1) + y) + z * (V["polarNum"] + 1) * (V["width"] + 1))
    return out


def _voxel_map(V):
    keys = voxel_key(V["pol"], V["pit"], V["az"], V)
    vm = {}
    for i, k in enumerate(keys.tolist()):
        vm.setdefault(k, []).append(i)
    return vm


def _neighbours(i, V, vm):
    nb = []
    for k in neighbour_keys(int(V["pol"][i]), int(V["pit"][i]), int(V["az"][i]), V):
        nb += vm.get(k, [])
    return nb


def dcvc_literal(V):
    """DCVC (:912-985) as written, O(n^2): small scans only"""
    vm = _voxel_map(V)
    n = len(V["pol"])
    lab = [-1] * n
    cnt = 0
    for i in range(n):
        if lab[i] != -1:
            continue
        nb = _neighbours(i, V, vm) if voxel_key(V["pol"][i], V["pit"][i], V["az"][i], V) in vm else []
        for j in nb:
            cur, ng = lab[i], lab[j]
            if cur != -1 and ng != -1 and cur != ng:
                for t in range(n):
                    if lab[t] == cur:
                        lab[t] = ng
            elif ng != -1:
                lab[i] = ng
            elif cur != -1:
                lab[j] = cur
        if lab[i] == -1:
            cnt += 1
            lab[i] = cnt
            for j in nb:
                lab[j] = cnt
    return np.array(lab, np.int64)


def dcvc_literal_fast(V):
    """the same loop with the relabelling done by a union-find over labels: equal partition, full-size scans"""
    vm = _voxel_map(V)
    n = len(V["pol"])
    lab = np.full(n, -1, np.int64)
    parent = []

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i in range(n):
        if lab[i] != -1:
            continue
        nb = _neighbours(i, V, vm)
        cur = -1
        for j in nb:
            ng = lab[j]
            if ng != -1:
                ng = find(ng)
            if cur != -1 and ng != -1 and cur != ng:
                parent[cur] = ng          # every label `cur` becomes `ng`
                cur = ng
            elif ng != -1:
                cur = ng
            elif cur != -1:
                lab[j] = cur
        if cur == -1:
            parent.append(len(parent))
            cur = len(parent) - 1
            lab[np.asarray(nb, np.int64)] = cur
        lab[i] = cur
    roots = np.array([find(a) for a in range(len(parent))], np.int64)
    return roots[lab]


def dcvc_components(V):
    """the device's partition: connected components over the neighbour edges taken as undirected.  A point whose pitch
    index is height + 1, or whose azimuth index is above 300 (all three of its columns clamp to 300, :898), does not see
    its own voxel: it is a node of its own."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = len(V["pol"])
    vm = _voxel_map(V)
    rows, cols = [], []
    for k, mem in vm.items():
        i0 = mem[0]
        nb = _neighbours(i0, V, vm)
        own = V["pit"][i0] <= V["height"] and V["az"][i0] <= 300
        if own:
            rows += [i0] * (len(mem) - 1); cols += mem[1:]
            rows += [i0] * len(nb); cols += nb
        else:
            for i in mem:
                rows += [i] * len(nb); cols += nb
    A = coo_matrix((np.ones(len(rows), np.int8), (np.asarray(rows, np.int64), np.asarray(cols, np.int64))), shape=(n, n))
    _, lab = connected_components(A, directed=True, connection="weak")
    return lab.astype(np.int64)


def canonical(lab):
    """labels -> the smallest member index of each class (partition identity)"""
    lab = np.asarray(lab)
    first = {}
    out = np.empty(len(lab), np.int64)
    for i, l in enumerate(lab.tolist()):
        out[i] = first.setdefault(l, i)
    return out


def partition_differs(a, b):
    return not np.array_equal(canonical(a), canonical(b))


# ---- :995-1083 --------------------------------------------------------------------------------------
def label_analysis(lab, min_seg):
    """kept clusters (> min_seg members), size descending, ties by smallest member; members ascending"""
    can = canonical(lab)
    roots, counts = np.unique(can, return_counts=True)
    keep = counts > min_seg
    roots, counts = roots[keep], counts[keep]
    order = np.lexsort((roots, -counts))
    return [np.nonzero(can == roots[o])[0] for o in order]


def boxes_of(P, clusters):
    out = np.zeros((len(clusters), 6))
    for c, mem in enumerate(clusters):
        Q = P[mem]
        lo, hi = Q.min(axis=0), Q.max(axis=0)
        ln = hi - lo
        out[c, :3] = lo + ln / 2.0
        out[c, 3:] = np.abs(ln)
    return out


# ---- :1144-1302 -------------------------------------------------------------------------------------
def curvature(R):
    m = len(R)
    j = np.arange(5, m - 5)
    out = []
    for c in range(3):
        v = R[:, c]
        s = v[j - 5] + v[j - 4]
        s = s + v[j - 3]; s = s + v[j - 2]; s = s + v[j - 1]
        s = s - 10 * v[j]
        for o in (1, 2, 3, 4, 5):
            s = s + v[j + o]
        out.append(s)
    dx, dy, dz = out
    return (dx * dx + dy * dy) + dz * dz


def extract_from_section(R, ent, cv):
    """ent: ring-local point ids of the sector's entries, cv: their curvature -> (edge ids, general ids)"""
    order = np.lexsort((ent, cv))
    ent, cv = ent[order], cv[order]
    picked = set()
    edge, cnt = [], 0
    for i in range(len(ent) - 1, -1, -1):
        pid = int(ent[i])
        if pid in picked:
            continue
        if cv[i] <= 0.1:
            break
        cnt += 1
        picked.add(pid)
        if cnt <= 20:
            edge.append(pid)
        else:
            break
        for k in range(1, 6):
            d = R[pid + k] - R[pid + k - 1]
            if (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] > 0.05:
                break
            picked.add(pid + k)
        for k in range(-1, -6, -1):
            d = R[pid + k] - R[pid + k + 1]
            if (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] > 0.05:
                break
            picked.add(pid + k)
    general = [int(p) for p in ent if int(p) not in picked]
    return edge, general


def extract_edges(P_seg, ring_seg, cfg: SegCfg):
    """-> (edge, general) as indices into the segmented list"""
    edge, general = [], []
    for b in range(cfg.sensorModel):
        ids = np.nonzero(ring_seg == b)[0]
        if len(ids) < cfg.ringMinNum:
            continue
        R = P_seg[ids]
        cv = curvature(R)
        tp = len(ids) - 10
        L = tp // 6
        for j in range(6):
            s0 = L * j
            s1 = L * (j + 1) - 1 if j != 5 else tp - 1
            ent = np.arange(s0, s1) + 5
            e, g = extract_from_section(R, ent, cv[s0:s1])
            edge += [int(ids[p]) for p in e]
            general += [int(ids[p]) for p in g]
    return np.array(edge, np.int64), np.array(general, np.int64)


# ---- the node -----------------------------------------------------------------------------------------
STATUS_OK, STATUS_INVALID, STATUS_TOO_FEW = 0, -1, -2


def segment(xyz, cfg: SegCfg | None = None, first_frame: bool = True, literal: str | None = None):
    """Segmentation::spinOnce on one scan.  literal: None, "fast" or "slow": also run the reference's DCVC loop and report
    whether its partition parts from the components (`literal_differs`)."""
    cfg = cfg or SegCfg()
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    e64 = np.zeros(0, np.int64)
    out = dict(status=STATUS_OK, ring=None, ground=e64, object=e64, segmented=e64, label=np.zeros(0, np.int32),
               edge=e64, general=e64, boxes=np.zeros((0, 6)), margins=[], literal_differs=None)
    if cfg.quadrant != 4 or cfg.sensorModel != 64:
        out["status"] = STATUS_INVALID
        return out
    G = ground_stage(xyz, cfg)
    out.update(ring=G["ring"], ground=G["ground"], object=G["object"])
    margins = set(G["margins"])
    obj = G["object"]
    if len(obj) == 0:
        out["status"] = STATUS_TOO_FEW
        out["margins"] = sorted(margins)
        return out
    V = polar_voxels(xyz[obj], cfg, first_frame)
    if V is None:
        out["status"] = STATUS_INVALID
        return out
    margins |= set(obj[V["margin"]].tolist())
    lab = dcvc_components(V)
    if literal:
        lit = dcvc_literal(V) if literal == "slow" else dcvc_literal_fast(V)
        out["literal_differs"] = partition_differs(lab, lit)
    clusters = label_analysis(lab, cfg.minSeg)
    out["margins"] = sorted(margins)
    if not clusters:
        out["status"] = STATUS_TOO_FEW
        return out
    seg_local = np.concatenate(clusters)
    seg = obj[seg_local]
    out["segmented"] = seg
    out["label"] = np.concatenate([np.full(len(c), r + 1, np.int32) for r, c in enumerate(clusters)])
    out["boxes"] = boxes_of(xyz[obj], clusters)
    e, g = extract_edges(xyz[seg], G["ring"][seg], cfg)
    out["edge"], out["general"] = seg[e], seg[g]
    return out
