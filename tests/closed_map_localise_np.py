"""Localisation of a scan in the closed map restated in fp64 numpy: point-to-plane Gauss-Newton on the
surfels.  It is the contract tl_localise.hip is checked against: ids, residuals and counts bit for bit, the sums within the
bound of another summation order.  No operation here is contracted, and every expression is written in the order the header of
tl_localise.hip states.

Input: a built closed map (tests/voxel_map_np.py's VoxelMapNP), its surfels (tests/closed_map_surfel_np.py: the thirteen sums,
the normals, the variances), a scan (n, 3) in the sensor frame, a prior pose (4 x 4) and a config (DEFAULTS).
Eligible voxel: Ns >= min_points (the surfel config's), ev2 > 0, ev0 <= max_sigma * max_sigma, (ev1 - ev0) >= min_planarity * ev2;
its centre c is the row centroid, its normal n the surfel's.
Per point p and pose matrix M:  E = map_transform_point(M, p), left out when not finite; (i, q) = vmap_quantise(E), unmatched
when |i| >= 2^20 on an axis; the 27 cells i + (dx, dy, dz), dz outermost and dx innermost, each -1, 0, 1 (a cell with
|i| >= 2^20 on an axis is no voxel), the eligible voxel of the smallest D = (d_x*d_x + d_y*d_y) + d_z*d_z, d = E - c, under a
strict <; r = (n_x*d_x + n_y*d_y) + n_z*d_z; used when matched and fabs(r) <= tau.
Over the used points, unit weights: J = [n, E x n], H = sum J^T J (upper triangle by rows, 21 values), g = sum J^T r,
cost = 0.5 * sum r*r.  The iteration, the 6 x 6 Cholesky and the pose update are localise() below."""
from __future__ import annotations

import math

import numpy as np

import closed_map_carve_np as CN
import voxel_map_np as VN

DEFAULTS = dict(max_residual0=1.0, shrink=0.7, min_residual=0.1, max_sigma=float("inf"), min_planarity=0.05, step_tol_t=1e-6,
                step_tol_r=1e-7, min_pivot_ratio=1e-9, max_iterations=20, min_matches=50)
CONVERGED, MAX_ITERATIONS, DEGENERATE = 0, 1, 2
TERMS = 28   # H (21), g (6), cost
UPPER = [(a, b) for a in range(6) for b in range(a, 6)]
EPS = 1e-10  # the Sophus threshold of tl_se3.hpp


class Target:
    """the closed map as the stage sees it: per voxel in id order the record {c, n, eligible}, and the sorted keys"""

    def __init__(self, V, S, normals, evals, min_points=5, max_sigma=float("inf"), min_planarity=0.05):
        self.voxel, self.origin = float(V.voxel), np.asarray(V.origin, np.float64)
        s2 = np.float64(max_sigma) * np.float64(max_sigma)
        with np.errstate(invalid="ignore"):
            self.eligible = (S[:, 0] >= min_points) & (evals[:, 2] > 0.0) & (evals[:, 0] <= s2) & \
                            ((evals[:, 1] - evals[:, 0]) >= np.float64(min_planarity) * evals[:, 2])
        self.c = V.centroids() if len(V.keys) else np.zeros((0, 3))
        self.n = np.asarray(normals, np.float64).reshape(-1, 3)
        self.cells = np.asarray(V.i, np.int64).reshape(-1, 3) if hasattr(V, "i") else None
        self.order = np.argsort(V.keys, kind="stable")
        self.skeys = V.keys[self.order]

    def find(self, cells):
        """ids of the cells (m, 3) int64, -1 where the cell is no voxel"""
        ids = np.full(len(cells), -1, np.int64)
        inside = (np.abs(cells) < VN.LIMIT).all(axis=1)
        if not len(self.skeys) or not inside.any():
            return ids
        key = VN.pack(cells[inside])
        pos = np.minimum(np.searchsorted(self.skeys, key), len(self.skeys) - 1)
        hit = self.skeys[pos] == key
        got = np.full(len(key), -1, np.int64)
        got[hit] = self.order[pos[hit]]
        ids[inside] = got
        return ids


def associate(T, E):
    """E (n, 3) in the map -> (ids (n,) int64, -1 unmatched; d = E - c (n, 3), zero where unmatched)"""
    E = np.asarray(E, np.float64).reshape(-1, 3)
    ids = np.full(len(E), -1, np.int64)
    d = np.zeros((len(E), 3))
    with np.errstate(all="ignore"):
        s = (E - T.origin) / T.voxel
        f = np.floor(s)
        ok = np.isfinite(E).all(axis=1) & (np.abs(f) < VN.LIMIT).all(axis=1)
    rows = np.flatnonzero(ok)
    if not len(rows):
        return ids, d
    cell = f[rows].astype(np.int64)
    best = np.full(len(rows), np.inf)
    bid = np.full(len(rows), -1, np.int64)
    bd = np.zeros((len(rows), 3))
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                cand = T.find(cell + np.array([dx, dy, dz], np.int64))
                cand[cand >= 0] = np.where(T.eligible[cand[cand >= 0]], cand[cand >= 0], -1)
                has = np.flatnonzero(cand >= 0)
                dd = E[rows[has]] - T.c[cand[has]]
                D = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
                better = D < best[has]
                w = has[better]
                best[w], bid[w], bd[w] = D[better], cand[w], dd[better]
    ids[rows], d[rows] = bid, bd
    return ids, d


def linearise(T, points, M, tau):
    """one sweep at the matrix M -> dict(ids, residuals (zero where unmatched), matched, used, terms (used, 28) in point order,
    sums (28,): the terms added in numpy's order)"""
    M = np.asarray(M, np.float64).reshape(4, 4)
    E = CN.transform(M, points)
    ids, d = associate(T, E)
    hit = ids >= 0
    n = np.zeros((len(E), 3))
    n[hit] = T.n[ids[hit]]
    r = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
    used = hit & (np.fabs(r) <= tau)
    Eu, nu, ru = E[used], n[used], r[used]
    J = np.concatenate([nu, np.stack([Eu[:, 1] * nu[:, 2] - Eu[:, 2] * nu[:, 1], Eu[:, 2] * nu[:, 0] - Eu[:, 0] * nu[:, 2],
                                      Eu[:, 0] * nu[:, 1] - Eu[:, 1] * nu[:, 0]], axis=1)], axis=1)
    terms = np.concatenate([np.stack([J[:, a] * J[:, b] for a, b in UPPER], axis=1), J * ru[:, None], (0.5 * (ru * ru))[:, None]],
                           axis=1).reshape(-1, TERMS)
    return dict(ids=ids, residuals=r, matched=int(hit.sum()), used=int(used.sum()), terms=terms, sums=terms.sum(axis=0))


# ---- tl_se3.hpp restated (scalars, no contraction) -------------------------------------------------------------------------
def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def rotate(T, p):
    v = T[1:4]
    uv = cross(v, p)
    uv = (uv[0] + uv[0], uv[1] + uv[1], uv[2] + uv[2])
    c2 = cross(v, uv)
    return (p[0] + T[0] * uv[0] + c2[0], p[1] + T[0] * uv[1] + c2[1], p[2] + T[0] * uv[2] + c2[2])


def se3_exp(a):
    """-> pose (qw, qx, qy, qz, tx, ty, tz)"""
    ox, oy, oz = a[3], a[4], a[5]
    theta_sq = ox * ox + oy * oy + oz * oz
    if theta_sq < EPS * EPS:
        theta = 0.0
        po4 = theta_sq * theta_sq
        imag = 0.5 - (1.0 / 48.0) * theta_sq + (1.0 / 3840.0) * po4
        real = 1.0 - (1.0 / 8.0) * theta_sq + (1.0 / 384.0) * po4
    else:
        theta = math.sqrt(theta_sq)
        half = 0.5 * theta
        imag = math.sin(half) / theta
        real = math.cos(half)
    q = (real, imag * ox, imag * oy, imag * oz)
    om, u = (ox, oy, oz), (a[0], a[1], a[2])
    if theta < EPS:
        t = rotate(q, u)
    else:
        c1 = (1.0 - math.cos(theta)) / theta_sq
        c2 = (theta - math.sin(theta)) / (theta_sq * theta)
        w1 = cross(om, u)
        w2 = cross(om, w1)
        t = tuple(u[k] + c1 * w1[k] + c2 * w2[k] for k in range(3))
    return q + t


def compose(A, B):
    w = A[0] * B[0] - A[1] * B[1] - A[2] * B[2] - A[3] * B[3]
    x = A[0] * B[1] + A[1] * B[0] + A[2] * B[3] - A[3] * B[2]
    y = A[0] * B[2] + A[2] * B[0] + A[3] * B[1] - A[1] * B[3]
    z = A[0] * B[3] + A[3] * B[0] + A[1] * B[2] - A[2] * B[1]
    ln = math.sqrt(w * w + x * x + y * y + z * z)
    rt = rotate(A, B[4:7])
    return (w / ln, x / ln, y / ln, z / ln, A[4] + rt[0], A[5] + rt[1], A[6] + rt[2])


def pose_to_matrix(T):
    qw, qx, qy, qz = T[:4]
    tx, ty, tz = 2.0 * qx, 2.0 * qy, 2.0 * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    M = np.eye(4)
    M[0, :3] = [1.0 - (tyy + tzz), txy - twz, txz + twy]
    M[1, :3] = [txy + twz, 1.0 - (txx + tzz), tyz - twx]
    M[2, :3] = [txz - twy, tyz + twx, 1.0 - (txx + tyy)]
    M[:3, 3] = T[4:7]
    return M


def pose_from_matrix(M):
    """Eigen's quaternion of a rotation matrix, as tl_se3.hpp::pose_from_matrix -> pose, or None for a matrix it refuses"""
    m = np.asarray(M, np.float64).reshape(4, 4)
    if not np.isfinite(m[:3, 3]).all():
        return None
    last = m[3, 0] * m[3, 0] + m[3, 1] * m[3, 1] + m[3, 2] * m[3, 2] + (m[3, 3] - 1.0) * (m[3, 3] - 1.0)
    R = m[:3, :3]
    if not last < EPS or not np.sqrt(((R @ R.T - np.eye(3)) ** 2).sum()) < EPS or not np.linalg.det(R) > 0.0:
        return None
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    q = [0.0] * 4
    if tr > 0.0:
        s = math.sqrt(tr + 1.0)
        q[0] = 0.5 * s
        s = 0.5 / s
        q[1], q[2], q[3] = (m[2, 1] - m[1, 2]) * s, (m[0, 2] - m[2, 0]) * s, (m[1, 0] - m[0, 1]) * s
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        s = math.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[1 + i] = 0.5 * s
        s = 0.5 / s
        q[0], q[1 + j], q[1 + k] = (m[k, j] - m[j, k]) * s, (m[j, i] + m[i, j]) * s, (m[k, i] + m[i, k]) * s
    return (float(q[0]), float(q[1]), float(q[2]), float(q[3]), float(m[0, 3]), float(m[1, 3]), float(m[2, 3]))


# ---- the step ------------------------------------------------------------------------------------------------------------
def solve6(sums, min_pivot_ratio):
    """H d = -g by Cholesky (H = L L^T, rows in order, every inner sum left to right) -> d (6 floats), or None when a pivot
    s_k = H_kk - sum_j L_kj^2 is not > min_pivot_ratio * H_kk"""
    H = [[0.0] * 6 for _ in range(6)]
    for t, (a, b) in enumerate(UPPER):
        H[a][b] = H[b][a] = float(sums[t])
    g = [float(x) for x in sums[21:27]]
    L = [[0.0] * 6 for _ in range(6)]
    for k in range(6):
        s = H[k][k]
        for j in range(k):
            s = s - L[k][j] * L[k][j]
        if not s > min_pivot_ratio * H[k][k]:
            return None
        L[k][k] = math.sqrt(s)
        for i in range(k + 1, 6):
            t = H[i][k]
            for j in range(k):
                t = t - L[i][j] * L[k][j]
            L[i][k] = t / L[k][k]
    y = [0.0] * 6
    for i in range(6):
        t = -g[i]
        for j in range(i):
            t = t - L[i][j] * y[j]
        y[i] = t / L[i][i]
    d = [0.0] * 6
    for i in range(5, -1, -1):
        t = y[i]
        for j in range(i + 1, 6):
            t = t - L[j][i] * d[j]
        d[i] = t / L[i][i]
    return d


def localise(T, points, prior, cfg=None, sums_of=None):
    """-> (pose (4, 4), info, log).  log: per executed iteration dict(pose, tau, matched, used, cost, d); a degenerate
    iteration is logged with d = 0.  sums_of(terms) -> the 28 sums (default: numpy's order)"""
    cfg = dict(DEFAULTS, **(cfg or {}))
    prior = np.asarray(prior, np.float64).reshape(4, 4)
    P = pose_from_matrix(prior)
    assert P is not None
    log = []
    pw = float(cfg["max_residual0"])
    status = MAX_ITERATIONS
    for k in range(int(cfg["max_iterations"])):
        M = pose_to_matrix(P)
        tau = max(float(cfg["min_residual"]), pw)
        L = linearise(T, points, M, tau)
        sums = L["sums"] if sums_of is None else np.asarray(sums_of(L["terms"]), np.float64)
        rec = dict(pose=M, tau=tau, matched=L["matched"], used=L["used"], cost=float(sums[27]), d=np.zeros(6))
        log.append(rec)
        d = None
        if L["used"] >= cfg["min_matches"] and np.isfinite(sums).all():
            d = solve6(sums, float(cfg["min_pivot_ratio"]))
        if d is None:
            status = DEGENERATE
            break
        rec["d"] = np.array(d)
        P = compose(se3_exp(d), P)
        pw = pw * float(cfg["shrink"])
        if math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) < cfg["step_tol_t"] and \
                math.sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5]) < cfg["step_tol_r"]:
            status = CONVERGED
            break
    last = log[-1]
    info = dict(status=status, iterations=len(log), matched=last["matched"], used=last["used"],
                rms=math.sqrt(2.0 * last["cost"] / last["used"]) if last["used"] else 0.0)
    return (prior.copy() if status == DEGENERATE else pose_to_matrix(P)), info, log


def pose_error(A, B):
    """(metres, radians) between two 4 x 4 poses"""
    A, B = np.asarray(A, np.float64).reshape(4, 4), np.asarray(B, np.float64).reshape(4, 4)
    R = A[:3, :3].T @ B[:3, :3]
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.linalg.norm(A[:3, 3] - B[:3, 3])), float(math.atan2(0.5 * np.linalg.norm(w), 0.5 * (np.trace(R) - 1.0)))
