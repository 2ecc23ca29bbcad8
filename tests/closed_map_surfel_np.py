"""The surfels of the closed map restated in int64 / fp64 numpy: the contract the device is checked against
bit for bit.  No operation here is contracted, and every expression is written in the order tl_surfel.hip's header states.

Input: a built closed map (tests/voxel_map_np.py's VoxelMapNP: voxel v, origin o, rows key, N, Q), the K poses and the cloud mask
it was built with, and the keyframes' clouds as they are stored now ([four source clouds, four target clouds] per keyframe).
The points are the build's: keyframes 0 .. K-1 ascending, the mask's slots ascending, stored order; later keyframes add nothing.
Per point p of keyframe k:  E = map_transform_point(P_k, p), left out when not finite; (i, q) = vmap_quantise(E); a keyframe
with a finite point at |i| >= 2^20 adds nothing.  A point whose cell is not a voxel of the map is an orphan: counted, not summed.
Per point and axis a, integers:
    r_a = q_a >> 8,   w_a = (int64) floor(min(max(((O_a - E_a) / v) * 256.0, -2^30), 2^30) + 0.5),   O = the translation of P_k
Per voxel thirteen int64 sums, in this order: Ns, Rx Ry Rz, Sxx Sxy Sxz Syy Syz Szz (S_ab = sum r_a * r_b), Wx Wy Wz.
Per voxel with Ns >= min_points, fp64:
    m_a = (double) R_a / (double) Ns,   c_ab = (double) S_ab / (double) Ns - m_a * m_b,   (lambda ascending, V) = eig3(c),
    n = V[:, 0],   d = (n_x * (double) W_x + n_y * (double) W_y) + n_z * (double) W_z,   n = -n when d < 0,
    sc = v * 2^-16,   ev_a = lambda_a * (sc * sc)
and zeros for a voxel of fewer points.  The eigen solve is the C oracle's orc_eig3_sym (oracle.binding.eig3), the cyclic Jacobi
that tl_knn.hpp's eig3_sym restates."""
from __future__ import annotations

import numpy as np

import closed_map_carve_np as CN
import voxel_map_np as VN
from oracle import binding as ob

SUMS = 13
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
W_CLAMP = float(1 << 30)
DEFAULTS = dict(min_points=5)
READ_DEFAULTS = dict(min_count=1, max_sigma=float("inf"), min_planarity=0.05)


def moments(V, poses, clouds, mask):
    """-> (sums (n_voxels, 13) int64 in id order, orphan points)"""
    v, o = float(V.voxel), np.asarray(V.origin, np.float64)
    order = np.argsort(V.keys, kind="stable")
    skeys = V.keys[order]
    S = np.zeros((len(V.keys), SUMS), np.int64)
    orphans = 0
    for P, c in zip(poses, clouds):   # (the build's K keyframes: zip stops at the poses)
        P = np.asarray(P, np.float64)
        E = CN.transform(P, CN.concatenation(c, mask))
        rows, i, q, over = VN.quantise(E, v, o)
        if over or not len(rows):
            continue
        key = VN.pack(i)
        if len(skeys):
            pos = np.minimum(np.searchsorted(skeys, key), len(skeys) - 1)
            hit = skeys[pos] == key
        else:
            pos, hit = np.zeros(len(key), np.int64), np.zeros(len(key), bool)
        orphans += int((~hit).sum())
        ids = order[pos[hit]]
        r = q[hit] >> 8
        t = ((P[:3, 3] - E[rows][hit]) / v) * 256.0
        w = np.floor(np.minimum(np.maximum(t, -W_CLAMP), W_CLAMP) + 0.5).astype(np.int64)
        per_point = np.concatenate([np.ones((len(ids), 1), np.int64), r] + [(r[:, a] * r[:, b])[:, None] for a, b in PAIRS] + [w], axis=1)
        np.add.at(S, ids, per_point)
    return S, orphans


def solve(S, voxel, min_points=5):
    """-> (normals (n, 3), variances ascending (n, 3), solved (n,) bool)"""
    S = np.asarray(S, np.int64).reshape(-1, SUMS)
    normals, evals = np.zeros((len(S), 3)), np.zeros((len(S), 3))
    solved = S[:, 0] >= min_points
    sc = np.float64(voxel) * np.float64(2.0 ** -16)
    s2 = sc * sc
    for j in np.flatnonzero(solved):
        dN = np.float64(S[j, 0])
        m = S[j, 1:4].astype(np.float64) / dN
        c = np.zeros((3, 3))
        for k, (a, b) in enumerate(PAIRS):
            c[a, b] = c[b, a] = np.float64(S[j, 4 + k]) / dN - m[a] * m[b]
        lam, vec = ob.eig3(c)
        n = vec[:, 0].copy()
        W = S[j, 10:13].astype(np.float64)
        d = (n[0] * W[0] + n[1] * W[1]) + n[2] * W[2]
        if d < 0.0:
            n = -n
        normals[j], evals[j] = n, lam * s2
    return normals, evals, solved


def surfels(V, poses, clouds, mask, min_points=5):
    """-> (sums, normals, variances, the info the device reports without `launches`)"""
    S, orphans = moments(V, poses, clouds, mask)
    normals, evals, solved = solve(S, V.voxel, min_points)
    info = dict(n_keyframes=len(poses), n_points=int(S[:, 0].sum()), orphan_points=orphans, solved_voxels=int(solved.sum()))
    return S, normals, evals, info


def read_box(V, S, evals, lo=None, hi=None, min_count=1, max_sigma=float("inf"), min_planarity=0.05, min_points=5):
    """ids, in id order, of read_box's voxels (lo and hi None: the whole map) whose surfel passes the gate"""
    c = V.centroids()
    sel = V.N >= min_count
    if lo is not None:
        sel &= (c >= np.asarray(lo, np.float64)).all(axis=1) & (c <= np.asarray(hi, np.float64)).all(axis=1)
    s2 = np.float64(max_sigma) * np.float64(max_sigma)
    with np.errstate(invalid="ignore"):
        gate = (S[:, 0] >= min_points) & (evals[:, 2] > 0.0) & (evals[:, 0] <= s2) & \
               ((evals[:, 1] - evals[:, 0]) >= np.float64(min_planarity) * evals[:, 2])
    return np.flatnonzero(sel & gate)
