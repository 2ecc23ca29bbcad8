"""numpy restatement of loop verification's host and device arithmetic: the target window, T_rel in the
operation order of tl_api_odom.hip's mat_mul / rigid_inverse, the assembly's point transform, and the score."""
import numpy as np


def window(q, m, w):
    """target keyframes of (q, m): [m - w, m + w] clamped to [0, q - 1], ascending"""
    return list(range(max(m - w, 0), min(m + w, q - 1) + 1))


def mat_mul(A, B):
    """4x4 product, each entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3"""
    A, B = np.asarray(A, float), np.asarray(B, float)
    r = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            r[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    return r


def rigid_inverse(T):
    """(R^T, -R^T t), each entry of -R^T t summed in index order"""
    T = np.asarray(T, float)
    r = np.eye(4)
    r[:3, :3] = T[:3, :3].T
    for i in range(3):
        r[i, 3] = -((T[0, i] * T[0, 3] + T[1, i] * T[1, 3]) + T[2, i] * T[2, 3])
    return r


def t_rel(P_m, P_k):
    return mat_mul(rigid_inverse(P_m), P_k)


def move(T, xyz):
    """x' = ((R00 x + R01 y) + R02 z) + t0 per axis, as k_loop_assemble / k_loop_score round it"""
    T = np.asarray(T, float)
    p = np.asarray(xyz, float).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty_like(p)
    for i in range(3):
        out[:, i] = ((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3]
    return out


def assemble(q, m, w, poses, tgt):
    """(the target clouds by kind, in m's frame): tgt[k][kind] the stored target clouds of keyframe k"""
    ks = window(q, m, w)
    out = []
    for kind in range(4):
        parts = [move(t_rel(poses[m], poses[k]), tgt[k][kind]) for k in ks if len(tgt[k][kind])]
        out.append(np.concatenate(parts) if parts else np.zeros((0, 3)))
    return out


def nearest_d2(q, t):
    """squared distance of every query to its nearest target, d0 d0 + d1 d1 + d2 d2 in that order (inf without targets)"""
    if len(t) == 0:
        return np.full(len(q), np.inf)
    if len(q) > 4096:   # (queries by blocks: the same minima, less memory)
        return np.concatenate([nearest_d2(q[s:s + 4096], t) for s in range(0, len(q), 4096)])
    best = np.full(len(q), np.inf)
    for s in range(0, len(t), 2048):
        c = t[s:s + 2048]
        d0 = q[:, None, 0] - c[None, :, 0]
        d1 = q[:, None, 1] - c[None, :, 1]
        d2 = q[:, None, 2] - c[None, :, 2]
        r = d0 * d0
        r = r + d1 * d1
        r = r + d2 * d2
        best = np.minimum(best, r.min(axis=1))
    return best


def score(src, tgt, T, inlier_dist):
    """(overlap, rmse, inliers, points): every source point moved by T, an inlier when its nearest target of the same kind is
    closer than inlier_dist"""
    r2 = inlier_dist * inlier_dist
    inl, ss, pts = 0, 0.0, 0
    for kind in range(4):
        p = move(T, src[kind])
        d = nearest_d2(p, np.asarray(tgt[kind], float).reshape(-1, 3)) if len(p) else np.zeros(0)
        keep = d < r2
        inl += int(keep.sum())
        ss += float(d[keep].sum())
        pts += len(p)
    overlap = inl / pts if pts else 0.0
    rmse = np.sqrt(ss / inl) if inl else np.inf
    return overlap, rmse, inl, pts


SCORE_BLOCKS, SCORE_WAVES, SCORE_LANES = 256, 4, 64    # k_loop_score: 256 blocks of four waves of 64
SCORE_THREADS = SCORE_BLOCKS * SCORE_WAVES * SCORE_LANES


def device_sum(keep, d):
    """(count, sum of d over keep) of one kind, added as k_loop_score and the host add them: thread t takes points t,
    t + 65 536, ... in order from 0.0; each wave the xor butterfly v = v + v[lane ^ off], off = 32 .. 1, lane 0 kept; a block's
    four waves ((w0 + w1) + w2) + w3; the blocks in order from 0.0"""
    keep, d = np.asarray(keep, bool), np.asarray(d, float)
    acc = np.zeros((2, SCORE_THREADS))
    for s in range(0, len(d), SCORE_THREADS):
        k, v = keep[s:s + SCORE_THREADS], d[s:s + SCORE_THREADS]
        n = len(v)
        acc[0, :n] = np.where(k, acc[0, :n] + 1.0, acc[0, :n])
        acc[1, :n] = np.where(k, acc[1, :n] + np.where(k, v, 0.0), acc[1, :n])
    acc = acc.reshape(2, SCORE_BLOCKS, SCORE_WAVES, SCORE_LANES)
    lane = np.arange(SCORE_LANES)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lane ^ off]
    w = acc[..., 0]
    blocks = ((w[:, :, 0] + w[:, :, 1]) + w[:, :, 2]) + w[:, :, 3]
    out = np.zeros(2)
    for b in range(SCORE_BLOCKS):
        out = out + blocks[:, b]
    return float(out[0]), float(out[1])


def score_device_order(src, tgt, T, inlier_dist):
    """score() with every sum in the order of k_loop_score and tloam_loop_verify_*'s host loop: device_sum per kind, the kinds
    added in order 0..3 from 0.0; rmse = sqrt(ss / inl) (inf without inliers), overlap = inl / pts"""
    r2 = inlier_dist * inlier_dist
    inl, ss, pts = 0.0, 0.0, 0
    for kind in range(4):
        p = move(T, src[kind])
        t = np.asarray(tgt[kind], float).reshape(-1, 3)
        if len(p) and len(t):   # (a kind without targets has no grid: its points count, none is an inlier)
            d = nearest_d2(p, t)
            ck, sk = device_sum(d < r2, d)
            inl = inl + ck
            ss = ss + sk
        pts += len(p)
    overlap = inl / float(pts) if pts else 0.0
    rmse = float(np.sqrt(ss / inl)) if inl > 0.0 else np.inf
    return overlap, rmse, int(inl), pts
