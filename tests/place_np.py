"""numpy restatement of the place recognition stage -- what tloam_place_describe, tloam_place_add_scan
and the odometry frame's keyframes are checked against, bit for bit.

Descriptor (Scan Context, Kim & Kim, IROS 2018), fp64, in the sensor frame:
    a return is used when finite and 0 < r < max_radius, r = sqrt(x*x + y*y)
    ring   = floor(r / (max_radius / n_rings)),                        clamped to n_rings - 1
    sector = floor((atan2(y, x) + pi) / ((2 pi) / n_sectors)),         clamped to n_sectors - 1
    bin    = max(z + height_offset) over its returns (taken on the order-preserving integer image `okey`); empty: 0.0
Keys, summed in index order (explicit loops, never np.sum's pairwise order):
    ring_key[i]   = (desc[i, 0] + desc[i, 1] + ... + desc[i, S-1]) / S
    sector_key[j] = (desc[0, j] + desc[1, j] + ... + desc[R-1, j]) / R
Search for keyframe q over keyframes 0 .. q - exclude_recent:
    key distance  = sum over rings in order of (kq[i] - kc[i]) * (kq[i] - kc[i]); the num_candidates smallest, ties to the lower id
    column norm   n[j] = sqrt(sum over rings in order of v[i, j] * v[i, j])
    cos           = (sum over rings in order of q[i, j] * c[i, (j + s) % S]) / (nq[j] * nc[(j + s) % S])
    d(s)          = 1 - (sum over valid j in order of cos) / n_valid   (valid: both norms non-zero; d = 1 when none is)
    best pair     = min d, ties to the lower shift, then the lower keyframe id; a loop when d < dist_thres
    yaw           = s * ((2 pi) / S), minus 2 pi when above pi: the query's heading relative to the match's"""
from __future__ import annotations

import math

import numpy as np

PI = math.pi
TWO_PI = 2.0 * math.pi

DEFAULTS = dict(n_rings=20, n_sectors=60, num_candidates=10, exclude_recent=50, max_radius=80.0, height_offset=2.0,
                kf_dist=1.0, kf_angle=0.2, dist_thres=0.30)


def cfg_of(**over):
    c = dict(DEFAULTS)
    for k, v in over.items():
        if k not in c:
            raise KeyError(k)
        c[k] = v
    return c


def okey(v):
    """the order-preserving unsigned image of fp64 values (0 is below every image: the empty bin)"""
    b = np.ascontiguousarray(v, np.float64).view(np.uint64)
    neg = (b >> np.uint64(63)) != 0
    return np.where(neg, ~b, b | np.uint64(1 << 63))


def from_okey(k):
    k = np.asarray(k, np.uint64)
    top = (k >> np.uint64(63)) != 0
    b = np.where(top, k & np.uint64((1 << 63) - 1), ~k)
    return np.where(k == 0, np.uint64(0), b).view(np.float64)


def bins(xyz, n_rings=20, n_sectors=60, max_radius=80.0, **_):
    """(ring, sector, used) of every return"""
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    x, y = p[:, 0], p[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.sqrt(x * x + y * y)
        used = np.isfinite(p).all(axis=1) & (r > 0.0) & (r < max_radius)
        ring = np.floor(r / (max_radius / n_rings))
        sector = np.floor((np.arctan2(y, x) + PI) / (TWO_PI / n_sectors))
    ring = np.where(used, np.minimum(ring, n_rings - 1), 0).astype(np.int64)
    sector = np.where(used, np.minimum(sector, n_sectors - 1), 0).astype(np.int64)
    return ring, sector, used


def describe(xyz, **cfg):
    """(descriptor (R, S), ring_key (R,), sector_key (S,))"""
    c = cfg_of(**cfg)
    R, S = c["n_rings"], c["n_sectors"]
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    ring, sector, used = bins(p, **c)
    flat = np.zeros(R * S, np.uint64)
    v = p[used, 2] + c["height_offset"]
    np.maximum.at(flat, (ring * S + sector)[used], okey(v))
    desc = from_okey(flat).reshape(R, S)
    return (desc,) + keys(desc)


def keys(desc):
    R, S = desc.shape
    rk = np.zeros(R)
    for j in range(S):
        rk = rk + desc[:, j]
    sk = np.zeros(S)
    for i in range(R):
        sk = sk + desc[i, :]
    return rk / float(S), sk / float(R)


def margins(xyz, eps=1e-9, **cfg):
    """indices of the used returns within eps of a ring or sector boundary (where the device's atan2 may bin otherwise)"""
    c = cfg_of(**cfg)
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    _, _, used = bins(p, **c)
    x, y = p[:, 0], p[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.sqrt(x * x + y * y) / (c["max_radius"] / c["n_rings"])
        w = (np.arctan2(y, x) + PI) / (TWO_PI / c["n_sectors"])
        near = (np.abs(u - np.round(u)) < eps) | (np.abs(w - np.round(w)) < eps)
    return np.flatnonzero(used & near)


def col_norms(desc):
    acc = np.zeros(desc.shape[1])
    for i in range(desc.shape[0]):
        acc = acc + desc[i] * desc[i]
    return np.sqrt(acc)


def shift_distances(dq, dc):
    """d(s) for s = 0 .. S-1"""
    R, S = dq.shape
    nq, nc = col_norms(dq), col_norms(dc)
    j = np.arange(S)
    d = np.empty(S)
    for s in range(S):
        js = (j + s) % S
        dot = np.zeros(S)
        for i in range(R):
            dot = dot + dq[i] * dc[i, js]
        valid = (nq != 0.0) & (nc[js] != 0.0)
        total, nv = 0.0, 0
        with np.errstate(invalid="ignore", divide="ignore"):
            cosv = dot / (nq * nc[js])
        for k in range(S):
            if valid[k]:
                total = total + cosv[k]
                nv += 1
        d[s] = 1.0 - total / float(nv) if nv else 1.0
    return d


def key_distance(kq, kc):
    acc = 0.0
    for a, b in zip(kq, kc):
        e = a - b
        acc = acc + e * e
    return acc


def yaw_of(shift, n_sectors):
    y = shift * (TWO_PI / n_sectors)
    return y - TWO_PI if y > PI else y


class PlaceDB:
    """the keyframe database and its loop records, fed as the device is"""

    def __init__(self, **cfg):
        self.c = cfg_of(**cfg)
        self.desc, self.rkey, self.skey, self.poses, self.frames, self.loops = [], [], [], [], [], []
        self.last_pose = None

    def is_keyframe(self, pose):
        """the keyframe policy for an accepted frame's returned pose (first one after a reset: always)"""
        if self.last_pose is None:
            return True
        return moved(self.last_pose, pose, self.c["kf_dist"], self.c["kf_angle"])

    def frame(self, xyz, pose, frame_id):
        """an accepted odometry frame: added when the policy says so"""
        if self.is_keyframe(pose):
            self.add(xyz, pose, frame_id)
            return True
        return False

    def add(self, xyz, pose, frame_id):
        d, rk, sk = describe(xyz, **{k: self.c[k] for k in ("n_rings", "n_sectors", "max_radius", "height_offset")})
        self.add_described(d, rk, sk, pose, frame_id)

    def add_described(self, d, rk, sk, pose, frame_id):
        q = len(self.desc)
        self.desc.append(d); self.rkey.append(rk); self.skey.append(sk)
        self.poses.append(np.array(pose, float)); self.frames.append(int(frame_id))
        self.last_pose = np.array(pose, float)
        best = self.search(q)
        if best is not None and best[0] < self.c["dist_thres"]:
            dist, shift, m = best
            self.loops.append(dict(query=q, query_frame=self.frames[q], match=m, match_frame=self.frames[m], shift=shift,
                                   d=dist, yaw=yaw_of(shift, self.c["n_sectors"])))

    def candidates(self, q):
        m = q - self.c["exclude_recent"] + 1
        if m <= 0:
            return []
        dist = [key_distance(self.rkey[q], self.rkey[k]) for k in range(m)]
        order = sorted(range(m), key=lambda k: (dist[k], k))
        return order[: min(self.c["num_candidates"], m)]

    def search(self, q):
        """(d, shift, keyframe) of the best pair, or None when nothing is old enough"""
        best = None
        for k in self.candidates(q):
            d = shift_distances(self.desc[q], self.desc[k])
            s = int(np.argmin(d))   # (the first of equal minima: the lower shift)
            cand = (float(d[s]), s, k)
            if best is None or cand < best:
                best = cand
        return best


def moved(A, B, kf_dist, kf_angle):
    """B has moved at least kf_dist, or turned at least kf_angle, from A: the distance sqrt(dx*dx + dy*dy + dz*dz) of the
    translations, the angle acos(clamp((tr(R_A^T R_B) - 1) / 2)) with the trace summed column by column, row by row"""
    dx, dy, dz = B[0, 3] - A[0, 3], B[1, 3] - A[1, 3], B[2, 3] - A[2, 3]
    dist = math.sqrt(dx * dx + dy * dy + dz * dz)
    tr = 0.0
    for i in range(3):
        for k in range(3):
            tr = tr + A[k, i] * B[k, i]
    cs = min(1.0, max(-1.0, (tr - 1.0) * 0.5))
    return dist >= kf_dist or math.acos(cs) >= kf_angle
