"""The merged voxel map restated in int64 numpy: the contract the device is checked against bit for bit.

Input per adding frame: the registered scan (tloam_registered_scan's doubles).  Per finite point and axis
    s = (p - o) / v,  i = (int64) floor(s),  q = (int64) floor((s - i) * 2^24 + 0.5)
a frame with |i| >= 2^20 anywhere adds nothing (and counts as an overflow frame).  Per voxel an int64 count N and int64 sums
Q of q; the centroid is o + v * ((double) i + ((double) Q / (double) N) * 2^-24).  Ids in order of creation; a frame's new
voxels in order of their smallest point index in its scan."""
from __future__ import annotations

import numpy as np

BITS = 20
LIMIT = 1 << BITS
QSCALE = float(1 << 24)


def quantise(points, voxel=1.0, origin=(0.0, 0.0, 0.0)):
    """(row indices of the finite points, i (m, 3) int64, q (m, 3) int64, overflow)"""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    rows = np.flatnonzero(np.isfinite(P).all(axis=1))
    s = (P[rows] - np.asarray(origin, dtype=np.float64)) / float(voxel)
    f = np.floor(s)
    with np.errstate(invalid="ignore"):
        over = bool((~(np.abs(f) < LIMIT)).any())
    if over:
        return rows, None, None, True
    q = np.floor((s - f) * QSCALE + 0.5).astype(np.int64)
    return rows, f.astype(np.int64), q, False


def pack(i):
    """the device's key: i + 2^20 of each axis in 21 bits"""
    u = (np.asarray(i, dtype=np.int64) + LIMIT).astype(np.int64)
    return u[:, 0] | (u[:, 1] << 21) | (u[:, 2] << 42)


def frame_sums(i, q):
    """per distinct voxel of one frame: (keys in order of first occurrence, first row, N, Q) -- int64, exact"""
    keys = pack(i)
    uk, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    N = np.zeros(len(uk), np.int64)
    Q = np.zeros((len(uk), 3), np.int64)
    np.add.at(N, inv, 1)
    np.add.at(Q, inv, q)
    order = np.argsort(first, kind="stable")
    return uk[order], first[order], N[order], Q[order]


def centroids_of(i, Q, N, voxel=1.0, origin=(0.0, 0.0, 0.0)):
    o = np.asarray(origin, dtype=np.float64)
    return o + float(voxel) * (np.asarray(i, np.float64) + (np.asarray(Q, np.float64) / np.asarray(N, np.float64)[:, None]) / QSCALE)


class VoxelMapNP:
    def __init__(self, voxel=1.0, origin=(0.0, 0.0, 0.0)):
        self.voxel, self.origin = float(voxel), tuple(float(x) for x in origin)
        self.keys = np.zeros(0, np.int64)
        self.i = np.zeros((0, 3), np.int64)
        self.N = np.zeros(0, np.int64)
        self.Q = np.zeros((0, 3), np.int64)
        self.id_of = {}
        self.n_frames = self.last_new = self.overflow_frames = 0

    def add_frame(self, registered_scan) -> bool:
        rows, i, q, over = quantise(registered_scan, self.voxel, self.origin)
        if over:
            self.overflow_frames += 1
            return False
        keys, first, N, Q = frame_sums(i, q)
        ids = np.array([self.id_of.get(int(k), -1) for k in keys], np.int64)
        fresh = ids < 0
        base = len(self.keys)
        ids[fresh] = base + np.arange(int(fresh.sum()))   # (keys are in first-occurrence order already)
        for k, d in zip(keys[fresh].tolist(), ids[fresh].tolist()):
            self.id_of[k] = d
        self.keys = np.concatenate([self.keys, keys[fresh]])
        self.i = np.concatenate([self.i, i[first[fresh]]])
        self.N = np.concatenate([self.N, np.zeros(int(fresh.sum()), np.int64)])
        self.Q = np.concatenate([self.Q, np.zeros((int(fresh.sum()), 3), np.int64)])
        np.add.at(self.N, ids, N)
        np.add.at(self.Q, ids, Q)
        self.n_frames += 1
        self.last_new = int(fresh.sum())
        return True

    def centroids(self):
        return centroids_of(self.i, self.Q, self.N, self.voxel, self.origin)

    def box(self, lo, hi, min_count=1):
        """ids of the voxels whose centroid lies in [lo, hi] on every axis with N >= min_count, in id order"""
        c = self.centroids()
        sel = (self.N >= min_count) & (c >= np.asarray(lo, np.float64)).all(axis=1) & (c <= np.asarray(hi, np.float64)).all(axis=1)
        return np.flatnonzero(sel)

    def info(self, capacity=None):
        d = dict(n_voxels=len(self.keys), n_points=int(self.N.sum()), n_frames=self.n_frames, last_new=self.last_new,
                 capacity_voxels=capacity, overflow_frames=self.overflow_frames)
        return d
