"""Sequences through `synth_hdl64`'s street with their true poses, for the place recognition of DESIGN.md section 16.

`out_and_back`: the sensor drives out along the street in the lane y = -lane / 2, turns in place at the far end, and drives
back over the same stretch in the lane y = +lane / 2, its positions offset by half a step along the street from the outbound
ones: every return position lies within sqrt(lane^2 + (step / 2)^2) of an outbound one, with a heading about pi away (a small
deterministic wobble keeps the headings off the exact sector grid).  `one_way`: the outbound leg alone, over as many frames,
which revisits nothing.  Scans are `synth_hdl64.scan`'s, so the same keywords thin them (`n_az`, `rings`)."""
from __future__ import annotations

import numpy as np

from .synth_hdl64 import make_street, scan


def _pose(x, y, yaw):
    T = np.eye(4)
    c, s = np.cos(yaw), np.sin(yaw)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = [x, y, 0.0]
    return T


def out_and_back_poses(n_out, step=2.0, lane=0.8, x0=0.0, wobble=0.02, seed=0):
    """2 n_out poses (map <- sensor): n_out outbound (heading ~0), then n_out back (heading ~pi); `leg` marks 0 / 1"""
    r = np.random.default_rng(900 + seed)
    poses, leg = [], []
    for k in range(n_out):
        poses.append(_pose(x0 + k * step, -lane / 2, r.uniform(-wobble, wobble)))
        leg.append(0)
    for k in range(n_out):
        x = x0 + (n_out - 1 - k) * step - step / 2
        poses.append(_pose(x, lane / 2, np.pi + r.uniform(-wobble, wobble)))
        leg.append(1)
    return poses, np.array(leg)


def one_way_poses(n, step=2.0, lane=0.8, x0=0.0, wobble=0.02, seed=0):
    r = np.random.default_rng(900 + seed)
    return [_pose(x0 + k * step, -lane / 2, r.uniform(-wobble, wobble)) for k in range(n)]


def out_and_back(n_out, seed=0, step=2.0, lane=0.8, **scan_kw):
    """(scans, poses, leg) of an out-and-back pass through street `seed`"""
    W = make_street(seed)
    poses, leg = out_and_back_poses(n_out, step, lane, seed=seed)
    return [scan(W, T, seed=seed * 1000 + f, **scan_kw)[0] for f, T in enumerate(poses)], poses, leg


def one_way(n, seed=0, step=2.0, lane=0.8, **scan_kw):
    """(scans, poses) of a one-way pass through street `seed`"""
    W = make_street(seed)
    poses = one_way_poses(n, step, lane, seed=seed)
    return [scan(W, T, seed=seed * 1000 + f, **scan_kw)[0] for f, T in enumerate(poses)], poses


def relative_yaw(A, B):
    """the heading of A relative to B's, in (-pi, pi]"""
    ya, yb = np.arctan2(A[1, 0], A[0, 0]), np.arctan2(B[1, 0], B[0, 0])
    d = (ya - yb) % (2 * np.pi)
    return d - 2 * np.pi if d > np.pi else d
