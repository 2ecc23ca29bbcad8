"""Ray-cast HDL-64E scans of `synth_hdl64`'s street, fired as a real sweep: the sensor moves while it turns (input for the
deskew of DESIGN.md section 15).

The scanner fires azimuth column j of `n_az` (all 64 rings at once) at sweep fraction s_j = (j + 0.5) / n_az, from the pose
T_k * exp((s_j - ref) xi), where T_k is the pose the frame describes (at sweep fraction `ref`) and xi the per-frame twist
(upsilon, omega) of a constant-velocity trajectory T_{k+1} = T_k * exp(xi).  Every return is expressed in the sensor frame of
its own column's firing pose, in the ring-by-ring order of `synth_hdl64.scan`.  With zero twist every firing pose is T_k, and
`sweep_scan` draws the random numbers of `synth_hdl64.scan` in the same order: its scan equals that one bit for bit."""
from __future__ import annotations

import numpy as np

from .synth import se3_exp_np
from .synth_hdl64 import ELEV_DEG, Street, make_street


def _ground_t_rays(o, d, W: Street):
    """rays with one origin each, o (N, 3) -> distance to the sloped ground (synth_hdl64._ground_t with per-ray origins)"""
    best = np.full(len(d), np.inf)
    for q in range(4):
        a, b = W.slopes[q]
        den = d[:, 2] - a * d[:, 0] - b * d[:, 1]
        num = -W.height + a * o[:, 0] + b * o[:, 1] - o[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = num / den
        hx, hy = o[:, 0] + t * d[:, 0], o[:, 1] + t * d[:, 1]
        inq = ((hx >= 0) == (q in (0, 3))) & ((hy >= 0) == (q in (0, 1)))
        ok = (t > 0) & inq
        best = np.where(ok & (t < best), t, best)
    return best


def _box_t_rays(o, d, boxes):
    """synth_hdl64._box_t with per-ray origins o (N, 3)"""
    best = np.full(len(d), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
    for c0 in range(0, len(boxes), 16):
        B = boxes[c0:c0 + 16]
        t1 = (B[None, :, :3] - o[:, None, :]) * inv[:, None, :]
        t2 = (B[None, :, 3:] - o[:, None, :]) * inv[:, None, :]
        tmin = np.nanmax(np.minimum(t1, t2), axis=2)
        tmax = np.nanmin(np.maximum(t1, t2), axis=2)
        hit = (tmax >= tmin) & (tmax > 0)
        t = np.where(hit, np.where(tmin > 0, tmin, np.inf), np.inf)
        best = np.minimum(best, t.min(axis=1))
    return best


def sweep_scan(W: Street, pose, twist, ref=0.0, scan_period=0.1, n_az=1900, seed=0, noise=0.01, dropout=0.01, nan_inf=0,
               far_wall=False, rings=None):
    """one raw scan swept while moving: pose = T_k (map <- sensor at sweep fraction `ref`), twist = xi per frame interval.
    Returns (points (N, 3) float64 holding float32 values, sensor frame of each return's firing pose; ring ids (N,);
    times (N,) in seconds relative to T_k's instant, (s_j - ref) * scan_period; world hits (N, 3) float64, before the float32
    rounding).  Arguments otherwise as synth_hdl64.scan, whose random draws this repeats in order."""
    r = np.random.default_rng(77 + seed)
    ring_ids = np.arange(64) if rings is None else np.asarray(rings)
    el = np.deg2rad(ELEV_DEG[ring_ids])
    az = (np.arange(n_az) + 0.5) * (2 * np.pi / n_az) + r.uniform(0, 1e-4)
    E, A = np.meshgrid(el, az, indexing="ij")
    ds = np.column_stack([(np.cos(E) * np.cos(A)).ravel(), (np.cos(E) * np.sin(A)).ravel(), np.sin(E).ravel()])
    ring = np.repeat(ring_ids, n_az)
    col = np.tile(np.arange(n_az), len(ring_ids))
    # the firing pose of every column relative to T_k: D_j = exp((s_j - ref) xi)
    rel = (np.arange(n_az) + 0.5) / n_az - ref
    xi = np.asarray(twist, float).reshape(6)
    D = np.stack([se3_exp_np(s * xi) for s in rel])
    dR, dt = D[col, :3, :3], D[col, :3, 3]
    # ray directions in T_k's sensor frame, then in the world; origins in the world
    d_k = dR[:, :, 0] * ds[:, 0:1] + dR[:, :, 1] * ds[:, 1:2] + dR[:, :, 2] * ds[:, 2:3]
    R, o = pose[:3, :3], pose[:3, 3].copy()
    dw = d_k @ R.T
    o_ray = o + dt @ R.T
    t = np.minimum(_ground_t_rays(o_ray, dw, W), _box_t_rays(o_ray, dw, W.boxes))
    rad = 130.0 if far_wall else W.wall_radius   # the enclosing wall (cylinder around the sensor)
    hor = np.hypot(dw[:, 0], dw[:, 1])
    t = np.minimum(t, rad / np.maximum(hor, 1e-9))
    t = t + r.normal(0, noise, len(t))
    keep = r.uniform(size=len(t)) >= dropout
    P = (ds * t[:, None])[keep]
    hits = (o_ray + dw * t[:, None])[keep]
    ring = ring[keep]
    times = (rel * scan_period)[col[keep]]
    P = P.astype(np.float32).astype(np.float64)
    if nan_inf:
        idx = r.choice(len(P), nan_inf, replace=False)
        P[idx[: nan_inf // 2], r.integers(0, 3)] = np.nan
        P[idx[nan_inf // 2:], r.integers(0, 3)] = np.inf
    return np.ascontiguousarray(P), ring, np.ascontiguousarray(times), np.ascontiguousarray(hits)


def trajectory(n_frames, twist, init=None, rest_frames=0):
    """T_0 = init (identity), T_{k+1} = T_k * exp(twist): a constant per-frame twist (upsilon, omega) in the sensor frame;
    the first `rest_frames` frames stand still at T_0 and the motion starts after them"""
    step = se3_exp_np(np.asarray(twist, float))
    T = np.eye(4) if init is None else np.asarray(init, float).copy()
    poses = []
    for k in range(n_frames):
        if k >= max(rest_frames, 1):
            T = T @ step
        poses.append(T.copy())
    return poses


def sequence(n_frames, twist, seed=0, ref=0.0, scan_period=0.1, rest_frames=0, **kw):
    """consecutive swept scans along one constant-twist trajectory through synth_hdl64's street `seed` (the first
    `rest_frames` frames at rest, swept without motion): (scans, times, poses, hits)"""
    W = make_street(seed)
    poses = trajectory(n_frames, twist, rest_frames=rest_frames)
    zero = np.zeros(6)
    out = [sweep_scan(W, T, zero if f < rest_frames else twist, ref=ref, scan_period=scan_period, seed=seed * 1000 + f, **kw)
           for f, T in enumerate(poses)]
    return [o[0] for o in out], [o[2] for o in out], poses, [o[3] for o in out]
