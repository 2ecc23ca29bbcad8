"""Ray-cast HDL-64E scans of one synthetic street (the `synth_world` idea, as raw returns): input for the segmentation
stage (`tloam_segment`) and for `replay(..., segmenter="device")`.

The world: a ground of four planes with a gentle slope each (one per world quadrant), building fronts along both sides
of the road with gaps, poles, box-shaped cars, small clutter boxes, and an enclosing wall far out so that every beam
returns.  The scanner has 64 rings at the elevations `initSections` assumes (-24.9 deg + 0.4 deg per ring, +1.7 deg from
ring 31 on) and fires every ring as one counter-clockwise sweep that starts just past azimuth 0: consecutive rings meet at
a quadrant 4 -> quadrant 1 step, which is how the reference recovers the ring ids.  Ranges get Gaussian noise, a few
returns drop out, and the points are rounded to float32 like the KITTI files / the ROS wire.  Options: an enclosing wall
beyond 120 m (returns the DCVC stage keeps at polar (0, 0, 0)), and NaN / Inf injections."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

ELEV_DEG = np.array([-24.9 + 0.4 * i + (1.7 if i >= 31 else 0.0) for i in range(64)])


@dataclass
class Street:
    boxes: np.ndarray      # (B, 6): lo xyz, hi xyz (world)
    slopes: np.ndarray     # (4, 2): ground dz/dx, dz/dy per world quadrant
    wall_radius: float
    height: float = 1.73


def make_street(seed=0, length=200.0, wall_radius=90.0) -> Street:
    r = np.random.default_rng(4200 + seed)
    boxes = []
    for side in (-1.0, 1.0):                                  # building fronts with gaps
        x = -60.0
        while x < length:
            w = r.uniform(8.0, 20.0)
            if r.uniform() > 0.25:
                y0 = side * r.uniform(10.0, 14.0)
                depth = r.uniform(5.0, 12.0)
                lo_y, hi_y = (y0, y0 + depth) if side > 0 else (y0 - depth, y0)
                boxes.append([x, lo_y, -3.0, x + w, hi_y, r.uniform(4.0, 12.0)])
            x += w + r.uniform(1.0, 6.0)
    for _ in range(int(length / 6)):                          # poles
        px, py = r.uniform(-50, length), r.choice([-1.0, 1.0]) * r.uniform(6.0, 9.0)
        s = r.uniform(0.12, 0.3)
        boxes.append([px - s, py - s, -3.0, px + s, py + s, r.uniform(2.5, 6.0)])
    for _ in range(int(length / 8)):                          # parked / moving cars
        cx, cy = r.uniform(-50, length), r.choice([-1.0, 1.0]) * r.uniform(3.5, 7.0)
        L, W = r.uniform(3.8, 4.8), r.uniform(1.6, 1.9)
        boxes.append([cx - L / 2, cy - W / 2, -2.0, cx + L / 2, cy + W / 2, -1.73 + r.uniform(1.3, 1.7)])
    for _ in range(int(length / 4)):                          # clutter
        cx, cy = r.uniform(-50, length), r.uniform(-25, 25)
        if abs(cy) < 3.0:
            continue
        s = r.uniform(0.2, 0.8)
        boxes.append([cx - s, cy - s, -2.0, cx + s, cy + s, -1.73 + r.uniform(0.3, 1.5)])
    slopes = r.uniform(-0.015, 0.015, (4, 2))
    return Street(np.asarray(boxes, float), slopes, float(wall_radius))


def trajectory(n_frames, step=1.2, yaw_rate=0.01, seed=0):
    """map <- sensor poses along the road (4x4)"""
    poses, x, y, yaw = [], 0.0, 0.0, 0.0
    for _ in range(n_frames):
        T = np.eye(4)
        c, s = np.cos(yaw), np.sin(yaw)
        T[:2, :2] = [[c, -s], [s, c]]
        T[:3, 3] = [x, y, 0.0]
        poses.append(T)
        x += step * c; y += step * s; yaw += yaw_rate
    return poses


def _ground_t(o, d, W: Street):
    """ray -> distance to the sloped ground (the plane of the world quadrant the hit lands in)"""
    best = np.full(len(d), np.inf)
    for q in range(4):
        a, b = W.slopes[q]
        # z = -h + a x + b y ;  o_z + t d_z = -h + a (o_x + t d_x) + b (o_y + t d_y)
        den = d[:, 2] - a * d[:, 0] - b * d[:, 1]
        num = -W.height + a * o[0] + b * o[1] - o[2]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = num / den
        hx, hy = o[0] + t * d[:, 0], o[1] + t * d[:, 1]
        inq = ((hx >= 0) == (q in (0, 3))) & ((hy >= 0) == (q in (0, 1)))
        ok = (t > 0) & inq
        best = np.where(ok & (t < best), t, best)
    return best


def _box_t(o, d, boxes):
    best = np.full(len(d), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
    for c0 in range(0, len(boxes), 16):
        B = boxes[c0:c0 + 16]
        t1 = (B[None, :, :3] - o[None, None, :]) * inv[:, None, :]
        t2 = (B[None, :, 3:] - o[None, None, :]) * inv[:, None, :]
        tmin = np.nanmax(np.minimum(t1, t2), axis=2)
        tmax = np.nanmin(np.maximum(t1, t2), axis=2)
        hit = (tmax >= tmin) & (tmax > 0)
        t = np.where(hit, np.where(tmin > 0, tmin, np.inf), np.inf)
        best = np.minimum(best, t.min(axis=1))
    return best


def scan(W: Street, pose, n_az=1900, seed=0, noise=0.01, dropout=0.01, nan_inf=0, far_wall=False, rings=None):
    """one raw scan at `pose` (map <- sensor): (N, 3) float64 holding float32 values, in firing order (ring by ring), and
    the ring id of every return.  rings: fire only these rings (default all 64)"""
    r = np.random.default_rng(77 + seed)
    ring_ids = np.arange(64) if rings is None else np.asarray(rings)
    el = np.deg2rad(ELEV_DEG[ring_ids])
    az = (np.arange(n_az) + 0.5) * (2 * np.pi / n_az) + r.uniform(0, 1e-4)
    E, A = np.meshgrid(el, az, indexing="ij")
    ds = np.column_stack([(np.cos(E) * np.cos(A)).ravel(), (np.cos(E) * np.sin(A)).ravel(), np.sin(E).ravel()])
    ring = np.repeat(ring_ids, n_az)
    R, o = pose[:3, :3], pose[:3, 3].copy()
    dw = ds @ R.T
    t = np.minimum(_ground_t(o, dw, W), _box_t(o, dw, W.boxes))
    # the enclosing wall (cylinder around the sensor)
    rad = 130.0 if far_wall else W.wall_radius
    hor = np.hypot(dw[:, 0], dw[:, 1])
    t = np.minimum(t, rad / np.maximum(hor, 1e-9))
    t = t + r.normal(0, noise, len(t))
    keep = r.uniform(size=len(t)) >= dropout
    P = (ds * t[:, None])[keep]
    ring = ring[keep]
    P = P.astype(np.float32).astype(np.float64)
    if nan_inf:
        idx = r.choice(len(P), nan_inf, replace=False)
        P[idx[: nan_inf // 2], r.integers(0, 3)] = np.nan
        P[idx[nan_inf // 2:], r.integers(0, 3)] = np.inf
    return np.ascontiguousarray(P), ring


def sequence(n_frames, seed=0, **kw):
    """consecutive scans along one trajectory through one street: (scans, poses)"""
    W = make_street(seed)
    poses = trajectory(n_frames, seed=seed)
    return [scan(W, T, seed=seed * 1000 + f, **kw)[0] for f, T in enumerate(poses)], poses
