"""Host-side helpers around the closed map's ray-cast (Registration.closed_map_raycast): a lidar's firing
pattern as segment ends, and a measured scan checked ray by ray against what the map predicts.  Nothing here runs on the
device; the casts go through the handle that is passed in."""
from __future__ import annotations

import numpy as np

RAYCAST_SKIPPED, RAYCAST_MISS, RAYCAST_HIT_CENTROID, RAYCAST_HIT_PLANE = 0, 1, 2, 3


def lidar_pattern(rings, n_az, elev_lo, elev_hi, length):
    """Segment ends (rings * n_az, 3) in the sensor frame, ring-major: ring r at elevation elev_lo + r * (elev_hi - elev_lo) /
    (rings - 1) (radians; elev_lo alone when rings == 1), azimuth 2 pi k / n_az, each `length` long."""
    rings, n_az = int(rings), int(n_az)
    if rings < 1 or n_az < 1:
        raise ValueError("rings and n_az are at least 1")
    el = np.linspace(float(elev_lo), float(elev_hi), rings) if rings > 1 else np.array([float(elev_lo)])
    az = 2.0 * np.pi * np.arange(n_az) / n_az
    ce, se = np.cos(el)[:, None], np.sin(el)[:, None]
    d = np.stack([ce * np.cos(az)[None, :], ce * np.sin(az)[None, :], se * np.ones((1, n_az))], axis=-1)
    return np.ascontiguousarray((float(length) * d).reshape(-1, 3))


def scan_check(H, points, pose, extend=2.0):
    """The measured scan `points` (n, 3; sensor frame) at `pose` against the map: each ray is cast along its point out to
    |p| + extend, so that a surface a little behind the measured one is still found.
    -> (status (n,) uint8, predicted - measured range (n,) float64, NaN where the cast has no hit or |p| is 0 or not finite)"""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        r = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
        ends = p * ((r + float(extend)) / r)[:, None]
    status, ranges = H.closed_map_raycast(ends, pose)[:2]
    status, ranges = np.asarray(status), np.asarray(ranges)
    hit = status >= RAYCAST_HIT_CENTROID
    return status, np.where(hit, ranges - r, np.nan)
