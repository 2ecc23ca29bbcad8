"""What the ray-cast's tests share, beside tests/localise_scenes.py's wall and tests/diff_scenes.py's
sensors: the firing pattern, and the analytic ranges of that pattern against the wall y = 5, x in [0, 12], z in [0.5, 3.5]."""
from __future__ import annotations

import numpy as np

from tloam_amd import raycast as RC

LENGTH = 11.0
WALL_Y, WALL_X, WALL_Z = 5.0, (0.0, 12.0), (0.5, 3.5)
INSET, GROWN = 0.3, 0.8


def pattern():
    return RC.lidar_pattern(16, 180, -0.3, 0.3, LENGTH)


def wall_ranges(sensor, ends=None):
    """the pattern's rays from `sensor` (identity rotation) against the wall's plane -> (range to the plane (n,), +inf where the
    ray does not run towards it; on_wall (n,) bool: the hit lies at least INSET inside the wall's outline and within LENGTH;
    off_wall (n,) bool: the ray's line misses the outline grown by GROWN)"""
    ends = pattern() if ends is None else np.asarray(ends, np.float64)
    O = np.asarray(sensor, np.float64)
    L = np.sqrt((ends * ends).sum(axis=1))
    d = ends / L[:, None]
    with np.errstate(all="ignore"):
        t = np.where(d[:, 1] > 0.0, (WALL_Y - O[1]) / d[:, 1], np.inf)
        x, z = O[0] + t * d[:, 0], O[2] + t * d[:, 2]
    towards = np.isfinite(t)
    on = towards & (t <= LENGTH) & (x >= WALL_X[0] + INSET) & (x <= WALL_X[1] - INSET) & (z >= WALL_Z[0] + INSET) & \
        (z <= WALL_Z[1] - INSET)
    with np.errstate(invalid="ignore"):
        within = towards & (x >= WALL_X[0] - GROWN) & (x <= WALL_X[1] + GROWN) & (z >= WALL_Z[0] - GROWN) & (z <= WALL_Z[1] + GROWN)
    return t, on, ~within
