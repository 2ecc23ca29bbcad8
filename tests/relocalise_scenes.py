"""The scene the relocalisation's tests share: the static pass of tests/carve_scenes.py with every
keyframe's thinned scan as its place-recognition scan, and the new scan of tests/localise_scenes.py as it is and turned about the
sensor's z."""
from __future__ import annotations

import math

import numpy as np

import carve_scenes as CS
import localise_scenes as LS
import place_np as PN

PLACE = dict(exclude_recent=8)                 # the database's configuration (the rest: the defaults, 20 rings x 60 sectors)
OFF_GRID = 0.4                                 # rad: 3.82 sectors
# name -> (the turn of the sensor about its z, the shifts the turn predicts beside the untouched query's)
TURNS = {"as_it_is": (0.0, (0,)), "quarter": (0.5 * math.pi, (15,)), "half": (math.pi, (30,)), "off_grid": (OFF_GRID, (3, 4))}


def turned(scan, truth, name):
    """the scan a sensor turned by the angle about its own z would have taken -> (scan, its true pose).  The quarter and the
    half turn move coordinates and flip signs, nothing is rounded"""
    a = TURNS[name][0]
    x, y, z = scan[:, 0], scan[:, 1], scan[:, 2]
    if name == "as_it_is":
        pts, R = scan.copy(), np.eye(3)
    elif name == "quarter":
        pts, R = np.stack([y, -x, z], axis=1), np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    elif name == "half":
        pts, R = np.stack([-x, -y, z], axis=1), np.diag([-1.0, -1.0, 1.0])
    else:
        R = LS.rotation([0.0, 0.0, 1.0], a)
        pts = scan @ R                          # R^T p, row by row
    pose = np.array(truth, np.float64)
    pose[:3, :3] = pose[:3, :3] @ R
    return np.ascontiguousarray(pts), pose


def static():
    """-> (poses, clouds, keyframe scans, {name: (query, its true pose)})"""
    poses, clouds = CS.static_pass()
    scan, truth = LS.static_scan(poses)
    return poses, clouds, [c[1][0] for c in clouds], {name: turned(scan, truth, name) for name in TURNS}


def foreign():
    """a scan of a different world: the corner's scan (tests/localise_scenes.py) against the street's map.  (Another street of
    the generator shares the ground and the facades' layout with this one: its scan finds two thirds of its points a surfel.)"""
    return LS.corner()[2]


def database(scans):
    """the restated keyframe database of the scans -> (ring keys, descriptors)"""
    pc = PN.cfg_of(**PLACE)
    rk, ds = [], []
    for s in scans:
        d, r, _ = PN.describe(s, **{k: pc[k] for k in ("n_rings", "n_sectors", "max_radius", "height_offset")})
        ds.append(d); rk.append(r)
    return rk, ds
