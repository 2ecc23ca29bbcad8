"""Scenes the diff's tests share, beside tests/carve_scenes.py's and tests/localise_scenes.py's: a box the
map holds and the scan does not (gone), a box the scan holds and the map does not (appeared), and the ghost scene's box, which
the map holds as a ghost the carve has seen through (the gate).  Every scan is taken with identity rotation from a sensor
position, so its pose is a translation."""
from __future__ import annotations

import numpy as np

import carve_scenes as CS
import localise_scenes as LS

VOXEL = CS.GHOST["voxel"]
MAX_RANGE = CS.GHOST["max_range"]
SENSORS = ((6.0, 0.0, 1.5), (5.0, 0.0, 1.5), (7.0, -1.0, 1.2))
BOX_LO, BOX_HI = (5.5, 2.0, 1.0), (6.5, 3.0, 2.0)


def pose_at(sensor):
    P = np.eye(4)
    P[:3, 3] = sensor
    return P


def scan_from(world, sensor):
    return np.ascontiguousarray(np.asarray(world, np.float64) - np.asarray(sensor, np.float64))


def gone(sensor=SENSORS[0]):
    """the map: the ghost scene's wall and its box, the box in all six keyframes; the scan: the wall alone
    -> (poses, clouds, scan, pose)"""
    poses, _, wall, box = CS.ghost_scene()
    clouds = []
    for P in poses:
        seen = np.concatenate([wall[np.linalg.norm(wall - P[:3, 3], axis=1) <= MAX_RANGE], box])
        clouds.append(CS.slot0(seen - P[:3, 3]))
    return poses, clouds, scan_from(wall, sensor), pose_at(sensor)


def appeared(sensor=SENSORS[0]):
    """the map: the wall alone (localise_scenes.wall); the scan: wall plus box
    -> (poses, clouds, scan, pose, is_box (n,) bool)"""
    poses, clouds, _, _ = LS.wall()
    _, _, wall, box = CS.ghost_scene()
    is_box = np.arange(len(wall) + len(box)) >= len(wall)
    return poses, clouds, scan_from(np.concatenate([wall, box]), sensor), pose_at(sensor), is_box


def ghost_gate(sensor=SENSORS[0]):
    """the map: the ghost scene's wall and a box keyframe 1 alone sees, to be carved at CS.GHOST's max_range; the scan: wall plus
    box -> (poses, clouds, scan, pose, is_box).  The box is not CS.ghost_scene()'s: that one's upper faces lie on cell borders and
    leave thin slabs of points, which are planes the localiser's gate takes, so that box points on them are SURFACE with the gate
    off.  This box is 4 x 4 x 4 points at 0.25 m from (5.5, 2.0, 1.0): each of its eight voxels holds a 2 x 2 x 2 cube of points,
    which has no plane, and the ghost voxels explain its points as OCCUPIED and nothing else"""
    poses, clouds, wall, _ = CS.ghost_scene()
    box = CS.grid((5.5, 2.0, 1.0), (6.25, 2.75, 1.75), 0.25)
    k = CS.GHOST_BOX_KEYFRAME
    seen = np.concatenate([wall[np.linalg.norm(wall - poses[k][:3, 3], axis=1) <= MAX_RANGE], box])
    clouds[k] = CS.slot0(seen - poses[k][:3, 3])
    is_box = np.arange(len(wall) + len(box)) >= len(wall)
    return poses, clouds, scan_from(np.concatenate([wall, box]), sensor), pose_at(sensor), is_box


def box_voxels(V):
    """ids of the voxels whose centroid lies in the box"""
    return V.box(BOX_LO, BOX_HI)
