"""Scenes the localisation's tests share, beside tests/carve_scenes.py's: the corner, the ghost scene
without its box (a single wall), the new scan of the static pass, and the offsets a prior starts from."""
from __future__ import annotations

import numpy as np

import carve_scenes as CS
import closed_map_carve_np as CN
import closed_map_localise_np as LN
import closed_map_surfel_np as SN
from tloam_amd import synth_hdl64 as G

CORNER = dict(voxel=0.5)
STARTS = ((0.3, 0.02), (0.6, 0.05), (1.0, 0.05), (1.5, 0.1))   # metres, radians off the generator's pose
CORNER_START = (0.2, 0.03)
SCAN_SEED = 77
T_DIR = np.array([0.6, -0.64, 0.48])
R_AXIS = np.array([0.36, -0.48, 0.8])


def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def offset(pose, metres, radians):
    """`pose` moved by `metres` along T_DIR and turned by `radians` about R_AXIS"""
    P = np.array(pose, np.float64)
    P[:3, :3] = rotation(R_AXIS, radians) @ P[:3, :3]
    P[:3, 3] += metres * T_DIR
    return P


def corner_planes():
    """three point grids at 0.2 m spacing on the grid planes x = 0, y = 0 and z = 0, each 4 x 4 m and 0.6 m clear of the other
    two planes, so that no voxel holds points of two of them"""
    a = 0.6 + 0.2 * np.arange(21)
    u, w = [m.ravel() for m in np.meshgrid(a, a, indexing="ij")]
    z = np.zeros(len(u))
    return np.concatenate([np.stack([z, u, w], axis=1), np.stack([u, z, w], axis=1), np.stack([u, w, z], axis=1)])


def corner():
    """-> (poses (2, 4, 4), clouds, scan, the scan's true pose).  The keyframes stand inside the corner with identity rotation
    and dyadic translations, so that the planes' own coordinate comes back as an exact 0; the scan is the same points seen
    from a third, turned pose"""
    world = corner_planes()
    poses, clouds = [], []
    for t in ([2.0, 2.5, 1.5], [2.75, 1.5, 2.25]):
        P = np.eye(4)
        P[:3, 3] = t
        poses.append(P)
        clouds.append(CS.slot0(world - P[:3, 3]))
    truth = np.eye(4)
    truth[:3, :3] = rotation([0.2, -0.3, 0.9], 0.4)
    truth[:3, 3] = [1.7, 2.2, 1.9]
    scan = (world - truth[:3, 3]) @ truth[:3, :3]
    return np.array(poses), clouds, np.ascontiguousarray(scan), truth


def wall():
    """the ghost scene without its box: a single wall -> (poses, clouds, scan, the scan's true pose)"""
    poses, clouds, wall_pts, _ = CS.ghost_scene()
    k = CS.GHOST_BOX_KEYFRAME
    seen = wall_pts[np.linalg.norm(wall_pts - poses[k][:3, 3], axis=1) <= 12.0]
    clouds[k] = CS.slot0(seen - poses[k][:3, 3])
    truth = np.eye(4)
    truth[:3, 3] = [5.0, 0.5, 1.25]
    return poses, clouds, np.ascontiguousarray(wall_pts - truth[:3, 3]), truth


def midway(A, B):
    """the pose half-way between two poses of the pass (translation and yaw averaged)"""
    P = np.eye(4)
    ya, yb = np.arctan2(A[1, 0], A[0, 0]), np.arctan2(B[1, 0], B[0, 0])
    P[:3, :3] = rotation([0.0, 0.0, 1.0], 0.5 * (ya + yb))
    P[:3, 3] = 0.5 * (A[:3, 3] + B[:3, 3])
    return P


def static_scan(poses, seed=SCAN_SEED):
    """a new thinned scan of the static pass's street, taken midway between keyframes 3 and 4 -> (scan, its true pose)"""
    truth = midway(np.asarray(poses[3]), np.asarray(poses[4]))
    return G.scan(G.make_street(1), truth, seed=seed, **CS.THIN)[0], truth


def target(poses, clouds, mask, voxel, origin=(0.0, 0.0, 0.0), min_points=5, **gate):
    """the restated map, its surfels and the localisation's view of them -> (V, S, normals, evals, Target)"""
    V = CN.build_map(poses, clouds, mask, voxel, origin)
    S, normals, evals, _ = SN.surfels(V, poses, clouds, mask, min_points)
    return V, S, normals, evals, LN.Target(V, S, normals, evals, min_points, **gate)
