"""Scenes the carve's tests share: the ghost scene and the static out-and-back pass.  Keyframe clouds are
[four source clouds, four target clouds]; these scenes use target slot 0 alone (cloud_mask 0x10)."""
from __future__ import annotations

import numpy as np

from tloam_amd import synth_hdl64 as G
from tloam_amd import synth_revisit as RV

MASK = 0x10
NONE = np.zeros((0, 3))

# the ghost scene: a wall every keyframe sees, a box only keyframe 1 sees
GHOST = dict(voxel=0.5, max_range=12.0)
GHOST_BOX_KEYFRAME = 1

# the static pass: the first keyframes of tests/test_gpu_closed_map.py's out-and-back run, each thinned scan its keyframe's cloud
STATIC = dict(voxel=0.5, max_range=20.0)
STATIC_KEYFRAMES = 8
THIN = dict(n_az=600, rings=np.arange(0, 64, 2))


def slot0(cloud):
    return [[NONE] * 4, [np.ascontiguousarray(cloud, np.float64), NONE, NONE, NONE]]


def grid(lo, hi, spacing=0.2):
    axes = [lo[a] + spacing * np.arange(int(round((hi[a] - lo[a]) / spacing)) + 1) for a in range(3)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)


def ghost_scene():
    """-> (poses (6, 4, 4), clouds, wall points, box points; the last two in the world).  A vertical wall at y = 5, x in [0, 12],
    z in [0.5, 3.5], 0.2 m spacing; six keyframes at (2 k, 0, 1.5), identity rotation, each seeing the wall points within 12 m;
    a 1 x 1 x 1 m box of points centred at (6, 2.5, 1.5), in keyframe 1 only."""
    wall = grid((0.0, 5.0, 0.5), (12.0, 5.0, 3.5))
    box = grid((5.5, 2.0, 1.0), (6.5, 3.0, 2.0))
    poses, clouds = [], []
    for k in range(6):
        P = np.eye(4)
        P[:3, 3] = [2.0 * k, 0.0, 1.5]
        seen = wall[np.linalg.norm(wall - P[:3, 3], axis=1) <= 12.0]
        if k == GHOST_BOX_KEYFRAME:
            seen = np.concatenate([seen, box])
        poses.append(P)
        clouds.append(slot0(seen - P[:3, 3]))
    return np.array(poses), clouds, wall, box


def static_pass(keyframes=STATIC_KEYFRAMES):
    """-> (poses, clouds) of the first keyframes of the out-and-back pass (16 out, seed 1, thinned scans): nothing in it moves"""
    W = G.make_street(1)
    poses, _ = RV.out_and_back_poses(16, seed=1)
    poses = poses[:keyframes]
    return np.array(poses), [slot0(G.scan(W, T, seed=1000 + f, **THIN)[0]) for f, T in enumerate(poses)]
