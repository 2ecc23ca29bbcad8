"""Scenes the extension's tests share: the ghost scene's wall, six poses and 1 m box (carve_scenes.py), with
the wall points the box shadows taken out of every keyframe that sees the box, cut after keyframe 3 into a base and an extension.
  removed    the box stands in keyframes 0 to 2 and is gone in 3 to 5: the extension's rays pass through where it stood
  appeared   the box stands in keyframes 3 to 5 only: the base's rays passed through where it now stands, before it existed
Target slot 0 alone (cloud_mask 0x10), voxel 0.5 m, rays up to 12 m: carve_scenes.GHOST."""
from __future__ import annotations

import numpy as np

import carve_scenes as CS

CUT = 3
BOX_LO, BOX_HI = np.array([5.5, 2.0, 1.0]), np.array([6.5, 3.0, 2.0])


def shadowed(O, pts):
    """the points whose segment from O meets the box (slab test, closed)"""
    D = pts - O
    with np.errstate(all="ignore"):
        t1, t2 = (BOX_LO - O) / D, (BOX_HI - O) / D
    lo, hi = np.fmin(t1, t2), np.fmax(t1, t2)
    par = D == 0.0
    inside = (O >= BOX_LO) & (O <= BOX_HI)
    lo = np.where(par, np.where(inside, -np.inf, np.inf), lo)
    hi = np.where(par, np.where(inside, np.inf, -np.inf), hi)
    return np.maximum(lo.max(axis=1), 0.0) <= np.minimum(hi.min(axis=1), 1.0)


def scene(box_keyframes):
    """-> (poses (6, 4, 4), clouds, wall points, box points; the last two in the world)"""
    wall = CS.grid((0.0, 5.0, 0.5), (12.0, 5.0, 3.5))
    box = CS.grid(tuple(BOX_LO), tuple(BOX_HI))
    poses, clouds = [], []
    for k in range(6):
        P = np.eye(4)
        P[:3, 3] = [2.0 * k, 0.0, 1.5]
        seen = wall[np.linalg.norm(wall - P[:3, 3], axis=1) <= 12.0]
        if k in box_keyframes:
            seen = np.concatenate([seen[~shadowed(P[:3, 3], seen)], box])
        poses.append(P)
        clouds.append(CS.slot0(seen - P[:3, 3]))
    return np.array(poses), clouds, wall, box


def removed():
    return scene((0, 1, 2))


def appeared():
    return scene((3, 4, 5))


def cells(points, voxel):
    return {tuple(c) for c in np.floor(np.asarray(points) / voxel).astype(np.int64).tolist()}
