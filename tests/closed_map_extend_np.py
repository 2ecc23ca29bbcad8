"""The closed map's extension (tl_extend.hip, tl_api_extend.hip) restated in numpy.  It composes the
restatements that exist and copies none of them: the rows are VoxelMapNP.add_frame per new keyframe (closed_map_carve_np's
transform and concatenation), the surfels closed_map_surfel_np.moments of the new keyframes added to the sums and .solve of the
result, the carve closed_map_carve_np.carve of the map AS EXTENDED over the new keyframes alone, added to the old counts:

    M_ext = [M_before, 0 ...] + carve(V_ext, new keyframes only)

ExtendedMapNP holds the map a context holds: build() is sections 19, 21 and 22 over its first keyframes, extend() this section
over later ones."""
from __future__ import annotations

import numpy as np

import closed_map_carve_np as CN
import closed_map_surfel_np as SN
import voxel_map_np as VN


def add_keyframes(V, poses, clouds, mask):
    """the build's rule for each keyframe, in place -> dict(added, empty, overflow, points, new_voxels, touched_voxels)"""
    d = dict(added_keyframes=0, empty_keyframes=0, overflow_keyframes=0, points=0, new_voxels=0, touched_voxels=0)
    before_keys, before_N = len(V.keys), V.N.copy()
    for P, c in zip(poses, clouds):
        cat = CN.concatenation(c, mask)
        if not len(cat):
            d["empty_keyframes"] += 1
        elif V.add_frame(CN.transform(P, cat)):
            d["added_keyframes"] += 1
        else:
            d["overflow_keyframes"] += 1
    d["new_voxels"] = len(V.keys) - before_keys
    d["points"] = int(V.N.sum() - before_N.sum())
    d["touched_voxels"] = d["new_voxels"] + int((V.N[:before_keys] != before_N).sum())
    return d


class ExtendedMapNP:
    def __init__(self, mask, voxel=1.0, origin=(0.0, 0.0, 0.0), surfels=False, carve=None, ray_mask=0, min_points=5):
        """carve: None (not carved) or the carve's max_range / end_margin / radius"""
        self.mask, self.ray_mask, self.min_points = mask, ray_mask or mask, min_points
        self.V = VN.VoxelMapNP(voxel, origin)
        self.S = np.zeros((0, SN.SUMS), np.int64) if surfels else None
        self.carve_cfg = carve
        self.M = np.zeros(0, np.int64) if carve is not None else None
        self.poses = np.zeros((0, 4, 4))
        self.orphans = 0
        self.carve_info = dict(n_keyframes=0, n_rays=0, skipped_rays=0, steps=0, tested=0, misses=0, voxels_missed=0)

    def extend(self, poses, clouds):
        """the keyframes (poses[k], clouds[k]) added -> the extend info without first_keyframe, grown and launches"""
        poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
        V = self.V
        nv0 = len(V.keys)
        info = add_keyframes(V, poses, clouds, self.mask)
        info["n_keyframes"] = len(poses)
        fresh = len(V.keys) - nv0
        info.update(rays=0, skipped_rays=0, steps=0, tested=0, misses=0, solved_voxels=0)
        if self.S is not None:
            add, orphans = SN.moments(V, poses, clouds, self.mask)
            self.S = np.concatenate([self.S, np.zeros((fresh, SN.SUMS), np.int64)]) + add
            self.orphans += orphans
            info["solved_voxels"] = int((self.S[:, 0] >= self.min_points).sum())
        if self.M is not None:
            add, c = CN.carve(V, poses, clouds, self.ray_mask, **self.carve_cfg)
            self.M = np.concatenate([self.M, np.zeros(fresh, np.int64)]) + add
            for k in ("n_rays", "skipped_rays", "steps", "tested"):
                self.carve_info[k] += c[k]
            self.carve_info.update(misses=int(self.M.sum()), voxels_missed=int((self.M > 0).sum()))
            info.update(rays=c["n_rays"], skipped_rays=c["skipped_rays"], steps=c["steps"], tested=c["tested"], misses=c["misses"])
        self.poses = np.concatenate([self.poses, poses])
        self.carve_info["n_keyframes"] = len(self.poses)
        return info

    build = extend   # (from nothing, an extension is the build, the full surfel pass and the full carve)

    def surfels(self):
        """-> (sums, normals, variances, the surfel info without `launches`)"""
        normals, evals, solved = SN.solve(self.S, self.V.voxel, self.min_points)
        info = dict(n_keyframes=len(self.poses), n_points=int(self.S[:, 0].sum()), orphan_points=self.orphans,
                    solved_voxels=int(solved.sum()))
        return self.S, normals, evals, info
