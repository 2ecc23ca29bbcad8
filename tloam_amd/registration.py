"""Host-side mirror of the reference's registration plugin, bound to the C ABI (include/tloam_hip.h).

`HipRegistration` follows tloam::RegistrationInterface
(include/tloam/models/registration/registration_interface.hpp:40-48):

    setInputSource(Frame&)            -> set_input_source(frame)
    setInputTarget(Frame&)            -> set_input_target(frame)
    scanMatching(out, predict, pose)  -> scan_matching(predict, ...)  -> (ok, result_pose)
    getFitnessScore()                 -> get_fitness_score()

and is selected the way FrontEnd::initRegistraton selects "TLS" (front_end.cpp:155-167): see
`make_registration("TLS_HIP", cfg)`.  All computation happens in libtloam_hip.so (hand-written HIP
kernels for gfx950); this module only marshals numpy arrays into the C ABI through ctypes.  There is
no CPU fallback: a missing library or a missing GPU raises.
"""
from __future__ import annotations

import ctypes as C
import sys
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TLOAM_HIP_LIB") or os.path.join(_HERE, "libtloam_hip.so")  # env override: tuning builds only

KIND_PLANAR, KIND_GROUND, KIND_EDGE, KIND_SPHERE = 0, 1, 2, 3
RES_PLANE, RES_LINE, RES_POINT = 0, 1, 2

STATUS = {0: "TLOAM_OK", -1: "TLOAM_E_INVALID", -2: "TLOAM_E_TOO_FEW_POINTS", -3: "TLOAM_E_BAD_POSE",
          -4: "TLOAM_E_HIP", -5: "TLOAM_E_RCCL", -6: "TLOAM_E_NOT_READY", -7: "TLOAM_E_WEIGHT_RANGE"}


class SubmapConfig(C.Structure):
    """tloam_submap_config: the submap keys of config/mapping/lidar_odometry.yaml:6-17."""
    _fields_ = [("planar_frame_size", C.c_int32), ("sphere_frame_size", C.c_int32),
                ("edge_crop_box_length", C.c_double), ("ground_crop_box_length", C.c_double),
                ("edge_down_sample_submap", C.c_double), ("ground_down_sample_submap", C.c_double),
                ("ground_down_sample", C.c_double)]


class FeatureConfig(C.Structure):
    """tloam_feature_config: the `feature:` block of config/mapping/feature.yaml."""
    _fields_ = [("radius", C.c_double), ("K", C.c_int32), ("min_neigh", C.c_int32), ("planar_num", C.c_int32),
                ("sphere_num", C.c_int32), ("cvr_scan", C.c_double), ("cvr_submap", C.c_double),
                ("planar_scan_thres", C.c_double), ("planar_submap_thres", C.c_double),
                ("planar_vertic_thres", C.c_double)]


class SegConfig(C.Structure):
    """tloam_seg_config: the `velodyne`, `groundSeg` and `DCVC` blocks of config/mapping/segmentation.yaml."""
    _fields_ = [("sensor_model", C.c_int32), ("reserved0", C.c_int32), ("scan_period", C.c_double),
                ("sensor_height", C.c_double), ("vertical_res", C.c_double), ("init_angle", C.c_double),
                ("sensor_min_range", C.c_double), ("sensor_max_range", C.c_double), ("near_dis", C.c_double),
                ("quadrant", C.c_int32), ("num_sec", C.c_int32), ("dis", C.c_double), ("max_iter", C.c_int32),
                ("ground_seed_num", C.c_int32), ("ring_min_num", C.c_int32), ("reserved1", C.c_int32),
                ("start_r", C.c_double), ("delta_r", C.c_double), ("delta_p", C.c_double), ("delta_a", C.c_double),
                ("min_seg", C.c_int32), ("reserved2", C.c_int32)]


class OdomConfig(C.Structure):
    """tloam_odom_config: the three stage configurations plus edge_down_sample (lidar_odometry.yaml:8)."""
    _fields_ = [("seg", SegConfig), ("feature", FeatureConfig), ("submap", SubmapConfig), ("edge_down_sample", C.c_double)]


def _int_fields(info):
    """An info struct of integer fields as {name: int}."""
    return {name: int(getattr(info, name)) for name, _ in info._fields_}


class MapConfig(C.Structure):
    """tloam_map_config: mapping_flag (lidar_odometry.yaml:21), the map's voxel (front_end.cpp:272), the HBM reserved."""
    _fields_ = [("enabled", C.c_int32), ("reserved0", C.c_int32), ("voxel", C.c_double), ("reserve_points", C.c_int64)]


class MapInfo(C.Structure):
    """tloam_map_info."""
    _fields_ = [("n_points", C.c_int64), ("n_frames", C.c_int64), ("last_first", C.c_int64), ("last_count", C.c_int64),
                ("capacity_points", C.c_int64), ("overflow_frames", C.c_int64)]

    as_dict = _int_fields


class VoxelMapConfig(C.Structure):
    """tloam_voxel_map_config: the merged voxel map's switch, voxel v, origin o, the HBM reserved."""
    _fields_ = [("enabled", C.c_int32), ("reserved0", C.c_int32), ("voxel", C.c_double), ("origin", C.c_double * 3),
                ("reserve_voxels", C.c_int64)]


class VoxelMapInfo(C.Structure):
    """tloam_voxel_map_info."""
    _fields_ = [("n_voxels", C.c_int64), ("n_points", C.c_int64), ("n_frames", C.c_int64), ("last_new", C.c_int64),
                ("capacity_voxels", C.c_int64), ("overflow_frames", C.c_int64)]

    as_dict = _int_fields


class ClosedMapConfig(C.Structure):
    """tloam_closed_map_config: the closed map's voxel v, origin o, the cloud slots that take part (bit side * 4 + kind), the HBM
    the first build reserves."""
    _fields_ = [("voxel", C.c_double), ("origin", C.c_double * 3), ("cloud_mask", C.c_int32), ("reserved0", C.c_int32),
                ("reserve_voxels", C.c_int64)]


class ClosedMapInfo(C.Structure):
    """tloam_closed_map_info."""
    _fields_ = [("n_keyframes", C.c_int64), ("added_keyframes", C.c_int64), ("empty_keyframes", C.c_int64),
                ("overflow_keyframes", C.c_int64), ("n_voxels", C.c_int64), ("n_points", C.c_int64),
                ("capacity_voxels", C.c_int64), ("pose_source", C.c_int32), ("launches", C.c_int32)]

    as_dict = _int_fields


class ClosedMapCarveConfig(C.Structure):
    """tloam_closed_map_carve_config: the longest ray, the margin in front of a return in which nothing is missed, the largest
    distance from a centroid to a ray that misses it, the cloud slots whose points are rays (0: the build's)."""
    _fields_ = [("max_range", C.c_double), ("end_margin", C.c_double), ("radius", C.c_double), ("ray_mask", C.c_int32),
                ("reserved0", C.c_int32)]


class ClosedMapCarveInfo(C.Structure):
    """tloam_closed_map_carve_info."""
    _fields_ = [("n_keyframes", C.c_int64), ("n_rays", C.c_int64), ("skipped_rays", C.c_int64), ("steps", C.c_int64),
                ("tested", C.c_int64), ("misses", C.c_int64), ("voxels_missed", C.c_int64), ("launches", C.c_int32),
                ("reserved0", C.c_int32)]

    as_dict = _int_fields


class ClosedMapExtendInfo(C.Structure):
    """tloam_closed_map_extend_info: what one extension of the closed map took and did."""
    _fields_ = [("first_keyframe", C.c_int64), ("n_keyframes", C.c_int64), ("added_keyframes", C.c_int64),
                ("empty_keyframes", C.c_int64), ("overflow_keyframes", C.c_int64), ("points", C.c_int64), ("new_voxels", C.c_int64),
                ("touched_voxels", C.c_int64), ("rays", C.c_int64), ("skipped_rays", C.c_int64), ("steps", C.c_int64),
                ("tested", C.c_int64), ("misses", C.c_int64), ("solved_voxels", C.c_int64), ("grown", C.c_int32),
                ("launches", C.c_int32)]

    as_dict = _int_fields


class ClosedMapSurfelConfig(C.Structure):
    """tloam_closed_map_surfel_config: the fewest points a voxel is solved from."""
    _fields_ = [("min_points", C.c_int32), ("reserved0", C.c_int32)]


class ClosedMapSurfelInfo(C.Structure):
    """tloam_closed_map_surfel_info."""
    _fields_ = [("n_keyframes", C.c_int64), ("n_points", C.c_int64), ("orphan_points", C.c_int64), ("solved_voxels", C.c_int64),
                ("launches", C.c_int32), ("reserved0", C.c_int32)]

    as_dict = _int_fields


class ClosedMapLocaliseConfig(C.Structure):
    """tloam_closed_map_localise_config: the truncation's schedule (max_residual0 * shrink^k, floored at min_residual), the
    gate on the surfels (max_sigma, min_planarity), the step tolerances, the Cholesky's pivot ratio, the iteration limit and the
    fewest used points."""
    _fields_ = [("max_residual0", C.c_double), ("shrink", C.c_double), ("min_residual", C.c_double), ("max_sigma", C.c_double),
                ("min_planarity", C.c_double), ("step_tol_t", C.c_double), ("step_tol_r", C.c_double),
                ("min_pivot_ratio", C.c_double), ("max_iterations", C.c_int32), ("min_matches", C.c_int32)]


class ClosedMapLocaliseInfo(C.Structure):
    """tloam_closed_map_localise_info."""
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("matched", C.c_int64), ("used", C.c_int64), ("rms", C.c_double),
                ("launches", C.c_int32), ("prepared", C.c_int32)]

    def as_dict(self):
        return {"status": int(self.status), "iterations": int(self.iterations), "matched": int(self.matched),
                "used": int(self.used), "rms": float(self.rms), "launches": int(self.launches), "prepared": int(self.prepared)}


class ClosedMapLocaliseRecord(C.Structure):
    """tloam_closed_map_localise_record: one executed iteration."""
    _fields_ = [("pose_colmajor", C.c_double * 16), ("tau", C.c_double), ("cost", C.c_double), ("d", C.c_double * 6),
                ("matched", C.c_int64), ("used", C.c_int64)]

    def as_dict(self):
        return {"pose": np.array(self.pose_colmajor[:]).reshape(4, 4).T.copy(), "tau": float(self.tau), "cost": float(self.cost),
                "d": np.array(self.d[:]), "matched": int(self.matched), "used": int(self.used)}


LOCALISE_CONVERGED, LOCALISE_MAX_ITERATIONS, LOCALISE_DEGENERATE = 0, 1, 2
LOCALISE_MAX_BATCH = 32


class ClosedMapRelocaliseConfig(C.Structure):
    """tloam_closed_map_relocalise_config: how many keyframes are localised from, the Scan Context distance above which a
    candidate is skipped, and the acceptance of the winner.  The defaults are choices, not measurements."""
    _fields_ = [("num_candidates", C.c_int32), ("reserved0", C.c_int32), ("max_dist", C.c_double),
                ("min_used_ratio", C.c_double), ("max_rms", C.c_double)]


class ClosedMapRelocaliseInfo(C.Structure):
    """tloam_closed_map_relocalise_info."""
    _fields_ = [("status", C.c_int32), ("n_hypotheses", C.c_int32), ("best", C.c_int32), ("launches", C.c_int32),
                ("keyframe", C.c_int64), ("shift", C.c_int32), ("reserved0", C.c_int32), ("dist", C.c_double), ("yaw", C.c_double),
                ("localise", ClosedMapLocaliseInfo)]

    def as_dict(self):
        return {"status": int(self.status), "n_hypotheses": int(self.n_hypotheses), "best": int(self.best),
                "launches": int(self.launches), "keyframe": int(self.keyframe), "shift": int(self.shift),
                "dist": float(self.dist), "yaw": float(self.yaw), "localise": self.localise.as_dict()}


class ClosedMapRelocaliseHypothesis(C.Structure):
    """tloam_closed_map_relocalise_hypothesis."""
    _fields_ = [("keyframe", C.c_int64), ("shift", C.c_int32), ("skipped", C.c_int32), ("dist", C.c_double), ("yaw", C.c_double),
                ("prior_colmajor", C.c_double * 16), ("pose_colmajor", C.c_double * 16), ("localise", ClosedMapLocaliseInfo)]

    def as_dict(self):
        return {"keyframe": int(self.keyframe), "shift": int(self.shift), "skipped": int(self.skipped), "dist": float(self.dist),
                "yaw": float(self.yaw), "prior": np.array(self.prior_colmajor[:]).reshape(4, 4).T.copy(),
                "pose": np.array(self.pose_colmajor[:]).reshape(4, 4).T.copy(), "localise": self.localise.as_dict()}


RELOCALISE_FOUND, RELOCALISE_NOT_FOUND = 0, 1


class ClosedMapDiffConfig(C.Structure):
    """tloam_closed_map_diff_config: the rays' longest range, end margin and radius (the carve's meaning), the residual within
    which a point lies on a surfel, the distance within which a centroid explains it, and the carve gate (min_miss, miss_ratio,
    carve_gate).  The defaults are choices, not measurements."""
    _fields_ = [("max_range", C.c_double), ("end_margin", C.c_double), ("radius", C.c_double), ("plane_tol", C.c_double),
                ("near", C.c_double), ("min_miss", C.c_int64), ("miss_ratio", C.c_double), ("carve_gate", C.c_int32),
                ("reserved0", C.c_int32)]


class ClosedMapDiffInfo(C.Structure):
    """tloam_closed_map_diff_info."""
    _fields_ = [("n_points", C.c_int64), ("n_invalid", C.c_int64), ("n_surface", C.c_int64), ("n_occupied", C.c_int64),
                ("n_new", C.c_int64), ("rays", C.c_int64), ("skipped_rays", C.c_int64), ("steps", C.c_int64), ("tested", C.c_int64),
                ("through", C.c_int64), ("voxels_through", C.c_int64), ("voxels_hit", C.c_int64), ("scans", C.c_int64),
                ("launches", C.c_int32), ("prepared", C.c_int32), ("cleared", C.c_int32), ("reserved0", C.c_int32)]

    as_dict = _int_fields


DIFF_ACCUMULATE = 1   # TLOAM_DIFF_ACCUMULATE: the call adds to the stored counts
DIFF_INVALID, DIFF_SURFACE, DIFF_OCCUPIED, DIFF_NEW = 0, 1, 2, 3


class ClosedMapRaycastConfig(C.Structure):
    """tloam_closed_map_raycast_config: the longest segment, the hit radius in voxel sizes, the fewest points of a voxel a ray
    can hit, the carve gate (min_miss, miss_ratio, carve_gate) and which test a voxel is put to (planes: 0 the centroid test
    alone, 1 the plane test where the voxel is eligible, 2 the plane test alone).  The defaults are
    choices, not measurements."""
    _fields_ = [("max_range", C.c_double), ("radius_cells", C.c_double), ("min_count", C.c_int64), ("min_miss", C.c_int64),
                ("miss_ratio", C.c_double), ("planes", C.c_int32), ("carve_gate", C.c_int32)]


class ClosedMapRaycastInfo(C.Structure):
    """tloam_closed_map_raycast_info."""
    _fields_ = [("rays", C.c_int64), ("skipped", C.c_int64), ("missed", C.c_int64), ("hits_centroid", C.c_int64),
                ("hits_plane", C.c_int64), ("steps", C.c_int64), ("tested", C.c_int64), ("launches", C.c_int32),
                ("prepared", C.c_int32)]

    as_dict = _int_fields


RAYCAST_SKIPPED, RAYCAST_MISS, RAYCAST_HIT_CENTROID, RAYCAST_HIT_PLANE = 0, 1, 2, 3   # TLOAM_RAYCAST_*


class FreeConfig(C.Structure):
    """tloam_closed_map_free_config: the rays' longest range and end margin (the carve's meaning), the most bytes a grid may
    take, which voxels count as occupied when the grid is read (min_count and the carve gate: min_miss, miss_ratio, carve_gate),
    and the keyframe clouds whose points are rays.  The defaults are choices, not measurements."""
    _fields_ = [("max_range", C.c_double), ("end_margin", C.c_double), ("max_bytes", C.c_int64), ("min_count", C.c_int64),
                ("min_miss", C.c_int64), ("miss_ratio", C.c_double), ("ray_mask", C.c_int32), ("carve_gate", C.c_int32)]


class FreeInfo(C.Structure):
    """tloam_closed_map_free_info."""
    _fields_ = [("lo_cells", C.c_int64 * 3), ("n_bricks", C.c_int64 * 3), ("bytes", C.c_int64), ("keyframes", C.c_int64),
                ("scans", C.c_int64), ("free_cells", C.c_int64), ("bricks_nonzero", C.c_int64), ("rays", C.c_int64),
                ("skipped_rays", C.c_int64), ("cells_marked", C.c_int64), ("cells_outside", C.c_int64), ("launches", C.c_int32),
                ("reserved0", C.c_int32)]

    def as_dict(self):
        d = {name: int(getattr(self, name)) for name, _ in self._fields_[2:]}
        return {"lo_cells": tuple(int(x) for x in self.lo_cells), "n_bricks": tuple(int(x) for x in self.n_bricks), **d}


OCCUPANCY_INVALID, OCCUPANCY_UNKNOWN, OCCUPANCY_FREE, OCCUPANCY_OCCUPIED = 0, 1, 2, 3   # TLOAM_OCCUPANCY_*


SNAPSHOT_CLOUDS = 1   # TLOAM_SNAPSHOT_CLOUDS: the keyframes' eight clouds go into the snapshot too


class ClosedMapSnapshotInfo(C.Structure):
    """tloam_closed_map_snapshot_info: what a closed map snapshot says it holds."""
    _fields_ = [("format_version", C.c_int32), ("flags", C.c_int32), ("n_keyframes_database", C.c_int64),
                ("n_keyframes_map", C.c_int64), ("n_voxels", C.c_int64), ("n_points", C.c_int64), ("has_carve", C.c_int32),
                ("has_surfels", C.c_int32), ("has_clouds", C.c_int32), ("n_rings", C.c_int32), ("n_sectors", C.c_int32),
                ("reserved0", C.c_int32), ("cloud_points", C.c_int64), ("voxel", C.c_double), ("origin", C.c_double * 3),
                ("bytes", C.c_uint64)]

    def as_dict(self):
        out = {name: getattr(self, name) for name, _ in self._fields_ if name not in ("origin", "reserved0")}
        out["origin"] = tuple(self.origin)
        return out


class DeskewConfig(C.Structure):
    """tloam_deskew_config: the deskew's switch, its time source (0 azimuth, 1 per-point times), the sweep's direction (+1
    counter-clockwise seen from +z), the azimuth it starts at and the sweep fraction the pose describes."""
    _fields_ = [("enabled", C.c_int32), ("time_source", C.c_int32), ("direction", C.c_int32), ("reserved0", C.c_int32),
                ("start_azimuth", C.c_double), ("ref_fraction", C.c_double)]


class DeskewInfo(C.Structure):
    """tloam_deskew_info."""
    _fields_ = [("frames_deskewed", C.c_int64), ("last_frame", C.c_int64), ("last_twist", C.c_double * 6),
                ("last_max_shift", C.c_double), ("next_motion_colmajor", C.c_double * 16)]

    def as_dict(self):
        return {"frames_deskewed": int(self.frames_deskewed), "last_frame": int(self.last_frame),
                "last_twist": np.array(self.last_twist[:]), "last_max_shift": float(self.last_max_shift),
                "next_motion": np.array(self.next_motion_colmajor[:]).reshape(4, 4).T.copy()}


class PlaceConfig(C.Structure):
    """tloam_place_config: place recognition's switch, the Scan Context grid (rings x sectors within max_radius, z +
    height_offset), the search (num_candidates ring-key neighbours older than exclude_recent keyframes, a loop below
    dist_thres), the keyframe policy (kf_dist, kf_angle) and the HBM reserved."""
    _fields_ = [("enabled", C.c_int32), ("n_rings", C.c_int32), ("n_sectors", C.c_int32), ("num_candidates", C.c_int32),
                ("exclude_recent", C.c_int32), ("reserved0", C.c_int32), ("max_radius", C.c_double),
                ("height_offset", C.c_double), ("kf_dist", C.c_double), ("kf_angle", C.c_double), ("dist_thres", C.c_double),
                ("reserve_keyframes", C.c_int64)]


class PlaceInfo(C.Structure):
    """tloam_place_info."""
    _fields_ = [("n_keyframes", C.c_int64), ("n_loops", C.c_int64), ("last_keyframe_frame", C.c_int64),
                ("capacity_keyframes", C.c_int64)]

    as_dict = _int_fields


class PlaceLoop(C.Structure):
    """tloam_place_loop: one loop record."""
    _fields_ = [("query_keyframe", C.c_int64), ("query_frame", C.c_int64), ("match_keyframe", C.c_int64),
                ("match_frame", C.c_int64), ("shift", C.c_int32), ("reserved0", C.c_int32), ("dist", C.c_double),
                ("yaw", C.c_double)]

    def as_dict(self):
        return {"query": int(self.query_keyframe), "query_frame": int(self.query_frame), "match": int(self.match_keyframe),
                "match_frame": int(self.match_frame), "shift": int(self.shift), "d": float(self.dist), "yaw": float(self.yaw)}


class LoopInfo(C.Structure):
    """tloam_loop_info."""
    _fields_ = [("n_constraints", C.c_int64), ("n_accepted", C.c_int64), ("arena_points", C.c_int64),
                ("arena_capacity_points", C.c_int64)]

    as_dict = _int_fields


class GraphConfig(C.Structure):
    """tloam_graph_config: the pose-graph optimisation's iteration limits and tolerances, and the sigmas the context's graph
    weights its chain (odometry) and loop edges with."""
    _fields_ = [("max_iterations", C.c_int32), ("max_cg_iterations", C.c_int32), ("step_tol", C.c_double),
                ("cg_tol", C.c_double), ("odom_sigma_t", C.c_double), ("odom_sigma_r", C.c_double),
                ("loop_sigma_t", C.c_double), ("loop_sigma_r", C.c_double)]


class GraphEdge(C.Structure):
    """tloam_graph_edge: (i, j, Z = rigid_inverse(P_i) P_j column-major, six inverse variances)."""
    _fields_ = [("i", C.c_int64), ("j", C.c_int64), ("rel_pose_colmajor", C.c_double * 16), ("weight", C.c_double * 6)]


GRAPH_STOP = {0: "not_run", 1: "step", 2: "iterations", 3: "cost", 4: "cg_limit"}


class GraphInfo(C.Structure):
    """tloam_graph_info."""
    _fields_ = [("n_nodes", C.c_int64), ("n_edges", C.c_int64), ("n_loop_edges", C.c_int64), ("iterations", C.c_int32),
                ("stop_reason", C.c_int32), ("reverted", C.c_int32), ("reserved0", C.c_int32), ("cg_iterations", C.c_int64),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("last_step", C.c_double),
                ("last_cg_residual", C.c_double)]

    def as_dict(self):
        return {"n_nodes": int(self.n_nodes), "n_edges": int(self.n_edges), "n_loop_edges": int(self.n_loop_edges),
                "iterations": int(self.iterations), "stop_reason": int(self.stop_reason), "stop": GRAPH_STOP[int(self.stop_reason)],
                "reverted": int(self.reverted), "cg_iterations": int(self.cg_iterations), "initial_cost": float(self.initial_cost),
                "final_cost": float(self.final_cost), "last_step": float(self.last_step),
                "last_cg_residual": float(self.last_cg_residual)}


class GraphRobustConfig(C.Structure):
    """tloam_graph_robust_config: the robust mode of the pose graph, GNC-TLS on the loop edges."""
    _fields_ = [("enabled", C.c_int32), ("max_outer", C.c_int32), ("noise_chi2", C.c_double), ("mu_factor", C.c_double)]


GRAPH_ROBUST_STOP = {0: "off", 1: "all_inliers", 2: "binary", 3: "outer_limit"}


class GraphRobustInfo(C.Structure):
    """tloam_graph_robust_info."""
    _fields_ = [("outer_iterations", C.c_int32), ("stop_reason", C.c_int32), ("gn_iterations", C.c_int64),
                ("cg_iterations", C.c_int64), ("rejected", C.c_int64), ("kept", C.c_int64), ("undecided", C.c_int64),
                ("mu_first", C.c_double), ("mu_last", C.c_double), ("max_chi2_first", C.c_double)]

    def as_dict(self):
        return {"outer_iterations": int(self.outer_iterations), "stop_reason": int(self.stop_reason),
                "stop": GRAPH_ROBUST_STOP[int(self.stop_reason)], "gn_iterations": int(self.gn_iterations),
                "cg_iterations": int(self.cg_iterations), "rejected": int(self.rejected), "kept": int(self.kept),
                "undecided": int(self.undecided), "mu_first": float(self.mu_first), "mu_last": float(self.mu_last),
                "max_chi2_first": float(self.max_chi2_first)}


class TlsConfig(C.Structure):
    """tloam_tls_config: the 16 keys of the `TLS:` block (config/mapping/lidar_odometry.yaml:23-39)."""
    _fields_ = [
        ("k_corr", C.c_int32), ("factor_num", C.c_int32),
        ("edge_dist_thres", C.c_double), ("edge_dir_thres", C.c_double),
        ("edge_maxnum", C.c_int32), ("sphere_maxnum", C.c_int32),
        ("sphere_dist_thres", C.c_double), ("planar_dist_thres", C.c_double),
        ("planar_maxnum", C.c_int32), ("ground_maxnum", C.c_int32),
        ("ground_dist_thres", C.c_double),
        ("max_iterations", C.c_int32), ("reserved0", C.c_int32),
        ("cost_threshold", C.c_double), ("gnc_factor", C.c_double),
        ("noise_bound", C.c_double), ("fitness_thres", C.c_double),
    ]


class LoopConfig(C.Structure):
    """tloam_loop_config: loop verification's switch, the target window around the match keyframe, the initial guess (0: the
    loop record's yaw, 1: the stored poses), the score's inlier distance and the acceptance bounds, the arena reserved, and the
    coarse stage's TLS configuration."""
    _fields_ = [("enabled", C.c_int32), ("window", C.c_int32), ("init_mode", C.c_int32), ("reserved0", C.c_int32),
                ("inlier_dist", C.c_double), ("min_overlap", C.c_double), ("max_rmse", C.c_double),
                ("reserve_points", C.c_int64), ("coarse", TlsConfig)]


class CtxInfo(C.Structure):
    """tloam_ctx_info."""
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("device_cus", C.c_int32), ("comm_mode", C.c_int32),
                ("rank", C.c_int32), ("nranks", C.c_int32), ("rccl_comm_count", C.c_int32), ("rccl_comm_rank", C.c_int32),
                ("fallbacks_taken", C.c_int32), ("fallback_events", C.c_int32), ("k3_grid", C.c_int32), ("k3_single", C.c_int32),
                ("one_launch_solve", C.c_int32), ("loopback", C.c_int32), ("direct_set", C.c_int32), ("set_stale", C.c_int32),
                ("k3_wide", C.c_int32)]


class GridInfo(C.Structure):
    """tloam_grid_info."""
    _fields_ = [("dim", (C.c_int32 * 3) * 4), ("n", C.c_int32 * 4), ("ncell", C.c_int64 * 4), ("cell", C.c_double * 4),
                ("scan_path", C.c_int32), ("table_elem_bytes", C.c_int32)]


GRID_SCAN_NONE, GRID_SCAN_SMALL, GRID_SCAN_TILES, GRID_SCAN_SINGLE_PASS, GRID_SCAN_GENERIC = range(5)


class Stats(C.Structure):
    """tloam_stats."""
    _fields_ = [
        ("outer_iterations", C.c_int32), ("gn_evaluations", C.c_int32),
        ("gn_iterations", C.c_int32), ("accepted_steps", C.c_int32),
        ("n_corr", C.c_int32 * 4), ("converged_early", C.c_int32), ("weight_range_violations", C.c_int32),
        ("kind_cost", C.c_double * 4), ("mu", C.c_double), ("solver_cost", C.c_double),
        ("se3", C.c_double * 6),
        ("gn_sweeps", C.c_int32), ("host_wait_us", C.c_int32),
    ]

    def as_dict(self):
        # (on the per-frame path of every caller: array fields as slices / a buffer view, ~2 us instead of ~4)
        return {"outer_iterations": self.outer_iterations, "gn_evaluations": self.gn_evaluations,
                "gn_iterations": self.gn_iterations, "accepted_steps": self.accepted_steps,
                "n_corr": self.n_corr[:], "converged_early": self.converged_early,
                "bad_weights": self.weight_range_violations, "kind_cost": self.kind_cost[:], "mu": self.mu,
                "solver_cost": self.solver_cost, "se3": np.frombuffer(self.se3, dtype=np.float64).copy(),
                "gn_sweeps": self.gn_sweeps, "host_wait_us": self.host_wait_us}


class LoopConstraint(C.Structure):
    """tloam_loop_constraint: one verified pair."""
    _fields_ = [("query_keyframe", C.c_int64), ("query_frame", C.c_int64), ("match_keyframe", C.c_int64),
                ("match_frame", C.c_int64), ("status", C.c_int32), ("accepted", C.c_int32),
                ("rel_pose_colmajor", C.c_double * 16), ("init_colmajor", C.c_double * 16), ("coarse", Stats), ("fine", Stats),
                ("overlap", C.c_double), ("rmse", C.c_double), ("inliers", C.c_int64), ("points", C.c_int64),
                ("dist", C.c_double), ("yaw", C.c_double)]

    def as_dict(self):
        return {"query": int(self.query_keyframe), "query_frame": int(self.query_frame), "match": int(self.match_keyframe),
                "match_frame": int(self.match_frame), "status": int(self.status), "accepted": bool(self.accepted),
                "rel_pose": np.array(self.rel_pose_colmajor[:]).reshape(4, 4).T.copy(),
                "init": np.array(self.init_colmajor[:]).reshape(4, 4).T.copy(),
                "coarse": self.coarse.as_dict(), "fine": self.fine.as_dict(), "overlap": float(self.overlap),
                "rmse": float(self.rmse), "inliers": int(self.inliers), "points": int(self.points), "d": float(self.dist),
                "yaw": float(self.yaw)}


class OdomStats(C.Structure):
    """tloam_odom_stats."""
    _fields_ = [("match", Stats), ("frame", C.c_int64), ("n_ground", C.c_int64), ("n_edge", C.c_int64),
                ("n_general", C.c_int64), ("n_edge_ds", C.c_int64), ("n_ground_ds", C.c_int64),
                ("n_planar_scan", C.c_int64), ("n_sphere_scan", C.c_int64), ("n_planar_submap", C.c_int64),
                ("n_sphere_submap", C.c_int64), ("h2d_bytes", C.c_int64), ("d2h_bytes", C.c_int64), ("host_syncs", C.c_int64)]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_[1:]}
        d["match"] = self.match.as_dict()
        return d


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)

_lib = None


class TloamHipError(RuntimeError):
    pass


def load_library():
    """dlopen libtloam_hip.so (built by tloam_amd/build.py).  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TloamHipError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in HBM (effective if HIP is not up yet)
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    sz = C.c_size_t
    sig = {
        "tloam_abi_version": (C.c_int, []),
        "tloam_status_string": (C.c_char_p, [C.c_int]),
        "tloam_last_error": (C.c_char_p, [vp]),
        "tloam_default_config": (None, [C.POINTER(TlsConfig)]),
        "tloam_create": (C.c_int, [C.POINTER(TlsConfig), C.c_int, C.POINTER(vp)]),
        "tloam_destroy": (None, [vp]),
        "tloam_set_source": (C.c_int, [vp, C.c_int, dp, sz]),
        "tloam_set_target": (C.c_int, [vp, C.c_int, dp, sz]),
        "tloam_set_source_frame": (C.c_int, [vp, C.POINTER(dp), C.POINTER(sz)]),
        "tloam_set_target_frame": (C.c_int, [vp, C.POINTER(dp), C.POINTER(sz)]),
        "tloam_frame_stash": (C.c_int, [vp, C.c_int]),
        "tloam_frame_select": (C.c_int, [vp, C.c_int]),
        "tloam_scan_match": (C.c_int, [vp, dp, dp, dp, dp, sz, C.POINTER(Stats)]),
        "tloam_sm_begin": (C.c_int, [vp, dp, dp]),
        "tloam_sm_outer": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(Stats)]),
        "tloam_sm_end": (C.c_int, [vp, dp, C.POINTER(Stats)]),
        "tloam_fitness": (C.c_int, [vp, dp, dp]),
        "tloam_get_correspondences": (C.c_int, [vp, C.c_int, sz, C.POINTER(sz), ip, dp, dp, dp, dp, dp]),
        "tloam_get_weights": (C.c_int, [vp, C.c_int, sz, C.POINTER(sz), dp]),
        "tloam_knn": (C.c_int, [vp, C.c_int, dp, sz, C.c_double, C.c_int, ip, dp, ip]),
        "tloam_set_correspondences": (C.c_int, [vp, C.c_int, sz, dp, dp, dp, dp, dp]),
        "tloam_accumulate": (C.c_int, [vp, dp, dp, dp, dp]),
        "tloam_get_costs": (C.c_int, [vp, C.c_int, sz, C.POINTER(sz), dp]),
        "tloam_get_normal_equations": (C.c_int, [vp, dp, dp, dp]),
        "tloam_comm_mailbox_export": (C.c_int, [vp, vp]),
        "tloam_comm_init_mailbox": (C.c_int, [vp, C.c_int, C.c_int, vp]),
        "tloam_solve": (C.c_int, [vp, dp, C.POINTER(Stats)]),
        "tloam_time_accumulate": (C.c_int, [vp, dp, C.c_int, dp]),
        "tloam_time_sharded_sweep": (C.c_int, [vp, dp, C.c_int, C.c_int, dp]),
        "tloam_time_build": (C.c_int, [vp, C.c_int, dp, C.POINTER(C.c_int64)]),
        "tloam_k3_timer": (C.c_int, [vp, C.c_int, dp, C.POINTER(C.c_int64), dp]),
        "tloam_k3_timer_all": (C.c_int, [vp, dp, C.POINTER(C.c_int64)]),
        "tloam_k3_span": (C.c_int, [vp, C.c_int, dp, C.POINTER(C.c_int64)]),
        "tloam_gn_iter_timer": (C.c_int, [vp, C.c_int, dp, C.POINTER(C.c_int64)]),
        "tloam_time_read_stream": (C.c_int, [vp, sz, C.c_int, dp]),
        "tloam_get_info": (C.c_int, [vp, C.POINTER(CtxInfo)]),
        "tloam_get_grid_info": (C.c_int, [vp, C.POINTER(GridInfo)]),
        "tloam_debug_state": (C.c_int, [vp, dp, C.c_int]),
        "tloam_debug_se3": (C.c_int, [vp, C.c_int, dp, dp, dp]),
        "tloam_debug_partials": (C.c_int, [vp, dp, C.c_int]),
        "tloam_debug_raise_fault": (C.c_int, [vp, C.c_int]),
        "tloam_submap_default_config": (None, [C.POINTER(SubmapConfig)]),
        "tloam_submap_init": (C.c_int, [vp, C.POINTER(SubmapConfig), dp, sz, dp, sz, dp, sz, dp, sz]),
        "tloam_submap_update": (C.c_int, [vp, dp, dp, sz, dp, sz, dp, sz, dp, sz]),
        "tloam_get_target": (C.c_int, [vp, C.c_int, sz, C.POINTER(sz), dp]),
        "tloam_feature_default_config": (None, [C.POINTER(FeatureConfig)]),
        "tloam_pca_info": (C.c_int, [vp, C.POINTER(FeatureConfig), dp, sz, dp, dp, dp, dp, ip, ip]),
        "tloam_extract_planar_sphere": (C.c_int, [vp, C.POINTER(FeatureConfig), dp, sz, ip, C.POINTER(sz), ip,
                                                  C.POINTER(sz), ip, C.POINTER(sz), ip, C.POINTER(sz)]),
        "tloam_seg_default_config": (None, [C.POINTER(SegConfig)]),
        "tloam_segment": (C.c_int, [vp, C.POINTER(SegConfig), dp, sz, ip, ip, C.POINTER(sz), ip, C.POINTER(sz), ip, ip,
                                    C.POINTER(sz), ip, C.POINTER(sz), ip, C.POINTER(sz), dp, sz, C.POINTER(sz)]),
        "tloam_voxel_down_sample": (C.c_int, [vp, C.c_double, dp, sz, dp, sz, C.POINTER(sz)]),
        "tloam_odom_default_config": (None, [C.POINTER(OdomConfig)]),
        "tloam_odometry_reset": (C.c_int, [vp, C.POINTER(OdomConfig), dp]),
        "tloam_odometry_frame": (C.c_int, [vp, dp, sz, dp, C.POINTER(OdomStats)]),
        "tloam_map_default_config": (None, [C.POINTER(MapConfig)]),
        "tloam_map_configure": (C.c_int, [vp, C.POINTER(MapConfig)]),
        "tloam_map_get_info": (C.c_int, [vp, C.POINTER(MapInfo)]),
        "tloam_map_read": (C.c_int, [vp, sz, sz, dp]),
        "tloam_registered_scan": (C.c_int, [vp, sz, C.POINTER(sz), dp]),
        "tloam_voxel_map_default_config": (None, [C.POINTER(VoxelMapConfig)]),
        "tloam_voxel_map_configure": (C.c_int, [vp, C.POINTER(VoxelMapConfig)]),
        "tloam_voxel_map_get_info": (C.c_int, [vp, C.POINTER(VoxelMapInfo)]),
        "tloam_voxel_map_read": (C.c_int, [vp, sz, sz, dp, C.POINTER(C.c_int64)]),
        "tloam_voxel_map_read_box": (C.c_int, [vp, dp, dp, C.c_int64, sz, C.POINTER(sz), dp, C.POINTER(C.c_int64)]),
        "tloam_deskew_default_config": (None, [C.POINTER(DeskewConfig)]),
        "tloam_deskew_configure": (C.c_int, [vp, C.POINTER(DeskewConfig)]),
        "tloam_deskew_get_info": (C.c_int, [vp, C.POINTER(DeskewInfo)]),
        "tloam_odometry_frame_timed": (C.c_int, [vp, dp, dp, sz, dp, C.POINTER(OdomStats)]),
        "tloam_deskew_scan": (C.c_int, [vp, C.POINTER(DeskewConfig), C.c_double, dp, dp, dp, sz, dp]),
        "tloam_place_default_config": (None, [C.POINTER(PlaceConfig)]),
        "tloam_place_configure": (C.c_int, [vp, C.POINTER(PlaceConfig)]),
        "tloam_place_get_info": (C.c_int, [vp, C.POINTER(PlaceInfo)]),
        "tloam_place_read_keyframes": (C.c_int, [vp, sz, sz, C.POINTER(C.c_int64), dp, dp, dp, dp]),
        "tloam_place_read_loops": (C.c_int, [vp, sz, sz, C.POINTER(PlaceLoop)]),
        "tloam_place_add_scan": (C.c_int, [vp, dp, sz, dp, C.c_int64, C.POINTER(C.c_int64)]),
        "tloam_place_describe": (C.c_int, [vp, C.POINTER(PlaceConfig), dp, sz, dp, dp, dp]),
        "tloam_loop_default_config": (None, [C.POINTER(LoopConfig)]),
        "tloam_loop_configure": (C.c_int, [vp, C.POINTER(LoopConfig)]),
        "tloam_loop_get_info": (C.c_int, [vp, C.POINTER(LoopInfo)]),
        "tloam_place_set_keyframe_clouds": (C.c_int, [vp, C.c_int64, C.POINTER(dp), C.POINTER(sz), C.POINTER(dp),
                                                      C.POINTER(sz)]),
        "tloam_place_read_keyframe_clouds": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, sz, C.POINTER(sz), dp]),
        "tloam_loop_verify_pending": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "tloam_loop_verify_pair": (C.c_int, [vp, C.c_int64, C.c_int64, dp, C.POINTER(LoopConstraint)]),
        "tloam_loop_read_constraints": (C.c_int, [vp, sz, sz, C.POINTER(LoopConstraint)]),
        "tloam_graph_default_config": (None, [C.POINTER(GraphConfig)]),
        "tloam_graph_configure": (C.c_int, [vp, C.POINTER(GraphConfig)]),
        "tloam_graph_solve": (C.c_int, [vp, C.POINTER(GraphConfig), sz, dp, sz, C.POINTER(GraphEdge), dp, C.POINTER(GraphInfo)]),
        "tloam_graph_optimize": (C.c_int, [vp, C.POINTER(GraphInfo)]),
        "tloam_graph_read_poses": (C.c_int, [vp, sz, sz, dp]),
        "tloam_graph_correct_pose": (C.c_int, [vp, C.c_int64, dp, dp]),
        "tloam_graph_robust_default_config": (None, [C.POINTER(GraphRobustConfig)]),
        "tloam_graph_robust_configure": (C.c_int, [vp, C.POINTER(GraphRobustConfig)]),
        "tloam_graph_solve_robust": (C.c_int, [vp, C.POINTER(GraphConfig), C.POINTER(GraphRobustConfig), sz, dp, sz,
                                               C.POINTER(GraphEdge), dp, C.POINTER(GraphInfo), C.POINTER(GraphRobustInfo), dp, dp]),
        "tloam_graph_read_loop_scales": (C.c_int, [vp, sz, sz, C.POINTER(C.c_int64), dp, dp]),
        "tloam_graph_get_robust_info": (C.c_int, [vp, C.POINTER(GraphRobustInfo)]),
        "tloam_closed_map_default_config": (None, [C.POINTER(ClosedMapConfig)]),
        "tloam_closed_map_configure": (C.c_int, [vp, C.POINTER(ClosedMapConfig)]),
        "tloam_closed_map_get_info": (C.c_int, [vp, C.POINTER(ClosedMapInfo)]),
        "tloam_closed_map_build": (C.c_int, [vp, C.c_int, dp, sz, C.POINTER(ClosedMapInfo)]),
        "tloam_closed_map_read": (C.c_int, [vp, sz, sz, dp, C.POINTER(C.c_int64)]),
        "tloam_closed_map_read_box": (C.c_int, [vp, dp, dp, C.c_int64, sz, C.POINTER(sz), dp, C.POINTER(C.c_int64)]),
        "tloam_closed_map_read_poses": (C.c_int, [vp, sz, sz, dp]),
        "tloam_closed_map_extend": (C.c_int, [vp, C.c_int, dp, sz, C.POINTER(ClosedMapExtendInfo)]),
        "tloam_closed_map_get_extend_info": (C.c_int, [vp, C.POINTER(ClosedMapExtendInfo)]),
        "tloam_closed_map_carve_default_config": (None, [C.POINTER(ClosedMapCarveConfig)]),
        "tloam_closed_map_carve_configure": (C.c_int, [vp, C.POINTER(ClosedMapCarveConfig)]),
        "tloam_closed_map_get_carve_info": (C.c_int, [vp, C.POINTER(ClosedMapCarveInfo)]),
        "tloam_closed_map_carve": (C.c_int, [vp, C.POINTER(ClosedMapCarveInfo)]),
        "tloam_closed_map_read_misses": (C.c_int, [vp, sz, sz, C.POINTER(C.c_int64)]),
        "tloam_closed_map_read_carved": (C.c_int, [vp, dp, dp, C.c_int64, C.c_int64, C.c_double, sz, C.POINTER(sz), dp,
                                                   C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "tloam_closed_map_surfel_default_config": (None, [C.POINTER(ClosedMapSurfelConfig)]),
        "tloam_closed_map_surfel_configure": (C.c_int, [vp, C.POINTER(ClosedMapSurfelConfig)]),
        "tloam_closed_map_get_surfel_info": (C.c_int, [vp, C.POINTER(ClosedMapSurfelInfo)]),
        "tloam_closed_map_surfels": (C.c_int, [vp, C.POINTER(ClosedMapSurfelInfo)]),
        "tloam_closed_map_localise_default_config": (None, [C.POINTER(ClosedMapLocaliseConfig)]),
        "tloam_closed_map_localise_configure": (C.c_int, [vp, C.POINTER(ClosedMapLocaliseConfig)]),
        "tloam_closed_map_localise": (C.c_int, [vp, dp, sz, dp, dp, C.POINTER(ClosedMapLocaliseInfo)]),
        "tloam_closed_map_localise_log": (C.c_int, [vp, sz, C.POINTER(sz), C.POINTER(ClosedMapLocaliseRecord)]),
        "tloam_closed_map_linearise": (C.c_int, [vp, dp, sz, dp, C.c_double, C.POINTER(C.c_int32), dp, dp, C.POINTER(C.c_int64)]),
        "tloam_closed_map_localise_batch": (C.c_int, [vp, dp, sz, dp, sz, dp, C.POINTER(ClosedMapLocaliseInfo),
                                                      C.POINTER(C.c_int32)]),
        "tloam_closed_map_localise_batch_log": (C.c_int, [vp, sz, sz, C.POINTER(sz), C.POINTER(ClosedMapLocaliseRecord)]),
        "tloam_closed_map_relocalise_default_config": (None, [C.POINTER(ClosedMapRelocaliseConfig)]),
        "tloam_closed_map_relocalise_configure": (C.c_int, [vp, C.POINTER(ClosedMapRelocaliseConfig)]),
        "tloam_closed_map_relocalise": (C.c_int, [vp, dp, sz, dp, C.POINTER(ClosedMapRelocaliseInfo)]),
        "tloam_closed_map_relocalise_hypotheses": (C.c_int, [vp, sz, C.POINTER(sz), C.POINTER(ClosedMapRelocaliseHypothesis)]),
        "tloam_closed_map_read_moments": (C.c_int, [vp, sz, sz, C.POINTER(C.c_int64)]),
        "tloam_closed_map_read_surfels": (C.c_int, [vp, sz, sz, dp, dp, C.POINTER(C.c_int64)]),
        "tloam_closed_map_read_surfels_box": (C.c_int, [vp, dp, dp, C.c_int64, C.c_double, C.c_double, sz, C.POINTER(sz), dp, dp, dp,
                                                        C.POINTER(C.c_int64)]),
        "tloam_closed_map_diff_default_config": (None, [C.POINTER(ClosedMapDiffConfig)]),
        "tloam_closed_map_diff_configure": (C.c_int, [vp, C.POINTER(ClosedMapDiffConfig)]),
        "tloam_closed_map_get_diff_info": (C.c_int, [vp, C.POINTER(ClosedMapDiffInfo)]),
        "tloam_closed_map_diff": (C.c_int, [vp, dp, sz, dp, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_int32),
                                            C.POINTER(ClosedMapDiffInfo)]),
        "tloam_closed_map_read_diff": (C.c_int, [vp, sz, sz, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "tloam_closed_map_raycast_default_config": (None, [C.POINTER(ClosedMapRaycastConfig)]),
        "tloam_closed_map_raycast_configure": (C.c_int, [vp, C.POINTER(ClosedMapRaycastConfig)]),
        "tloam_closed_map_get_raycast_info": (C.c_int, [vp, C.POINTER(ClosedMapRaycastInfo)]),
        "tloam_closed_map_raycast": (C.c_int, [vp, dp, sz, dp, C.POINTER(C.c_uint8), dp, C.POINTER(C.c_int32),
                                               C.POINTER(ClosedMapRaycastInfo)]),
        "tloam_closed_map_free_default_config": (None, [C.POINTER(FreeConfig)]),
        "tloam_closed_map_free_configure": (C.c_int, [vp, C.POINTER(FreeConfig)]),
        "tloam_closed_map_get_free_info": (C.c_int, [vp, C.POINTER(FreeInfo)]),
        "tloam_closed_map_free_reset": (C.c_int, [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "tloam_closed_map_free_add_keyframes": (C.c_int, [vp, C.POINTER(FreeInfo)]),
        "tloam_closed_map_free_add_scan": (C.c_int, [vp, dp, sz, dp, C.POINTER(FreeInfo)]),
        "tloam_closed_map_read_free_words": (C.c_int, [vp, sz, sz, C.POINTER(C.c_uint64)]),
        "tloam_closed_map_occupancy": (C.c_int, [vp, dp, sz, dp, C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
        "tloam_closed_map_read_free": (C.c_int, [vp, dp, dp, sz, C.POINTER(sz), dp]),
        "tloam_closed_map_free_columns": (C.c_int, [vp, C.c_double, C.c_double, C.c_int64, C.POINTER(C.c_uint8), sz, C.POINTER(sz),
                                                    C.POINTER(sz)]),
        "tloam_closed_map_read_gone": (C.c_int, [vp, dp, dp, C.c_int64, C.c_double, sz, C.POINTER(sz), dp, C.POINTER(C.c_int64),
                                                 C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "tloam_closed_map_save_size": (C.c_int, [vp, C.c_int, C.POINTER(sz)]),
        "tloam_closed_map_save": (C.c_int, [vp, C.c_int, vp, sz, C.POINTER(sz)]),
        "tloam_closed_map_probe": (C.c_int, [vp, sz, C.POINTER(ClosedMapSnapshotInfo)]),
        "tloam_closed_map_load": (C.c_int, [vp, vp, sz, C.POINTER(ClosedMapSnapshotInfo)]),
        "tloam_rccl_unique_id": (C.c_int, [vp]),
        "tloam_comm_init_rccl": (C.c_int, [vp, C.c_int, C.c_int, vp]),
        "tloam_comm_init_callback": (C.c_int, [vp, C.c_int, C.c_int, ALLREDUCE_FN, vp]),
        "tloam_shard_range": (None, [sz, C.c_int, C.c_int, C.POINTER(sz), C.POINTER(sz)]),
        "tloam_shard_ranges_frame": (None, [C.POINTER(sz), C.c_int, C.c_int, C.POINTER(sz), C.POINTER(sz)]),
        "tloam_se3_exp": (C.c_int, [dp, dp]),
        "tloam_se3_log": (C.c_int, [dp, dp]),
        "tloam_se3_plus": (C.c_int, [dp, dp, dp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError if the ABI lost a symbol
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


EXPORTED_SYMBOLS = (
    "tloam_abi_version", "tloam_status_string", "tloam_last_error", "tloam_default_config", "tloam_create",
    "tloam_destroy", "tloam_set_source", "tloam_set_target", "tloam_set_source_frame", "tloam_set_target_frame",
    "tloam_frame_stash", "tloam_frame_select", "tloam_scan_match", "tloam_sm_begin",
    "tloam_sm_outer", "tloam_sm_end", "tloam_fitness", "tloam_get_correspondences", "tloam_get_weights",
    "tloam_knn", "tloam_set_correspondences", "tloam_accumulate", "tloam_get_costs", "tloam_get_normal_equations",
    "tloam_solve",
    "tloam_time_accumulate", "tloam_time_sharded_sweep", "tloam_time_build", "tloam_k3_timer", "tloam_k3_timer_all", "tloam_k3_span", "tloam_gn_iter_timer", "tloam_time_read_stream", "tloam_get_info", "tloam_get_grid_info", "tloam_debug_state", "tloam_debug_partials", "tloam_debug_se3",
    "tloam_debug_raise_fault",
    "tloam_submap_default_config", "tloam_submap_init", "tloam_submap_update", "tloam_get_target",
    "tloam_feature_default_config", "tloam_pca_info", "tloam_extract_planar_sphere",
    "tloam_seg_default_config", "tloam_segment", "tloam_voxel_down_sample", "tloam_odom_default_config",
    "tloam_odometry_reset", "tloam_odometry_frame", "tloam_map_default_config", "tloam_map_configure", "tloam_map_get_info",
    "tloam_map_read", "tloam_registered_scan", "tloam_voxel_map_default_config", "tloam_voxel_map_configure",
    "tloam_voxel_map_get_info", "tloam_voxel_map_read", "tloam_voxel_map_read_box", "tloam_deskew_default_config",
    "tloam_deskew_configure", "tloam_deskew_get_info", "tloam_odometry_frame_timed", "tloam_deskew_scan", "tloam_place_default_config",
    "tloam_place_configure", "tloam_place_get_info", "tloam_place_read_keyframes", "tloam_place_read_loops", "tloam_place_add_scan",
    "tloam_place_describe", "tloam_loop_default_config", "tloam_loop_configure", "tloam_loop_get_info",
    "tloam_place_set_keyframe_clouds", "tloam_place_read_keyframe_clouds", "tloam_loop_verify_pending", "tloam_loop_verify_pair",
    "tloam_loop_read_constraints", "tloam_graph_default_config", "tloam_graph_configure", "tloam_graph_solve", "tloam_graph_optimize",
    "tloam_graph_read_poses", "tloam_graph_correct_pose", "tloam_graph_robust_default_config", "tloam_graph_robust_configure",
    "tloam_graph_solve_robust", "tloam_graph_read_loop_scales", "tloam_graph_get_robust_info", "tloam_closed_map_default_config", "tloam_closed_map_configure",
    "tloam_closed_map_get_info", "tloam_closed_map_build", "tloam_closed_map_read", "tloam_closed_map_read_box",
    "tloam_closed_map_read_poses", "tloam_closed_map_extend", "tloam_closed_map_get_extend_info",
    "tloam_closed_map_carve_default_config", "tloam_closed_map_carve_configure",
    "tloam_closed_map_get_carve_info", "tloam_closed_map_carve", "tloam_closed_map_read_misses", "tloam_closed_map_read_carved",
    "tloam_closed_map_surfel_default_config", "tloam_closed_map_surfel_configure", "tloam_closed_map_get_surfel_info",
    "tloam_closed_map_surfels", "tloam_closed_map_read_moments", "tloam_closed_map_read_surfels", "tloam_closed_map_read_surfels_box",
    "tloam_closed_map_localise_default_config", "tloam_closed_map_localise_configure", "tloam_closed_map_localise",
    "tloam_closed_map_localise_log", "tloam_closed_map_linearise", "tloam_closed_map_localise_batch",
    "tloam_closed_map_localise_batch_log", "tloam_closed_map_relocalise_default_config", "tloam_closed_map_relocalise_configure",
    "tloam_closed_map_relocalise", "tloam_closed_map_relocalise_hypotheses",
    "tloam_closed_map_diff_default_config", "tloam_closed_map_diff_configure", "tloam_closed_map_get_diff_info",
    "tloam_closed_map_diff", "tloam_closed_map_read_diff", "tloam_closed_map_read_gone",
    "tloam_closed_map_raycast_default_config", "tloam_closed_map_raycast_configure", "tloam_closed_map_get_raycast_info",
    "tloam_closed_map_raycast",
    "tloam_closed_map_free_default_config", "tloam_closed_map_free_configure", "tloam_closed_map_get_free_info",
    "tloam_closed_map_free_reset", "tloam_closed_map_free_add_keyframes", "tloam_closed_map_free_add_scan",
    "tloam_closed_map_occupancy", "tloam_closed_map_read_free", "tloam_closed_map_free_columns",
    "tloam_closed_map_read_free_words",
    "tloam_closed_map_save_size", "tloam_closed_map_save", "tloam_closed_map_probe", "tloam_closed_map_load",
    "tloam_rccl_unique_id", "tloam_comm_init_rccl",
    "tloam_comm_mailbox_export", "tloam_comm_init_mailbox",
    "tloam_comm_init_callback", "tloam_shard_range", "tloam_shard_ranges_frame", "tloam_se3_exp", "tloam_se3_log", "tloam_se3_plus",
)


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _lp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64))


def _u8p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))


def _per_point(n, want_ids):
    """the per-point outputs of a scan query, never empty -> (bytes (max(n, 1),) uint8, ids (max(n, 1),) int32 or None, cut);
    cut(a): the first n of `a` as the caller's own copy (None stays None)"""
    return (np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int32) if want_ids else None,
            lambda a: None if a is None else a[:n].copy())


def _box(lo, hi):
    """the two corners of a box read, both or neither -> ((3,) float64, (3,) float64) or (None, None)"""
    if (lo is None) != (hi is None):
        raise ValueError("lo and hi go together")
    if lo is None:
        return None, None
    return np.ascontiguousarray(lo, dtype=np.float64).reshape(3), np.ascontiguousarray(hi, dtype=np.float64).reshape(3)


def _aos(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, 3))


def _colmajor(T):
    return np.ascontiguousarray(np.asarray(T, dtype=np.float64).T).reshape(-1)


def _id_range(first, count, total):
    """ids [first, first + count) of a list of total() entries (asked only when count is None: to the end) -> (first, count)"""
    first = int(first)
    return first, int(max(total() - first, 0) if count is None else count)


def _strict_config(cls, default_fn, over, coerce=None):
    """`cls` as the library's `default_fn` fills it, then the keyword overrides (passed through `coerce[name]` where it has
    one); a name the struct does not have raises KeyError."""
    cfg = cls()
    getattr(load_library(), default_fn)(C.byref(cfg))
    for k, v in over.items():
        if not hasattr(cfg, k):
            raise KeyError(k)
        if coerce and k in coerce:
            v = coerce[k](v)
        setattr(cfg, k, v)
    return cfg


def default_config(**over) -> TlsConfig:
    return _strict_config(TlsConfig, "tloam_default_config", over)


def shard_range(n, rank, nranks):
    lo, hi = C.c_size_t(0), C.c_size_t(0)
    load_library().tloam_shard_range(C.c_size_t(n), int(rank), int(nranks), C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def shard_ranges_frame(n4, rank, nranks):
    """[(lo, hi)] x 4: the blocks of a whole Frame a sharded context keeps (tloam_shard_ranges_frame)."""
    n = (C.c_size_t * 4)(*[int(v) for v in n4])
    lo, hi = (C.c_size_t * 4)(), (C.c_size_t * 4)()
    load_library().tloam_shard_ranges_frame(n, int(rank), int(nranks), lo, hi)
    return [(int(lo[k]), int(hi[k])) for k in range(4)]


def closed_map_probe(blob) -> dict:
    """what a closed map snapshot says it holds, from its header and section table alone (host only: no context, no GPU);
    raises TloamHipError when they do not hold"""
    blob = bytes(blob)
    info = ClosedMapSnapshotInfo()
    rc = load_library().tloam_closed_map_probe(blob, len(blob), C.byref(info))
    if rc:
        raise TloamHipError(f"tloam_closed_map_probe: {STATUS.get(rc, rc)}")
    return info.as_dict()


def se3_exp(x):
    T = np.zeros(16)
    rc = load_library().tloam_se3_exp(_dp(np.ascontiguousarray(x, float)), _dp(T))
    if rc:
        raise TloamHipError(STATUS.get(rc, rc))
    return T.reshape(4, 4).T.copy()


def se3_log(T):
    x = np.zeros(6)
    rc = load_library().tloam_se3_log(_dp(_colmajor(T)), _dp(x))
    if rc:
        raise TloamHipError(STATUS.get(rc, rc))
    return x


def se3_plus(x, delta):
    o = np.zeros(6)
    load_library().tloam_se3_plus(_dp(np.ascontiguousarray(x, float)), _dp(np.ascontiguousarray(delta, float)), _dp(o))
    return o


class HipRegistration:
    """MI355X-native drop-in for tloam::LocalRegistration behind RegistrationInterface."""

    def __init__(self, cfg: TlsConfig | None = None, device: int = 0):
        self.L = load_library()
        self.cfg = cfg if cfg is not None else default_config()
        self.h = C.c_void_p()
        rc = self.L.tloam_create(C.byref(self.cfg), int(device), C.byref(self.h))
        if rc != 0:
            raise TloamHipError(f"tloam_create: {STATUS.get(rc, rc)} -- a gfx950 (MI355X) device is required; "
                                "this path has no CPU fallback")
        self._n = {}
        self._cb = None
        # marshalling buffers of scan_match (column-major 4x4 in / out), allocated once: the binding adds ~3 us per
        # call instead of ~10
        self._pred_buf, self._res_buf = (C.c_double * 16)(), (C.c_double * 16)()
        self._pred_view = np.frombuffer(self._pred_buf).reshape(4, 4).T
        self._res_view = np.frombuffer(self._res_buf).reshape(4, 4).T

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.L.tloam_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self.L.tloam_last_error(self.h)
            raise TloamHipError(f"{what}: {STATUS.get(rc, rc)} {msg.decode() if msg else ''}")

    # ---- RegistrationInterface ------------------------------------------------------------
    def _note(self, rc, what):
        """entry points whose status the caller inspects (they do not raise): a HIP / exchange failure leaves its text on stderr"""
        if rc in (-4, -5):
            sys.stderr.write(f"[tloam_amd] {what}: {STATUS.get(rc, rc)}: {self.L.tloam_last_error(self.h).decode(errors='replace')}\n")
        return rc

    def _read_list(self, fn, name, rec_type, *head):
        """a list getter's two calls, fn(*head, capacity, n, records): the count, then the records -> [dict]"""
        n = C.c_size_t(0)
        self._check(fn(*head, 0, C.byref(n), None), name)
        if not n.value:
            return []
        rec = (rec_type * n.value)()
        self._check(fn(*head, n.value, C.byref(n), rec), name)
        return [r.as_dict() for r in rec[: n.value]]

    def _read_box(self, fn, name, head, columns):
        """a box read's two calls, fn(*head, capacity, n, *columns): the probe for the count (a short capacity, -1, with n > 0 is
        its answer), then the columns -- (width, or None for a vector; dtype float64 or int64) each -- fetched and trimmed"""
        n = C.c_size_t(0)
        rc = fn(*head, 0, C.byref(n), *[None] * len(columns))
        if rc not in (0, -1) or (rc == -1 and n.value == 0):
            self._check(rc, name)
        m = n.value
        cols = [np.zeros((max(m, 1), w) if w else max(m, 1), dt) for w, dt in columns]
        if m:
            self._check(fn(*head, m, C.byref(n), *[_dp(a) if a.dtype == np.float64 else _lp(a) for a in cols]), name)
        return tuple(a[: n.value].copy() for a in cols)

    def _frame_call(self, fn, name, tag, frame):
        clouds = [_aos(frame.cloud(k)) for k in range(4)]
        ptrs = (C.POINTER(C.c_double) * 4)(*[_dp(a) for a in clouds])
        ns = (C.c_size_t * 4)(*[len(a) for a in clouds])
        for k in range(4):
            self._n[(tag, k)] = len(clouds[k])
        self._check(fn(self.h, ptrs, ns), name)
        return True

    def set_input_source(self, frame) -> bool:
        """setInputSource (registration.cpp:232-239): the four clouds of the Frame in one call."""
        return self._frame_call(self.L.tloam_set_source_frame, "tloam_set_source_frame", "s", frame)

    def set_input_target(self, frame) -> bool:
        """setInputTarget (registration.cpp:241-248)."""
        return self._frame_call(self.L.tloam_set_target_frame, "tloam_set_target_frame", "t", frame)

    def scan_matching(self, predict_pose, omega_perturb=None, scan_cloud=None):
        """scanMatching (registration.cpp:879-1133) -> (True, result_pose 4x4).  `scan_cloud`
        ((n,3) float64, C-contiguous) is transformed in place like out_result_.scan_cloud."""
        rc, T, st = self.scan_match(predict_pose, omega_perturb, scan_cloud)
        self._check(rc, "tloam_scan_match")
        self.last_stats = st
        return True, T

    def get_fitness_score(self):
        """getFitnessScore (registration.cpp:257-296)."""
        f, r = C.c_double(0), C.c_double(0)
        self._check(self.L.tloam_fitness(self.h, C.byref(f), C.byref(r)), "tloam_fitness")
        return f.value, r.value

    # ---- C ABI, one to one --------------------------------------------------------------------
    def set_source(self, kind, xyz):
        a = _aos(xyz)
        self._n[("s", kind)] = len(a)
        rc = self.L.tloam_set_source(self.h, int(kind), _dp(a), len(a))
        self._check(rc, "tloam_set_source")
        return rc

    def set_target(self, kind, xyz):
        a = _aos(xyz)
        self._n[("t", kind)] = len(a)
        rc = self.L.tloam_set_target(self.h, int(kind), _dp(a), len(a))
        self._check(rc, "tloam_set_target")
        return rc

    def set_frames(self, source, target):
        self.set_input_source(source)
        self.set_input_target(target)

    def frame_stash(self, slot):
        """tloam_frame_stash: the registered clouds move into slot `slot` of the HBM frame store."""
        self._check(self.L.tloam_frame_stash(self.h, int(slot)), "tloam_frame_stash")

    def frame_select(self, slot):
        """tloam_frame_select: the clouds of `slot` become the registered ones (-1: the context's own); O(1)."""
        rc = self.L.tloam_frame_select(self.h, int(slot))
        if rc != 0:
            self._check(rc, "tloam_frame_select")

    def scan_match(self, predict, omega=None, scan=None):
        self._pred_view[...] = predict
        self._res_view[...] = 0.0
        st = Stats()
        om = None if omega is None else np.ascontiguousarray(omega, float)
        if scan is not None:
            assert scan.dtype == np.float64 and scan.flags.c_contiguous
        rc = self.L.tloam_scan_match(self.h, self._pred_buf, _dp(om), self._res_buf, _dp(scan),
                                     0 if scan is None else len(scan), C.byref(st))
        self._note(rc, "tloam_scan_match")
        return rc, self._res_view.copy(), st.as_dict()

    def sm_begin(self, predict, omega=None):
        om = None if omega is None else np.ascontiguousarray(omega, float)
        return self._note(self.L.tloam_sm_begin(self.h, _dp(_colmajor(predict)), _dp(om)), "tloam_sm_begin")

    def sm_outer(self):
        done = C.c_int(0)
        st = Stats()
        rc = self._note(self.L.tloam_sm_outer(self.h, C.byref(done), C.byref(st)), "tloam_sm_outer")
        return rc, bool(done.value), st.as_dict()

    def sm_end(self):
        res = np.zeros(16)
        st = Stats()
        rc = self._note(self.L.tloam_sm_end(self.h, _dp(res), C.byref(st)), "tloam_sm_end")
        return rc, res.reshape(4, 4).T.copy(), st.as_dict()

    # ---- device-resident submap (FrontEnd::updateSubmap, front_end.cpp:201-275 / :283-304)
    def submap_init(self, planar, sphere, edge, ground, cfg: SubmapConfig | None = None):
        cl = [_aos(x) for x in (planar, sphere, edge, ground)]
        args = []
        for a in cl:
            args += [_dp(a), len(a)]
        rc = self.L.tloam_submap_init(self.h, C.byref(cfg) if cfg is not None else None, *args)
        self._check(rc, "tloam_submap_init")
        return rc

    def submap_update(self, pose, planar, sphere, edge, ground):
        m = np.ascontiguousarray(np.asarray(pose, float).reshape(4, 4).T.ravel())  # column-major
        cl = [_aos(x) for x in (planar, sphere, edge, ground)]
        args = []
        for a in cl:
            args += [_dp(a), len(a)]
        rc = self.L.tloam_submap_update(self.h, _dp(m), *args)
        self._check(rc, "tloam_submap_update")
        return rc

    def get_target(self, kind):
        n = C.c_size_t(0)
        self.L.tloam_get_target(self.h, int(kind), 0, C.byref(n), None)
        out = np.zeros((max(n.value, 1), 3))
        if n.value:
            self._check(self.L.tloam_get_target(self.h, int(kind), n.value, C.byref(n), _dp(out)), "tloam_get_target")
        self._n[("t", kind)] = n.value
        return out[: n.value].copy()

    # ---- PCA feature extraction (featureExtract::calculatePCAInfo / extractPlanarSphere)
    def pca_info(self, xyz, cfg: FeatureConfig | None = None):
        cfg = cfg or default_feature_config()
        a = _aos(xyz)
        n, K = len(a), cfg.K
        out = dict(flatness=np.zeros(n), cvr=np.zeros(n), sphericity=np.zeros(n), normal=np.zeros((max(n, 1), 3)),
                   num_sum=np.zeros(n, np.int32), neigh=np.zeros((max(n, 1), K), np.int32))
        rc = self.L.tloam_pca_info(self.h, C.byref(cfg), _dp(a), n, _dp(out["flatness"]), _dp(out["cvr"]),
                                   _dp(out["sphericity"]), _dp(out["normal"]), _ip(out["num_sum"]), _ip(out["neigh"]))
        self._check(rc, "tloam_pca_info")
        out["normal"] = out["normal"][:n]
        out["neigh"] = out["neigh"][:n]
        return out

    def extract_planar_sphere(self, xyz, cfg: FeatureConfig | None = None):
        """-> (planar_scan_index, planar_submap_index, sphere_scan_index, sphere_submap_index)"""
        cfg = cfg or default_feature_config()
        a = _aos(xyz)
        n = len(a)
        lists = [np.zeros(max(n, 1), np.int32) for _ in range(4)]
        cnt = [C.c_size_t(0) for _ in range(4)]
        args = []
        for l, k in zip(lists, cnt):
            args += [_ip(l), C.byref(k)]
        rc = self.L.tloam_extract_planar_sphere(self.h, C.byref(cfg), _dp(a), n, *args)
        self._check(rc, "tloam_extract_planar_sphere")
        return tuple(l[: k.value].copy() for l, k in zip(lists, cnt))

    # ---- segmentation node (Segmentation::spinOnce, segmentation.cpp:40-93)
    def segment(self, xyz, cfg: SegConfig | None = None):
        """one raw scan -> dict: status (0, or -2 when the node publishes nothing), ring (per input point, -1 filtered),
        ground, object, segmented + label, edge, general (index lists into `xyz`), boxes (clusters x 6).  Raises on
        any other status."""
        cfg = cfg or default_seg_config()
        a = _aos(xyz)
        n = len(a)
        m = max(n, 1)
        ring = np.zeros(m, np.int32)
        lists = {k: np.zeros(m, np.int32) for k in ("ground", "object", "segmented", "label", "edge", "general")}
        boxes = np.zeros((m, 6))
        cnt = {k: C.c_size_t(0) for k in ("ground", "object", "segmented", "edge", "general", "boxes")}
        rc = self.L.tloam_segment(self.h, C.byref(cfg), _dp(a), n, _ip(ring), _ip(lists["ground"]), C.byref(cnt["ground"]),
                                  _ip(lists["object"]), C.byref(cnt["object"]), _ip(lists["segmented"]), _ip(lists["label"]),
                                  C.byref(cnt["segmented"]), _ip(lists["edge"]), C.byref(cnt["edge"]), _ip(lists["general"]),
                                  C.byref(cnt["general"]), _dp(boxes), m, C.byref(cnt["boxes"]))
        if rc not in (0, -2):
            self._check(rc, "tloam_segment")
        out = {"status": rc, "ring": ring[:n].copy()}
        for k in ("ground", "object", "segmented", "edge", "general"):
            out[k] = lists[k][: cnt[k].value].copy()
        out["label"] = lists["label"][: cnt["segmented"].value].copy()
        out["boxes"] = boxes[: cnt["boxes"].value].copy()
        return out

    # ---- per-scan voxel grid and the whole odometry frame (FrontEnd::updateLidarOdometry, front_end.cpp:278-337)
    def voxel_down_sample(self, xyz, voxel):
        """PointCloud2::VoxelDownSample on the device: voxel means in order of first occurrence.  Raises on
        TLOAM_E_INVALID (voxel <= 0, voxel too small)."""
        a = _aos(xyz)
        out = np.zeros((max(len(a), 1), 3))
        n = C.c_size_t(0)
        rc = self.L.tloam_voxel_down_sample(self.h, float(voxel), _dp(a), len(a), _dp(out), len(out), C.byref(n))
        self._check(rc, "tloam_voxel_down_sample")
        return out[: n.value].copy()

    def odometry_reset(self, init_pose=None, cfg: OdomConfig | None = None):
        """FrontEnd::setInitPose + a fresh odometry state (the next frame is the first one)."""
        T = None if init_pose is None else _colmajor(init_pose)
        self._check(self.L.tloam_odometry_reset(self.h, C.byref(cfg) if cfg is not None else None, _dp(T)),
                    "tloam_odometry_reset")

    def odometry_frame(self, xyz, times=None):
        """one raw scan -> (rc, pose 4x4, stats dict).  rc: 0, -2 (TLOAM_E_TOO_FEW_POINTS: the frame is skipped) or
        -7 (TLOAM_E_WEIGHT_RANGE: pose written, as scan_match); raises on any other status.  times: per-point seconds relative
        to the pose's instant -- tloam_odometry_frame_timed (deskew configured with time_source 1)."""
        a = _aos(xyz)
        T = np.zeros(16)
        st = OdomStats()
        if times is None:
            rc = self.L.tloam_odometry_frame(self.h, _dp(a), len(a), _dp(T), C.byref(st))
        else:
            t = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
            if len(t) != len(a):
                raise ValueError(f"{len(t)} times for {len(a)} points")
            rc = self.L.tloam_odometry_frame_timed(self.h, _dp(a), _dp(t), len(a), _dp(T), C.byref(st))
        if rc not in (0, -2, -7):
            self._check(rc, "tloam_odometry_frame_timed" if times is not None else "tloam_odometry_frame")
        if rc != -2 and st.frame > 0:   # the getters' capacities: this frame's source clouds, in kind order
            for k, m in enumerate((st.n_planar_scan, st.n_ground_ds, st.n_edge_ds, st.n_sphere_scan)):
                self._n[("s", k)] = int(m)
        return rc, T.reshape(4, 4).T.copy(), st.as_dict()

    # ---- the global map and the registered scan (FrontEnd::spinOnce :84-92, updateSubmap :269-274)
    def map_configure(self, cfg: MapConfig | None = None, **over):
        """mapping on / off (default_map_config(**over) when cfg is None); empties the map.  Kept across odometry_reset."""
        cfg = cfg if cfg is not None else default_map_config(**over)
        self._check(self.L.tloam_map_configure(self.h, C.byref(cfg)), "tloam_map_configure")

    def map_info(self) -> dict:
        info = MapInfo()
        self._check(self.L.tloam_map_get_info(self.h, C.byref(info)), "tloam_map_get_info")
        return info.as_dict()

    def map_read(self, first=0, count=None):
        """points [first, first + count) of the global map as an (m, 3) float64 array (count None: to the end)"""
        first, m = _id_range(first, count, lambda: self.map_info()["n_points"])
        out = np.zeros((max(m, 1), 3))
        self._check(self.L.tloam_map_read(self.h, first, m, _dp(out)), "tloam_map_read")
        return out[:m].copy()

    def registered_scan(self):
        """the last accepted frame's raw scan transformed by its pose (/raw_cloud, front_end.cpp:84-86) as (n, 3)"""
        n = C.c_size_t(0)
        rc = self.L.tloam_registered_scan(self.h, 0, C.byref(n), None)
        if rc not in (0, -1) or (rc == -1 and n.value == 0):
            self._check(rc, "tloam_registered_scan")
        out = np.zeros((max(n.value, 1), 3))
        self._check(self.L.tloam_registered_scan(self.h, n.value, C.byref(n), _dp(out)), "tloam_registered_scan")
        return out[: n.value].copy()

    # ---- the merged voxel map
    def voxel_map_configure(self, cfg: VoxelMapConfig | None = None, **over):
        """voxel map on / off (default_voxel_map_config(**over) when cfg is None); empties it.  Kept across odometry_reset."""
        cfg = cfg if cfg is not None else default_voxel_map_config(**over)
        self._check(self.L.tloam_voxel_map_configure(self.h, C.byref(cfg)), "tloam_voxel_map_configure")

    def voxel_map_info(self) -> dict:
        info = VoxelMapInfo()
        self._check(self.L.tloam_voxel_map_get_info(self.h, C.byref(info)), "tloam_voxel_map_get_info")
        return info.as_dict()

    def voxel_map_read(self, first=0, count=None):
        """voxels [first, first + count) in id order -> (centroids (m, 3) float64, counts (m,) int64); count None: to the end"""
        first, m = _id_range(first, count, lambda: self.voxel_map_info()["n_voxels"])
        cen, cnt = np.zeros((max(m, 1), 3)), np.zeros(max(m, 1), np.int64)
        self._check(self.L.tloam_voxel_map_read(self.h, int(first), m, _dp(cen), _lp(cnt)), "tloam_voxel_map_read")
        return cen[:m].copy(), cnt[:m].copy()

    def voxel_map_read_box(self, lo, hi, min_count=1):
        """the voxels whose centroid lies in [lo, hi] (inclusive, every axis) with N >= min_count, in id order ->
        (centroids (m, 3), counts (m,))"""
        lo = np.ascontiguousarray(lo, dtype=np.float64).reshape(3)
        hi = np.ascontiguousarray(hi, dtype=np.float64).reshape(3)
        return self._read_box(self.L.tloam_voxel_map_read_box, "tloam_voxel_map_read_box", (self.h, _dp(lo), _dp(hi), int(min_count)),
                              [(3, np.float64), (None, np.int64)])

    # ---- deskew of the frame's scan under constant velocity
    def deskew_configure(self, cfg: DeskewConfig | None = None, **over):
        """deskew on / off (default_deskew_config(**over) when cfg is None).  Kept across odometry_reset."""
        cfg = cfg if cfg is not None else default_deskew_config(**over)
        self._check(self.L.tloam_deskew_configure(self.h, C.byref(cfg)), "tloam_deskew_configure")

    def deskew_info(self) -> dict:
        info = DeskewInfo()
        self._check(self.L.tloam_deskew_get_info(self.h, C.byref(info)), "tloam_deskew_get_info")
        return info.as_dict()

    def deskew_scan(self, xyz, motion, cfg: DeskewConfig | None = None, scan_period=0.1, times=None):
        """the correction alone, on the device: (n, 3) scan, motion = the step (4x4 rigid), times in seconds (timed mode) ->
        the deskewed (n, 3) scan"""
        cfg = cfg if cfg is not None else default_deskew_config(enabled=1, time_source=0 if times is None else 1)
        a = _aos(xyz)
        t = None if times is None else np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
        if t is not None and len(t) != len(a):
            raise ValueError(f"{len(t)} times for {len(a)} points")
        out = np.zeros((max(len(a), 1), 3))
        M = _colmajor(motion)
        self._check(self.L.tloam_deskew_scan(self.h, C.byref(cfg), float(scan_period), _dp(M), _dp(a), _dp(t), len(a),
                                             _dp(out)), "tloam_deskew_scan")
        return out[: len(a)].copy()

    # ---- place recognition: Scan Context keyframes and loop search
    def place_configure(self, cfg: PlaceConfig | None = None, **over):
        """place recognition on / off (default_place_config(**over) when cfg is None); empties the keyframe database.  Kept
        across odometry_reset (which empties the database too)."""
        cfg = cfg if cfg is not None else default_place_config(**over)
        self._check(self.L.tloam_place_configure(self.h, C.byref(cfg)), "tloam_place_configure")
        self._place_cfg = cfg

    def _place_grid(self):
        cfg = getattr(self, "_place_cfg", None) or default_place_config()
        return int(cfg.n_rings), int(cfg.n_sectors)

    def place_info(self) -> dict:
        """keyframes, loops (this waits for the device's work in flight), the last keyframe's frame, capacity"""
        info = PlaceInfo()
        self._check(self.L.tloam_place_get_info(self.h, C.byref(info)), "tloam_place_get_info")
        return info.as_dict()

    def place_add_scan(self, xyz, pose, frame_id=-1) -> int:
        """one scan (sensor frame) with the caller's pose (4x4), added as a keyframe and searched -> its keyframe id"""
        a = _aos(xyz)
        M = _colmajor(pose)
        kf = C.c_int64(-1)
        self._check(self.L.tloam_place_add_scan(self.h, _dp(a), len(a), _dp(M), int(frame_id), C.byref(kf)),
                    "tloam_place_add_scan")
        return int(kf.value)

    def place_describe(self, xyz, cfg: PlaceConfig | None = None):
        """the Scan Context of one scan -> (descriptor (n_rings, n_sectors), ring_key, sector_key); cfg None: the context's"""
        R, S = (int(cfg.n_rings), int(cfg.n_sectors)) if cfg is not None else self._place_grid()
        a = _aos(xyz)
        d, rk, sk = np.zeros((R, S)), np.zeros(R), np.zeros(S)
        self._check(self.L.tloam_place_describe(self.h, C.byref(cfg) if cfg is not None else None, _dp(a), len(a), _dp(d),
                                                _dp(rk), _dp(sk)), "tloam_place_describe")
        return d, rk, sk

    def place_read_keyframes(self, first=0, count=None) -> dict:
        """keyframes [first, first + count) -> frames (m,), poses (m, 4, 4), ring_keys (m, R), sector_keys (m, S),
        descriptors (m, R, S)"""
        R, S = self._place_grid()
        first, m = _id_range(first, count, lambda: self.place_info()["n_keyframes"])
        fr, P = np.zeros(max(m, 1), np.int64), np.zeros((max(m, 1), 16))
        rk, sk, d = np.zeros((max(m, 1), R)), np.zeros((max(m, 1), S)), np.zeros((max(m, 1), R, S))
        self._check(self.L.tloam_place_read_keyframes(self.h, int(first), m, _lp(fr), _dp(P), _dp(rk), _dp(sk), _dp(d)),
                    "tloam_place_read_keyframes")
        return {"frames": fr[:m].copy(), "poses": P[:m].reshape(m, 4, 4).transpose(0, 2, 1).copy(), "ring_keys": rk[:m].copy(),
                "sector_keys": sk[:m].copy(), "descriptors": d[:m].copy()}

    def place_loops(self, first=0, count=None) -> list:
        """loop records [first, first + count) in the order they were found, as dicts"""
        first, m = _id_range(first, count, lambda: self.place_info()["n_loops"])
        buf = (PlaceLoop * max(m, 1))()
        self._check(self.L.tloam_place_read_loops(self.h, int(first), m, buf), "tloam_place_read_loops")
        return [buf[i].as_dict() for i in range(m)]

    # ---- loop verification: keyframe clouds and a two-stage TLS match
    def loop_configure(self, cfg: LoopConfig | None = None, **over):
        """loop verification on / off (default_loop_config(**over) when cfg is None); empties the keyframe database, its clouds
        and the constraints.  Kept across odometry_reset (which empties them too)."""
        cfg = cfg if cfg is not None else default_loop_config(**over)
        self._check(self.L.tloam_loop_configure(self.h, C.byref(cfg)), "tloam_loop_configure")

    def loop_info(self) -> dict:
        """constraints, accepted ones, the points the keyframe clouds take and the arena's capacity"""
        info = LoopInfo()
        self._check(self.L.tloam_loop_get_info(self.h, C.byref(info)), "tloam_loop_get_info")
        return info.as_dict()

    def place_set_keyframe_clouds(self, keyframe, src=None, tgt=None):
        """a keyframe's clouds from the caller: src / tgt are four (n, 3) clouds by kind, or None to leave that side"""
        def side(clouds):
            if clouds is None:
                return None, None, []
            a = [_aos(x) for x in clouds]
            assert len(a) == 4
            return (dp * 4)(*[_dp(x) for x in a]), (C.c_size_t * 4)(*[len(x) for x in a]), a
        dp = C.POINTER(C.c_double)
        sp, sn, keep_s = side(src)
        tp, tn, keep_t = side(tgt)
        self._check(self.L.tloam_place_set_keyframe_clouds(self.h, int(keyframe), sp, sn, tp, tn),
                    "tloam_place_set_keyframe_clouds")
        del keep_s, keep_t

    def place_read_keyframe_clouds(self, keyframe, side=None, kind=None):
        """one stored cloud (side 0 source / 1 target, kind TLOAM_KIND_*) as (n, 3); side None: [[4 source], [4 target]]"""
        if side is None:
            return [[self.place_read_keyframe_clouds(keyframe, s, k) for k in range(4)] for s in range(2)]
        n = C.c_size_t(0)
        self._check(self.L.tloam_place_read_keyframe_clouds(self.h, int(keyframe), int(side), int(kind), 0, C.byref(n), None),
                    "tloam_place_read_keyframe_clouds")
        out = np.zeros((max(n.value, 1), 3))
        self._check(self.L.tloam_place_read_keyframe_clouds(self.h, int(keyframe), int(side), int(kind), n.value, C.byref(n),
                                                            _dp(out)), "tloam_place_read_keyframe_clouds")
        return out[: n.value].copy()

    def loop_verify_pending(self) -> int:
        """verifies every loop record not verified yet (one constraint each) -> how many"""
        n = C.c_int64(0)
        self._check(self.L.tloam_loop_verify_pending(self.h, C.byref(n)), "tloam_loop_verify_pending")
        return int(n.value)

    def loop_verify_pair(self, query, match, init=None) -> dict:
        """one pair from the caller's initial guess (4x4; None: rigid_inverse(P_m) P_q); not appended"""
        out = LoopConstraint()
        M = None if init is None else _colmajor(init)
        self._check(self.L.tloam_loop_verify_pair(self.h, int(query), int(match), _dp(M), C.byref(out)),
                    "tloam_loop_verify_pair")
        return out.as_dict()

    def loop_constraints(self, first=0, count=None) -> list:
        """constraints [first, first + count) as dicts"""
        first, m = _id_range(first, count, lambda: self.loop_info()["n_constraints"])
        buf = (LoopConstraint * max(m, 1))()
        self._check(self.L.tloam_loop_read_constraints(self.h, int(first), m, buf), "tloam_loop_read_constraints")
        return [buf[i].as_dict() for i in range(m)]

    # ---- pose-graph optimisation of the keyframes
    def graph_configure(self, cfg: GraphConfig | None = None, **over):
        """the context's graph configuration (default_graph_config(**over) when cfg is None); drops the corrected poses.  Kept
        across odometry_reset."""
        cfg = cfg if cfg is not None else default_graph_config(**over)
        self._check(self.L.tloam_graph_configure(self.h, C.byref(cfg)), "tloam_graph_configure")

    @staticmethod
    def _graph_arrays(poses, i, j, Z, w):
        """-> (poses column-major (n, 4, 4), number of edges, the tloam_graph_edge array)"""
        P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1))
        Zc = np.asarray(Z, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1).reshape(-1, 16)
        wv = np.asarray(w, np.float64).reshape(-1, 6)
        m = len(Zc)
        edges = (GraphEdge * max(m, 1))()
        if m:
            rec = np.frombuffer(edges, dtype=np.dtype([("i", np.int64), ("j", np.int64), ("Z", np.float64, 16),
                                                       ("w", np.float64, 6)]), count=m)
            rec["i"], rec["j"], rec["Z"], rec["w"] = np.asarray(i, np.int64), np.asarray(j, np.int64), Zc, wv
        return P, m, edges

    def graph_solve(self, poses, i, j, Z, w, cfg: GraphConfig | None = None):
        """the caller's graph: poses (n, 4, 4); edges i, j (m,), Z (m, 4, 4), w (m, 6), the first n - 1 the chain ->
        (poses (n, 4, 4), info dict); cfg None: the context's configuration"""
        P, m, edges = self._graph_arrays(poses, i, j, Z, w)
        out = np.zeros_like(P)
        info = GraphInfo()
        self._check(self.L.tloam_graph_solve(self.h, C.byref(cfg) if cfg is not None else None, len(P), _dp(P), m, edges,
                                             _dp(out), C.byref(info)), "tloam_graph_solve")
        return out.transpose(0, 2, 1).copy(), info.as_dict()

    # ---- its robust mode: GNC-TLS on the loop edges
    def graph_robust_configure(self, cfg: GraphRobustConfig | None = None, **over):
        """the context's robust configuration (default_graph_robust_config(**over) when cfg is None: off unless enabled=1);
        drops the corrected poses.  Kept across odometry_reset."""
        cfg = cfg if cfg is not None else default_graph_robust_config(**over)
        self._check(self.L.tloam_graph_robust_configure(self.h, C.byref(cfg)), "tloam_graph_robust_configure")

    def graph_solve_robust(self, poses, i, j, Z, w, cfg: GraphConfig | None = None, rcfg: GraphRobustConfig | None = None):
        """graph_solve with the robust mode -> (poses (n, 4, 4), info dict of the last inner solve, robust info dict, the loop
        edges' scales (m - (n - 1),), their statistics r); cfg / rcfg None: the context's configurations"""
        P, m, edges = self._graph_arrays(poses, i, j, Z, w)
        nl = max(m - (len(P) - 1), 0)
        out = np.zeros_like(P)
        scale, chi2 = np.zeros(max(nl, 1)), np.zeros(max(nl, 1))
        info, rinfo = GraphInfo(), GraphRobustInfo()
        self._check(self.L.tloam_graph_solve_robust(self.h, C.byref(cfg) if cfg is not None else None,
                                                    C.byref(rcfg) if rcfg is not None else None, len(P), _dp(P), m, edges, _dp(out),
                                                    C.byref(info), C.byref(rinfo), _dp(scale), _dp(chi2)), "tloam_graph_solve_robust")
        return out.transpose(0, 2, 1).copy(), info.as_dict(), rinfo.as_dict(), scale[:nl].copy(), chi2[:nl].copy()

    def graph_read_loop_scales(self, first=0, count=None):
        """the loop edges [first, first + count) of the last graph_optimize -> (constraint indices as loop_constraints numbers
        them, scales, statistics r); count None: all of them"""
        first, m = _id_range(first, count, lambda: getattr(self, "_graph_loops", 0))
        idx, scale, chi2 = np.zeros(max(m, 1), np.int64), np.zeros(max(m, 1)), np.zeros(max(m, 1))
        self._check(self.L.tloam_graph_read_loop_scales(self.h, int(first), m, idx.ctypes.data_as(C.POINTER(C.c_int64)), _dp(scale),
                                                        _dp(chi2)), "tloam_graph_read_loop_scales")
        return idx[:m].copy(), scale[:m].copy(), chi2[:m].copy()

    def graph_robust_info(self) -> dict:
        """tloam_graph_get_robust_info: the robust mode's report of the last graph_optimize"""
        info = GraphRobustInfo()
        self._check(self.L.tloam_graph_get_robust_info(self.h, C.byref(info)), "tloam_graph_get_robust_info")
        return info.as_dict()

    def graph_optimize(self) -> dict:
        """optimises the context's graph (keyframe poses, odometry chain, accepted constraints) -> info dict"""
        info = GraphInfo()
        self._check(self.L.tloam_graph_optimize(self.h, C.byref(info)), "tloam_graph_optimize")
        self._graph_n = int(info.n_nodes)   # (how many corrected poses graph_poses reads by default)
        self._graph_loops = int(info.n_loop_edges)
        return info.as_dict()

    def graph_poses(self, first=0, count=None):
        """corrected keyframe poses [first, first + count) of the last graph_optimize, (m, 4, 4); count None: all of them"""
        first, m = _id_range(first, count, lambda: getattr(self, "_graph_n", 0))
        out = np.zeros((max(m, 1), 16))
        self._check(self.L.tloam_graph_read_poses(self.h, int(first), m, _dp(out)), "tloam_graph_read_poses")
        return out[:m].reshape(m, 4, 4).transpose(0, 2, 1).copy()

    def graph_correct_pose(self, keyframe, pose):
        """P'_k rigid_inverse(P_k) pose for a pose taken near keyframe k (-1: the last corrected one)"""
        out = np.zeros(16)
        self._check(self.L.tloam_graph_correct_pose(self.h, int(keyframe), _dp(_colmajor(pose)), _dp(out)),
                    "tloam_graph_correct_pose")
        return out.reshape(4, 4).T.copy()

    # ---- the closed map: the keyframe clouds merged under corrected poses
    def closed_map_configure(self, cfg: ClosedMapConfig | None = None, **over):
        """the closed map's configuration (default_closed_map_config(**over) when cfg is None); empties it.  Kept across
        odometry_reset."""
        cfg = cfg if cfg is not None else default_closed_map_config(**over)
        self._check(self.L.tloam_closed_map_configure(self.h, C.byref(cfg)), "tloam_closed_map_configure")

    def closed_map_build(self, pose_source=1, poses=None) -> dict:
        """builds the closed map from every keyframe's stored clouds, replacing the previous one -> info dict.  pose_source 0: the
        stored keyframe poses, 1: the corrected poses of the last graph_optimize, 2: `poses` (K, 4, 4)"""
        P, n = None, 0
        if poses is not None:
            P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1))
            n = len(P)
        info = ClosedMapInfo()
        self._check(self.L.tloam_closed_map_build(self.h, int(pose_source), _dp(P), n, C.byref(info)), "tloam_closed_map_build")
        return info.as_dict()

    def closed_map_info(self) -> dict:
        info = ClosedMapInfo()
        self._check(self.L.tloam_closed_map_get_info(self.h, C.byref(info)), "tloam_closed_map_get_info")
        return info.as_dict()

    def closed_map_read(self, first=0, count=None):
        """voxels [first, first + count) in id order -> (centroids (m, 3) float64, counts (m,) int64); count None: to the end"""
        first, m = _id_range(first, count, lambda: self.closed_map_info()["n_voxels"])
        cen, cnt = np.zeros((max(m, 1), 3)), np.zeros(max(m, 1), np.int64)
        self._check(self.L.tloam_closed_map_read(self.h, int(first), m, _dp(cen), _lp(cnt)), "tloam_closed_map_read")
        return cen[:m].copy(), cnt[:m].copy()

    def closed_map_read_box(self, lo, hi, min_count=1):
        """the voxels whose centroid lies in [lo, hi] (inclusive, every axis) with N >= min_count, in id order ->
        (centroids (m, 3), counts (m,))"""
        lo = np.ascontiguousarray(lo, dtype=np.float64).reshape(3)
        hi = np.ascontiguousarray(hi, dtype=np.float64).reshape(3)
        return self._read_box(self.L.tloam_closed_map_read_box, "tloam_closed_map_read_box", (self.h, _dp(lo), _dp(hi), int(min_count)),
                              [(3, np.float64), (None, np.int64)])

    def closed_map_poses(self, first=0, count=None):
        """the poses keyframes [first, first + count) were built with, (m, 4, 4); count None: to the end"""
        first, m = _id_range(first, count, lambda: self.closed_map_info()["n_keyframes"])
        out = np.zeros((max(m, 1), 16))
        self._check(self.L.tloam_closed_map_read_poses(self.h, int(first), m, _dp(out)), "tloam_closed_map_read_poses")
        return out[:m].reshape(m, 4, 4).transpose(0, 2, 1).copy()

    # ---- the closed map extended in place by the keyframes added since its build
    def closed_map_extend(self, pose_source=0, poses=None) -> dict:
        """adds the keyframes [info.n_keyframes, n_kf) -- the ones added since the build, the load or the last extend -- to the
        built closed map in place, its surfels and its carve following -> info dict.  pose_source 0: their stored poses, 1: the
        build's rule (corrected poses), 2: `poses` (n_kf - K, 4, 4), of the new keyframes only"""
        P, n = None, 0
        if poses is not None:
            P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1))
            n = len(P)
        info = ClosedMapExtendInfo()
        self._check(self.L.tloam_closed_map_extend(self.h, int(pose_source), _dp(P), n, C.byref(info)), "tloam_closed_map_extend")
        return info.as_dict()

    def closed_map_extend_info(self) -> dict:
        info = ClosedMapExtendInfo()
        self._check(self.L.tloam_closed_map_get_extend_info(self.h, C.byref(info)), "tloam_closed_map_get_extend_info")
        return info.as_dict()

    # ---- the closed map's snapshot: out of this context, into a fresh one
    def closed_map_save(self, clouds=False) -> bytes:
        """the built closed map, its carve and surfels when they exist, the keyframe database and the configurations as one
        blob; clouds: also the keyframes' stored clouds, so that the loaded map can be built, carved and surfelled again"""
        flags = SNAPSHOT_CLOUDS if clouds else 0
        n = C.c_size_t(0)
        self._check(self.L.tloam_closed_map_save_size(self.h, flags, C.byref(n)), "tloam_closed_map_save_size")
        buf = C.create_string_buffer(max(n.value, 1))
        self._check(self.L.tloam_closed_map_save(self.h, flags, buf, n.value, C.byref(n)), "tloam_closed_map_save")
        return buf.raw[:n.value]

    def closed_map_load(self, blob) -> dict:
        """replaces this context's keyframes, loop constraints, corrected poses and closed map by the snapshot's -> what it
        held (closed_map_probe's dict).  A refused blob raises TloamHipError and leaves the context as it was"""
        blob = bytes(blob)
        info = ClosedMapSnapshotInfo()
        self._check(self.L.tloam_closed_map_load(self.h, blob, len(blob), C.byref(info)), "tloam_closed_map_load")
        # (the keyframe getters size their outputs by the place configuration's layout, which is now the snapshot's)
        self._place_cfg = default_place_config(enabled=1, n_rings=int(info.n_rings), n_sectors=int(info.n_sectors))
        return info.as_dict()

    # ---- the carve of the closed map: per voxel, the rays that passed through it
    def closed_map_carve_configure(self, cfg: ClosedMapCarveConfig | None = None, **over):
        """the carve's configuration (default_closed_map_carve_config(**over) when cfg is None); drops the counts, not the closed
        map.  Kept across odometry_reset."""
        cfg = cfg if cfg is not None else default_closed_map_carve_config(**over)
        self._check(self.L.tloam_closed_map_carve_configure(self.h, C.byref(cfg)), "tloam_closed_map_carve_configure")

    def closed_map_carve(self) -> dict:
        """counts, per voxel of the built closed map, the keyframe rays that passed through it -> info dict"""
        info = ClosedMapCarveInfo()
        self._check(self.L.tloam_closed_map_carve(self.h, C.byref(info)), "tloam_closed_map_carve")
        return info.as_dict()

    def closed_map_carve_info(self) -> dict:
        info = ClosedMapCarveInfo()
        self._check(self.L.tloam_closed_map_get_carve_info(self.h, C.byref(info)), "tloam_closed_map_get_carve_info")
        return info.as_dict()

    def closed_map_misses(self, first=0, count=None):
        """M of voxels [first, first + count) in id order, (m,) int64; count None: to the end"""
        first, m = _id_range(first, count, lambda: self.closed_map_info()["n_voxels"])
        out = np.zeros(max(m, 1), np.int64)
        self._check(self.L.tloam_closed_map_read_misses(self.h, int(first), m, _lp(out)), "tloam_closed_map_read_misses")
        return out[:m].copy()

    def closed_map_read_carved(self, lo=None, hi=None, min_count=1, min_miss=3, miss_ratio=1.0):
        """closed_map_read_box's voxels (lo and hi None: the whole map) without those seen through -- M >= min_miss and
        M > miss_ratio * N -- in id order -> (centroids (m, 3), counts (m,), misses (m,))"""
        lo, hi = _box(lo, hi)
        head = (self.h, _dp(lo), _dp(hi), int(min_count), int(min_miss), float(miss_ratio))
        return self._read_box(self.L.tloam_closed_map_read_carved, "tloam_closed_map_read_carved", head,
                              [(3, np.float64), (None, np.int64), (None, np.int64)])

    # ---- the surfels of the closed map: per voxel a normal and three variances
    def closed_map_surfel_configure(self, cfg: ClosedMapSurfelConfig | None = None, **over):
        """the surfels' configuration (default_closed_map_surfel_config(**over) when cfg is None); drops the surfels, not the
        closed map or the carve's counts.  Kept across odometry_reset."""
        cfg = cfg if cfg is not None else default_closed_map_surfel_config(**over)
        self._check(self.L.tloam_closed_map_surfel_configure(self.h, C.byref(cfg)), "tloam_closed_map_surfel_configure")

    def closed_map_surfels(self) -> dict:
        """gathers, per voxel of the built closed map, the second moments of its points and solves them -> info dict"""
        info = ClosedMapSurfelInfo()
        self._check(self.L.tloam_closed_map_surfels(self.h, C.byref(info)), "tloam_closed_map_surfels")
        return info.as_dict()

    def closed_map_surfel_info(self) -> dict:
        info = ClosedMapSurfelInfo()
        self._check(self.L.tloam_closed_map_get_surfel_info(self.h, C.byref(info)), "tloam_closed_map_get_surfel_info")
        return info.as_dict()

    def closed_map_moments(self, first=0, count=None):
        """the thirteen sums (Ns, R, S xx xy xz yy yz zz, W) of voxels [first, first + count) in id order, (m, 13) int64;
        count None: to the end"""
        first, m = _id_range(first, count, lambda: self.closed_map_info()["n_voxels"])
        out = np.zeros((max(m, 1), 13), np.int64)
        self._check(self.L.tloam_closed_map_read_moments(self.h, int(first), m, _lp(out)), "tloam_closed_map_read_moments")
        return out[:m].copy()

    def closed_map_read_surfels(self, first=0, count=None):
        """voxels [first, first + count) in id order -> (normals (m, 3), variances ascending (m, 3) in m^2, Ns (m,) int64);
        count None: to the end.  An unsolved voxel's normal and variances are zero"""
        first, m = _id_range(first, count, lambda: self.closed_map_info()["n_voxels"])
        nrm, ev, cnt = np.zeros((max(m, 1), 3)), np.zeros((max(m, 1), 3)), np.zeros(max(m, 1), np.int64)
        self._check(self.L.tloam_closed_map_read_surfels(self.h, int(first), m, _dp(nrm), _dp(ev), _lp(cnt)),
                    "tloam_closed_map_read_surfels")
        return nrm[:m].copy(), ev[:m].copy(), cnt[:m].copy()

    def closed_map_read_surfels_box(self, lo=None, hi=None, min_count=1, max_sigma=float("inf"), min_planarity=0.05):
        """closed_map_read_box's voxels (lo and hi None: the whole map) whose surfel is solved with ev2 > 0,
        ev0 <= max_sigma^2 and ev1 - ev0 >= min_planarity * ev2, in id order ->
        (centroids (m, 3), normals (m, 3), variances (m, 3), Ns (m,))"""
        lo, hi = _box(lo, hi)
        head = (self.h, _dp(lo), _dp(hi), int(min_count), float(max_sigma), float(min_planarity))
        return self._read_box(self.L.tloam_closed_map_read_surfels_box, "tloam_closed_map_read_surfels_box", head,
                              [(3, np.float64), (3, np.float64), (3, np.float64), (None, np.int64)])

    # ---- localisation of a scan in the closed map: point-to-plane Gauss-Newton on the surfels
    def closed_map_localise_configure(self, cfg: ClosedMapLocaliseConfig | None = None, **over):
        """the localisation's configuration (default_closed_map_localise_config(**over) when cfg is None).  Kept across
        odometry_reset; a refused configuration leaves the old one."""
        cfg = cfg if cfg is not None else default_closed_map_localise_config(**over)
        self._check(self.L.tloam_closed_map_localise_configure(self.h, C.byref(cfg)), "tloam_closed_map_localise_configure")

    def closed_map_localise(self, points, prior):
        """the scan `points` (n, 3; sensor frame) registered against the closed map's surfels from the pose `prior` (4 x 4)
        -> (pose (4, 4), info dict).  A DEGENERATE status returns the prior"""
        pts = _aos(points)
        pr, out = _colmajor(prior), np.zeros(16)
        info = ClosedMapLocaliseInfo()
        self._check(self.L.tloam_closed_map_localise(self.h, _dp(pts), len(pts), _dp(pr), _dp(out), C.byref(info)),
                    "tloam_closed_map_localise")
        return out.reshape(4, 4).T.copy(), info.as_dict()

    def closed_map_localise_log(self) -> list:
        """the executed iterations of the last closed_map_localise: dicts of pose (before the step), tau, cost, d, matched, used"""
        return self._read_list(self.L.tloam_closed_map_localise_log, "tloam_closed_map_localise_log", ClosedMapLocaliseRecord, self.h)

    def closed_map_linearise(self, points, pose, tau) -> dict:
        """one sweep at `pose` (4 x 4) with truncation `tau`, no step -> dict(ids (n,) int32, -1 unmatched; residuals (n,);
        H (21,) upper triangle by rows; g (6,); cost; matched; used)"""
        pts = _aos(points)
        ids, res = np.zeros(max(len(pts), 1), np.int32), np.zeros(max(len(pts), 1))
        out, cnt = np.zeros(28), np.zeros(2, np.int64)
        self._check(self.L.tloam_closed_map_linearise(self.h, _dp(pts), len(pts), _dp(_colmajor(pose)), float(tau), _ip(ids),
                                                      _dp(res), _dp(out), _lp(cnt)), "tloam_closed_map_linearise")
        return {"ids": ids[: len(pts)].copy(), "residuals": res[: len(pts)].copy(), "H": out[:21].copy(), "g": out[21:27].copy(),
                "cost": float(out[27]), "matched": int(cnt[0]), "used": int(cnt[1])}

    # ---- several hypotheses of one scan, and relocalisation without a prior
    def closed_map_localise_batch(self, points, priors):
        """the scan `points` registered from every pose of `priors` (B, 4, 4; B in 1 .. 32) in one set of launches
        -> (poses (B, 4, 4), [info dict] * B, best).  Hypothesis h has the bits of closed_map_localise(points, priors[h]);
        best is -1 when every hypothesis is DEGENERATE"""
        pts = _aos(points)
        priors = np.asarray(priors, np.float64)
        if priors.ndim != 3 or priors.shape[1:] != (4, 4):
            raise ValueError("priors: (B, 4, 4)")
        B = len(priors)
        pr = np.ascontiguousarray(priors.transpose(0, 2, 1)).reshape(-1)   # column-major, hypothesis by hypothesis
        out = np.zeros(16 * max(B, 1))
        infos = (ClosedMapLocaliseInfo * max(B, 1))()
        best = C.c_int32(-1)
        self._check(self.L.tloam_closed_map_localise_batch(self.h, _dp(pts), len(pts), _dp(pr), B, _dp(out), infos,
                                                           C.byref(best)), "tloam_closed_map_localise_batch")
        poses = out[: 16 * B].reshape(B, 4, 4).transpose(0, 2, 1).copy()
        return poses, [infos[h].as_dict() for h in range(B)], int(best.value)

    def closed_map_localise_batch_log(self, h) -> list:
        """the executed iterations of hypothesis h of the last closed_map_localise_batch (or closed_map_relocalise)"""
        return self._read_list(self.L.tloam_closed_map_localise_batch_log, "tloam_closed_map_localise_batch_log",
                               ClosedMapLocaliseRecord, self.h, int(h))

    def closed_map_relocalise_configure(self, cfg: ClosedMapRelocaliseConfig | None = None, **over):
        """the relocalisation's configuration (default_closed_map_relocalise_config(**over) when cfg is None).  Kept across
        odometry_reset; a refused configuration leaves the old one."""
        cfg = cfg if cfg is not None else default_closed_map_relocalise_config(**over)
        self._check(self.L.tloam_closed_map_relocalise_configure(self.h, C.byref(cfg)), "tloam_closed_map_relocalise_configure")

    def closed_map_relocalise(self, points):
        """the scan `points` (n, 3; sensor frame) localised in the closed map without a prior: place recognition's candidates,
        a hypothesis from each, the batched localiser, the pick -> (pose (4, 4) or None when NOT_FOUND, info dict)"""
        pts = _aos(points)
        out = np.zeros(16)
        info = ClosedMapRelocaliseInfo()
        self._check(self.L.tloam_closed_map_relocalise(self.h, _dp(pts), len(pts), _dp(out), C.byref(info)),
                    "tloam_closed_map_relocalise")
        pose = out.reshape(4, 4).T.copy() if info.status == RELOCALISE_FOUND else None
        return pose, info.as_dict()

    def closed_map_relocalise_hypotheses(self) -> list:
        """the hypotheses of the last closed_map_relocalise, in candidate order: dicts of keyframe, shift, skipped, dist, yaw,
        prior, pose and the localise info"""
        return self._read_list(self.L.tloam_closed_map_relocalise_hypotheses, "tloam_closed_map_relocalise_hypotheses",
                               ClosedMapRelocaliseHypothesis, self.h)

    # ---- a scan diffed against the closed map: new points, voxels seen through
    def closed_map_diff_configure(self, cfg: ClosedMapDiffConfig | None = None, **over):
        """the diff's configuration (default_closed_map_diff_config(**over) when cfg is None); drops the counts, not the closed
        map.  Kept across odometry_reset; a refused configuration leaves the old one."""
        cfg = cfg if cfg is not None else default_closed_map_diff_config(**over)
        self._check(self.L.tloam_closed_map_diff_configure(self.h, C.byref(cfg)), "tloam_closed_map_diff_configure")

    def closed_map_diff(self, points, pose, accumulate=False, want_ids=False):
        """the scan `points` (n, 3; sensor frame) at `pose` (4 x 4) against the closed map -> (labels (n,) uint8: DIFF_INVALID,
        DIFF_SURFACE, DIFF_OCCUPIED, DIFF_NEW; ids (n,) int32 of the voxel that explained each point, -1 for none, or None
        without want_ids; info dict).  accumulate: the per-voxel counts are added to the stored ones instead of replacing them"""
        pts = _aos(points)
        labels, ids, cut = _per_point(len(pts), want_ids)
        info = ClosedMapDiffInfo()
        self._check(self.L.tloam_closed_map_diff(self.h, _dp(pts), len(pts), _dp(_colmajor(pose)),
                                                 DIFF_ACCUMULATE if accumulate else 0, _u8p(labels), _ip(ids), C.byref(info)),
                    "tloam_closed_map_diff")
        return cut(labels), cut(ids), info.as_dict()

    def closed_map_diff_info(self) -> dict:
        info = ClosedMapDiffInfo()
        self._check(self.L.tloam_closed_map_get_diff_info(self.h, C.byref(info)), "tloam_closed_map_get_diff_info")
        return info.as_dict()

    def closed_map_diff_counts(self, first=0, count=None):
        """through and hits of voxels [first, first + count) in id order -> ((m,) int64, (m,) int64); count None: to the end"""
        first, m = _id_range(first, count, lambda: self.closed_map_info()["n_voxels"])
        through, hits = np.zeros(max(m, 1), np.int64), np.zeros(max(m, 1), np.int64)
        self._check(self.L.tloam_closed_map_read_diff(self.h, int(first), m, _lp(through), _lp(hits)), "tloam_closed_map_read_diff")
        return through[:m].copy(), hits[:m].copy()

    def closed_map_read_gone(self, lo=None, hi=None, min_through=3, gone_ratio=1.0):
        """the voxels (lo and hi None: of the whole map; else with their centroid in [lo, hi]) the diffed scans saw through --
        through >= min_through and through > gone_ratio * hits -- in id order ->
        (centroids (m, 3), counts (m,), through (m,), hits (m,))"""
        lo, hi = _box(lo, hi)
        head = (self.h, _dp(lo), _dp(hi), int(min_through), float(gone_ratio))
        return self._read_box(self.L.tloam_closed_map_read_gone, "tloam_closed_map_read_gone", head,
                              [(3, np.float64), (None, np.int64), (None, np.int64), (None, np.int64)])

    # ---- the closed map ray-cast: predicted ranges along segments from a pose
    def closed_map_raycast_configure(self, cfg: ClosedMapRaycastConfig | None = None, **over):
        """the ray-cast's configuration (default_closed_map_raycast_config(**over) when cfg is None); clears the last info, not
        the closed map.  Kept across odometry_reset; a refused configuration leaves the old one."""
        cfg = cfg if cfg is not None else default_closed_map_raycast_config(**over)
        self._check(self.L.tloam_closed_map_raycast_configure(self.h, C.byref(cfg)), "tloam_closed_map_raycast_configure")

    def closed_map_raycast(self, ends, pose, want_ids=False):
        """the segments from `pose`'s translation to `ends` (n, 3; sensor frame) under `pose` (4 x 4) through the closed map ->
        (status (n,) uint8: RAYCAST_SKIPPED, RAYCAST_MISS, RAYCAST_HIT_CENTROID, RAYCAST_HIT_PLANE; ranges (n,) float64, metres
        along the segment to the first hit, -1.0 without one; ids (n,) int32 of the voxel hit, -1 for none, or None without
        want_ids; info dict)"""
        e = _aos(ends)
        status, ids, cut = _per_point(len(e), want_ids)
        ranges = np.zeros(max(len(e), 1), np.float64)
        info = ClosedMapRaycastInfo()
        self._check(self.L.tloam_closed_map_raycast(self.h, _dp(e), len(e), _dp(_colmajor(pose)), _u8p(status), _dp(ranges),
                                                    _ip(ids), C.byref(info)), "tloam_closed_map_raycast")
        return cut(status), cut(ranges), cut(ids), info.as_dict()

    def closed_map_raycast_info(self) -> dict:
        info = ClosedMapRaycastInfo()
        self._check(self.L.tloam_closed_map_get_raycast_info(self.h, C.byref(info)), "tloam_closed_map_get_raycast_info")
        return info.as_dict()

    # ---- free space for the closed map: an occupancy grid from the rays
    def closed_map_free_configure(self, cfg: FreeConfig | None = None, **over):
        """the free space's configuration (default_closed_map_free_config(**over) when cfg is None); drops the grid, not the
        closed map.  Kept across odometry_reset; a refused configuration leaves the old one."""
        cfg = cfg if cfg is not None else default_closed_map_free_config(**over)
        self._check(self.L.tloam_closed_map_free_configure(self.h, C.byref(cfg)), "tloam_closed_map_free_configure")

    def closed_map_free_info(self) -> dict:
        info = FreeInfo()
        self._check(self.L.tloam_closed_map_get_free_info(self.h, C.byref(info)), "tloam_closed_map_get_free_info")
        return info.as_dict()

    def closed_map_free_reset(self, lo_cells=None, hi_cells=None) -> dict:
        """allocates and zeroes the grid over the cells [lo_cells, hi_cells] (inclusive, rounded out to bricks); both None: the
        auto box around the closed map's poses -> info dict"""
        if (lo_cells is None) != (hi_cells is None):
            raise ValueError("lo_cells and hi_cells go together")
        lo = hi = None
        if lo_cells is not None:
            lo = np.ascontiguousarray(lo_cells, dtype=np.int64).reshape(3)
            hi = np.ascontiguousarray(hi_cells, dtype=np.int64).reshape(3)
        self._check(self.L.tloam_closed_map_free_reset(self.h, _lp(lo), _lp(hi)), "tloam_closed_map_free_reset")
        return self.closed_map_free_info()

    def closed_map_free_add_keyframes(self) -> dict:
        """walks the rays of the keyframes the grid has not seen (all of the map's after a reset, the new ones after an extend)
        -> info dict"""
        info = FreeInfo()
        self._check(self.L.tloam_closed_map_free_add_keyframes(self.h, C.byref(info)), "tloam_closed_map_free_add_keyframes")
        return info.as_dict()

    def closed_map_free_add_scan(self, points, pose) -> dict:
        """walks the rays of the scan `points` (n, 3; sensor frame) at `pose` (4 x 4) -> info dict"""
        pts = _aos(points)
        info = FreeInfo()
        self._check(self.L.tloam_closed_map_free_add_scan(self.h, _dp(pts), len(pts), _dp(_colmajor(pose)), C.byref(info)),
                    "tloam_closed_map_free_add_scan")
        return info.as_dict()

    def closed_map_free_build(self, lo_cells=None, hi_cells=None) -> dict:
        """closed_map_free_reset, then closed_map_free_add_keyframes -> info dict"""
        self.closed_map_free_reset(lo_cells, hi_cells)
        return self.closed_map_free_add_keyframes()

    def closed_map_free_words(self, first=0, count=None):
        """the grid's words [first, first + count) -> (m,) uint64; count None: to the end"""
        def total():
            nb = self.closed_map_free_info()["n_bricks"]
            return nb[0] * nb[1] * nb[2]
        first, m = _id_range(first, count, total)
        words = np.zeros(max(m, 1), np.uint64)
        self._check(self.L.tloam_closed_map_read_free_words(self.h, int(first), m, words.ctypes.data_as(C.POINTER(C.c_uint64))),
                    "tloam_closed_map_read_free_words")
        return words[:m].copy()

    def closed_map_occupancy(self, points, pose=None, want_ids=False):
        """the state of `points` (n, 3; in the map frame, or with `pose` (4 x 4) in its sensor frame) -> (states (n,) uint8:
        OCCUPANCY_INVALID, OCCUPANCY_UNKNOWN, OCCUPANCY_FREE, OCCUPANCY_OCCUPIED; ids (n,) int32 of the voxel of an OCCUPIED
        point, -1 otherwise, or None without want_ids; counts (4,) int64 of points per state)"""
        pts = _aos(points)
        state, ids, cut = _per_point(len(pts), want_ids)
        counts = np.zeros(4, np.int64)
        self._check(self.L.tloam_closed_map_occupancy(self.h, _dp(pts), len(pts), None if pose is None else _dp(_colmajor(pose)),
                                                      _u8p(state), _ip(ids), _lp(counts)), "tloam_closed_map_occupancy")
        return cut(state), cut(ids), counts

    def closed_map_free_cells(self, lo=None, hi=None):
        """the centres (m, 3) of the FREE cells (lo and hi None: of the whole grid; else with their centre in [lo, hi]), brick
        index ascending, then bit ascending"""
        lo, hi = _box(lo, hi)
        return self._read_box(self.L.tloam_closed_map_read_free, "tloam_closed_map_read_free", (self.h, _dp(lo), _dp(hi)),
                              [(3, np.float64)])[0]

    def closed_map_free_columns(self, z_lo, z_hi, min_free=1):
        """the navigation grid (ny, nx) uint8 over the box's x-y footprint for the band of cells between heights z_lo and z_hi:
        OCCUPANCY_OCCUPIED, OCCUPANCY_FREE (at least min_free free band cells) or OCCUPANCY_UNKNOWN per column"""
        info = self.closed_map_free_info()
        nx, ny = C.c_size_t(0), C.c_size_t(0)
        out = np.zeros(max(16 * info["n_bricks"][0] * info["n_bricks"][1], 1), np.uint8)
        self._check(self.L.tloam_closed_map_free_columns(self.h, float(z_lo), float(z_hi), int(min_free),
                                                         _u8p(out), len(out), C.byref(nx), C.byref(ny)),
                    "tloam_closed_map_free_columns")
        return out[: nx.value * ny.value].reshape(ny.value, nx.value).copy()

    def fitness(self):
        f, r = C.c_double(0), C.c_double(0)
        rc = self.L.tloam_fitness(self.h, C.byref(f), C.byref(r))
        return rc, f.value, r.value

    def get_correspondences(self, kind, capacity=None):
        cap = int(capacity or max(self._n.get(("s", kind), 0), self._n.get(("c", kind), 0), 1))
        n = C.c_size_t(0)
        idx = np.zeros(cap, np.int32); a = np.zeros((cap, 3)); b = np.zeros((cap, 3))
        d = np.zeros(cap); w = np.zeros(cap); cost = np.zeros(cap)
        rc = self.L.tloam_get_correspondences(self.h, int(kind), cap, C.byref(n), _ip(idx), _dp(a), _dp(b),
                                              _dp(d), _dp(w), _dp(cost))
        self._check(rc, "tloam_get_correspondences")
        m = n.value
        return dict(idx=idx[:m], a=a[:m], b=b[:m], d=d[:m], w=w[:m], cost=cost[:m])

    def get_weights(self, kind):
        cap = max(self._n.get(("s", kind), 0), 1)
        n = C.c_size_t(0)
        w = np.zeros(cap)
        self._check(self.L.tloam_get_weights(self.h, int(kind), cap, C.byref(n), _dp(w)), "tloam_get_weights")
        return w[:n.value]

    def knn(self, kind, queries, radius, k):
        q = _aos(queries)
        idx = np.zeros((len(q), k), np.int32); d2 = np.zeros((len(q), k)); cnt = np.zeros(len(q), np.int32)
        rc = self.L.tloam_knn(self.h, int(kind), _dp(q), len(q), float(radius), int(k), _ip(idx), _dp(d2), _ip(cnt))
        self._check(rc, "tloam_knn")
        return idx, d2, cnt

    def set_correspondences(self, res_type, p, a, b=None, d=None, w=None):
        p = _aos(p); a = _aos(a)
        b = None if b is None else _aos(b)
        d = None if d is None else np.ascontiguousarray(d, float)
        w = np.ones(len(p)) if w is None else np.ascontiguousarray(w, float)
        kind = {RES_PLANE: KIND_PLANAR, RES_LINE: KIND_EDGE, RES_POINT: KIND_SPHERE}[res_type]
        self._n[("c", kind)] = len(p)
        rc = self.L.tloam_set_correspondences(self.h, int(res_type), len(p), _dp(p), _dp(a), _dp(b), _dp(d), _dp(w))
        self._check(rc, "tloam_set_correspondences")
        return rc

    def accumulate(self, se3):
        x = np.ascontiguousarray(se3, float)
        H = np.zeros(36); g = np.zeros(6); cost = C.c_double(0)
        self._check(self.L.tloam_accumulate(self.h, _dp(x), _dp(H), _dp(g), C.byref(cost)), "tloam_accumulate")
        return H.reshape(6, 6), g, cost.value

    def get_normal_equations(self):
        """(H 6x6, g, cost) the minimiser held at the accepted iterate when its last Solve returned."""
        H = np.zeros(36); g = np.zeros(6); cost = C.c_double(0)
        self._check(self.L.tloam_get_normal_equations(self.h, _dp(H), _dp(g), C.byref(cost)), "tloam_get_normal_equations")
        return H.reshape(6, 6), g, cost.value

    def get_costs(self, res_type):
        kind = {RES_PLANE: KIND_PLANAR, RES_LINE: KIND_EDGE, RES_POINT: KIND_SPHERE}[res_type]
        cap = max(self._n.get(("c", kind), 0), 1)
        n = C.c_size_t(0)
        c = np.zeros(cap)
        self._check(self.L.tloam_get_costs(self.h, int(res_type), cap, C.byref(n), _dp(c)), "tloam_get_costs")
        return c[:n.value]

    def solve(self, se3):
        x = np.array(se3, float)
        st = Stats()
        self._check(self.L.tloam_solve(self.h, _dp(x), C.byref(st)), "tloam_solve")
        return x, st.as_dict()

    def time_accumulate(self, se3, launches=100):
        x = np.ascontiguousarray(se3, float)
        us = C.c_double(0)
        self._check(self.L.tloam_time_accumulate(self.h, _dp(x), int(launches), C.byref(us)), "tloam_time_accumulate")
        return us.value

    def time_build(self, launches=20):
        """(mean us per launch, queries per launch) of the correspondence-search kernel on the last frame's state."""
        us = C.c_double(0); n = C.c_int64(0)
        self._check(self.L.tloam_time_build(self.h, int(launches), C.byref(us), C.byref(n)), "tloam_time_build")
        return us.value, n.value

    def time_sharded_sweep(self, se3, launches=50, with_exchange=True):
        """collective: every rank calls it with the same arguments (tloam_time_sharded_sweep)."""
        x = np.ascontiguousarray(se3, float)
        us = C.c_double(0)
        self._check(self.L.tloam_time_sharded_sweep(self.h, _dp(x), int(launches), int(bool(with_exchange)), C.byref(us)),
                    "tloam_time_sharded_sweep")
        return us.value

    def k3_timer(self, reset=False):
        us = C.c_double(0); n = C.c_int64(0); b = C.c_double(0)
        self._check(self.L.tloam_k3_timer(self.h, int(bool(reset)), C.byref(us), C.byref(n), C.byref(b)), "tloam_k3_timer")
        return us.value, n.value, b.value

    def k3_timer_all(self):
        us = C.c_double(0); n = C.c_int64(0)
        self._check(self.L.tloam_k3_timer_all(self.h, C.byref(us), C.byref(n)), "tloam_k3_timer_all")
        return us.value, n.value

    def k3_span(self, reset=False):
        """(total us, launches) of the streaming span of the one-launch GN iterations (tloam_k3_span)."""
        us = C.c_double(0); n = C.c_int64(0)
        self._check(self.L.tloam_k3_span(self.h, int(bool(reset)), C.byref(us), C.byref(n)), "tloam_k3_span")
        return us.value, n.value

    def gn_iter_timer(self, reset=False):
        """(total us, periods) of the GN iterations as the device clocks them (tloam_gn_iter_timer); the first call arms it."""
        us = C.c_double(0); n = C.c_int64(0)
        self._check(self.L.tloam_gn_iter_timer(self.h, int(bool(reset)), C.byref(us), C.byref(n)), "tloam_gn_iter_timer")
        return us.value, n.value

    def time_read_stream(self, nbytes, launches=20):
        """GB/s of a read stream with the sweep's access pattern over ~nbytes (tloam_time_read_stream)."""
        g = C.c_double(0)
        self._check(self.L.tloam_time_read_stream(self.h, int(nbytes), int(launches), C.byref(g)), "tloam_time_read_stream")
        return g.value

    def info(self):
        """tloam_get_info as a dict."""
        ci = CtxInfo()
        self._check(self.L.tloam_get_info(self.h, C.byref(ci)), "tloam_get_info")
        return {f: getattr(ci, f) for f, _ in CtxInfo._fields_ if f != "reserved"}

    def grid_info(self):
        """tloam_get_grid_info as a dict: the search grids of the context's last grid build (per kind dim, n, ncell, cell; the
        build path GRID_SCAN_* and the size of a table entry on it)."""
        gi = GridInfo()
        self._check(self.L.tloam_get_grid_info(self.h, C.byref(gi)), "tloam_get_grid_info")
        return {"dim": [list(d) for d in gi.dim], "n": gi.n[:], "ncell": gi.ncell[:], "cell": gi.cell[:],
                "scan_path": gi.scan_path, "table_elem_bytes": gi.table_elem_bytes}

    # ---- multi-GPU ---------------------------------------------------------------------------
    def comm_init_rccl(self, rank, nranks, unique_id: bytes):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._check(self.L.tloam_comm_init_rccl(self.h, int(rank), int(nranks), C.cast(buf, C.c_void_p)),
                    "tloam_comm_init_rccl")

    def comm_mailbox_export(self) -> bytes:
        """64 bytes (hipIpcMemHandle_t) of this context's exchange buffer; all-gather them in rank order."""
        buf = C.create_string_buffer(64)
        self._check(self.L.tloam_comm_mailbox_export(self.h, C.cast(buf, C.c_void_p)), "tloam_comm_mailbox_export")
        return bytes(buf.raw)

    def comm_init_mailbox(self, rank, nranks, handles):
        """handles: the nranks 64-byte handles in rank order (this rank's own entry is ignored)."""
        blob = b"".join(bytes(h) for h in handles)
        assert len(blob) == 64 * int(nranks)
        buf = C.create_string_buffer(blob, len(blob))
        self._check(self.L.tloam_comm_init_mailbox(self.h, int(rank), int(nranks), C.cast(buf, C.c_void_p)),
                    "tloam_comm_init_mailbox")

    def comm_init_callback(self, rank, nranks, fn):
        """fn(device_ptr:int, count:int, stream:int) -> 0 ; must sum-all-reduce `count` doubles in place."""
        def tramp(user, dev, count, stream):
            try:
                return int(fn(dev, count, stream) or 0)
            except Exception:  # never unwind through C
                import traceback
                traceback.print_exc()
                return 1
        self._cb = ALLREDUCE_FN(tramp)
        self._check(self.L.tloam_comm_init_callback(self.h, int(rank), int(nranks), self._cb, None),
                    "tloam_comm_init_callback")


def rccl_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    rc = load_library().tloam_rccl_unique_id(C.cast(buf, C.c_void_p))
    if rc != 0:
        raise TloamHipError(f"tloam_rccl_unique_id: {STATUS.get(rc, rc)}")
    return buf.raw


def default_feature_config(**over) -> FeatureConfig:
    cfg = FeatureConfig()
    load_library().tloam_feature_default_config(C.byref(cfg))
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def default_seg_config(**over) -> SegConfig:
    return _strict_config(SegConfig, "tloam_seg_default_config", over)


def default_odom_config(**over) -> OdomConfig:
    """tloam_odom_default_config; keyword overrides name a top-level field (edge_down_sample) or one of a stage's
    fields as `<stage>__<field>`, e.g. feature__radius=0.3."""
    cfg = OdomConfig()
    load_library().tloam_odom_default_config(C.byref(cfg))
    for k, v in over.items():
        if "__" in k:
            stage, field = k.split("__", 1)
            sub = getattr(cfg, stage)
            if not hasattr(sub, field):
                raise KeyError(k)
            setattr(sub, field, v)
        elif hasattr(cfg, k):
            setattr(cfg, k, v)
        else:
            raise KeyError(k)
    return cfg


def default_map_config(**over) -> MapConfig:
    """tloam_map_default_config (mapping off, voxel 1.0) with keyword overrides, e.g. enabled=1"""
    return _strict_config(MapConfig, "tloam_map_default_config", over)


def default_voxel_map_config(**over) -> VoxelMapConfig:
    """tloam_voxel_map_default_config (off, voxel 1.0, origin 0) with keyword overrides, e.g. enabled=1, origin=(0, 0, 5)"""
    return _strict_config(VoxelMapConfig, "tloam_voxel_map_default_config", over,
                          {"origin": lambda v: (C.c_double * 3)(*[float(x) for x in v])})


def default_deskew_config(**over) -> DeskewConfig:
    """tloam_deskew_default_config (off, azimuth mode, counter-clockwise, start 0, ref 0) with keyword overrides"""
    return _strict_config(DeskewConfig, "tloam_deskew_default_config", over)


def default_place_config(**over) -> PlaceConfig:
    """tloam_place_default_config (off; 20 x 60 within 80 m, height offset 2; 10 candidates older than 50 keyframes, a loop
    below 0.30; a keyframe every 1 m or 0.2 rad) with keyword overrides"""
    return _strict_config(PlaceConfig, "tloam_place_default_config", over)


def default_loop_config(**over) -> LoopConfig:
    """tloam_loop_default_config (off; a window of 2, the loop record's yaw as the guess; the measured score bounds; the coarse
    stage's TLS values) with keyword overrides; `coarse__<name>` sets a field of the coarse TLS configuration"""
    flat = {k: v for k, v in over.items() if not k.startswith("coarse__")}
    cfg = _strict_config(LoopConfig, "tloam_loop_default_config", flat)
    for k, v in over.items():
        if k.startswith("coarse__"):
            name = k[len("coarse__"):]
            if not hasattr(cfg.coarse, name):
                raise KeyError(k)
            setattr(cfg.coarse, name, v)
    return cfg


def default_graph_config(**over) -> GraphConfig:
    """tloam_graph_default_config (30 Gauss-Newton iterations of at most 20000 conjugate-gradient iterations, step_tol 1e-7,
    cg_tol 1e-10, the odometry and loop sigmas) with keyword overrides"""
    return _strict_config(GraphConfig, "tloam_graph_default_config", over)


def default_graph_robust_config(**over) -> GraphRobustConfig:
    """tloam_graph_robust_default_config (off; noise_chi2 36, mu_factor 1.4, at most 100 outer iterations) with keyword
    overrides, e.g. enabled=1"""
    return _strict_config(GraphRobustConfig, "tloam_graph_robust_default_config", over)


def default_closed_map_config(**over) -> ClosedMapConfig:
    """tloam_closed_map_default_config (voxel 1.0, origin 0, cloud_mask 0xF0) with keyword overrides, e.g. voxel=0.25,
    origin=(0, 0, 5), cloud_mask=0x0F"""
    return _strict_config(ClosedMapConfig, "tloam_closed_map_default_config", over,
                          {"origin": lambda v: (C.c_double * 3)(*[float(x) for x in v])})


def default_closed_map_carve_config(**over) -> ClosedMapCarveConfig:
    """tloam_closed_map_carve_default_config (max_range 60, end_margin 1, radius 0.25, ray_mask 0: the build's) with keyword
    overrides, e.g. max_range=20.0, radius=float("inf")"""
    return _strict_config(ClosedMapCarveConfig, "tloam_closed_map_carve_default_config", over)


def default_closed_map_raycast_config(**over) -> ClosedMapRaycastConfig:
    """tloam_closed_map_raycast_default_config (max_range 120, radius_cells 0.75, planes 1, min_count 1, min_miss 3,
    miss_ratio 1, carve_gate 0) with `over` applied; an unknown field raises"""
    return _strict_config(ClosedMapRaycastConfig, "tloam_closed_map_raycast_default_config", over)


def default_closed_map_free_config(**over) -> FreeConfig:
    """tloam_closed_map_free_default_config (max_range 60, end_margin 1, ray_mask 0: the build's, max_bytes 1 GiB, min_count 1,
    min_miss 3, miss_ratio 1, carve_gate 0) with keyword overrides; an unknown field raises"""
    return _strict_config(FreeConfig, "tloam_closed_map_free_default_config", over)


def default_closed_map_diff_config(**over) -> ClosedMapDiffConfig:
    """tloam_closed_map_diff_default_config (max_range 60, end_margin 1, radius 0.25, plane_tol 0.1, near 0.5, min_miss 3,
    miss_ratio 1, carve_gate 0) with keyword overrides, e.g. max_range=20.0, carve_gate=1"""
    return _strict_config(ClosedMapDiffConfig, "tloam_closed_map_diff_default_config", over)


def default_closed_map_relocalise_config(**over) -> ClosedMapRelocaliseConfig:
    """tloam_closed_map_relocalise_default_config with keyword overrides."""
    return _strict_config(ClosedMapRelocaliseConfig, "tloam_closed_map_relocalise_default_config", over)


def default_closed_map_localise_config(**over) -> ClosedMapLocaliseConfig:
    """tloam_closed_map_localise_default_config with keyword overrides."""
    return _strict_config(ClosedMapLocaliseConfig, "tloam_closed_map_localise_default_config", over)


def default_closed_map_surfel_config(**over) -> ClosedMapSurfelConfig:
    """tloam_closed_map_surfel_default_config (min_points 5) with keyword overrides."""
    return _strict_config(ClosedMapSurfelConfig, "tloam_closed_map_surfel_default_config", over)


def default_submap_config(**over) -> SubmapConfig:
    cfg = SubmapConfig()
    load_library().tloam_submap_default_config(C.byref(cfg))
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def make_registration(method: str, cfg: TlsConfig | None = None, device: int = 0):
    """FrontEnd::initRegistraton (front_end.cpp:155-167) keyed on `local_registration_method`."""
    if method == "TLS_HIP":
        return HipRegistration(cfg, device)
    raise ValueError("Other methods are not yet supported")  # the reference's message, front_end.cpp:163
