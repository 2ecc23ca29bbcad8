"""The C ABI of libtloam_hip.so (include/tloam_hip.h) said once for Python: the constants, one ctypes mirror per struct, the
signature of every entry point (`SIGNATURES`) and the loader that applies them.  tests/test_abi_header.py ties all of it to the
header: every struct's field names, sizes and offsets, and the set of declared functions.  `registration` re-exports every
name here."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH =os.environ.get("TLOAM_HIP_LIB") or os.path.join(_HERE, "libtloam_hip.so")  # env override: tuning builds only

KIND_PLANAR, KIND_GROUND, KIND_EDGE, KIND_SPHERE = 0, 1, 2, 3
RES_PLANE, RES_LINE, RES_POINT = 0, 1, 2

STATUS = {0: "TLOAM_OK", -1: "TLOAM_E_INVALID", -2: "TLOAM_E_TOO_FEW_POINTS", -3: "TLOAM_E_BAD_POSE",
          -4: "TLOAM_E_HIP", -5: "TLOAM_E_RCCL", -6: "TLOAM_E_NOT_READY", -7: "TLOAM_E_WEIGHT_RANGE"}


def _plain(v):
    """an integer field's value: int, an array of them (of any depth) as tuples"""
    return tuple(_plain(x) for x in v) if isinstance(v, C.Array) else int(v)


class Struct(C.Structure):
    """The mirrors' base.  `_c_name_` names the C type; `as_dict` is the one rule from the field types: integers as int (arrays
    of them as tuples), doubles as float (arrays of them as numpy arrays, a 4 x 4 `<name>_colmajor` as the row-major matrix
    under `<name>`), a nested struct as its own dict, the fields named in `_drop_` left out."""
    _c_name_ = None
    _drop_ = ()

    def as_dict(self):
        out = {}
        for name, ctype in self._fields_:
            if name in self._drop_:
                continue
            v = getattr(self, name)
            if issubclass(ctype, C.Structure):
                out[name] = v.as_dict()
            elif ctype is C.c_double:
                out[name] = float(v)
            elif not (issubclass(ctype, C.Array) and ctype._type_ is C.c_double):
                out[name] = _plain(v)
            elif name.endswith("_colmajor"):
                out[name[:-len("_colmajor")]] = np.array(v[:]).reshape(4, 4).T.copy()
            else:
                out[name] = np.array(v[:])
        return out


class SubmapConfig(Struct):
    """tloam_submap_config: the submap keys of config/mapping/lidar_odometry.yaml:6-17."""
    _c_name_ = "tloam_submap_config"
    _fields_ = [("planar_frame_size", C.c_int32), ("sphere_frame_size", C.c_int32),
                ("edge_crop_box_length", C.c_double), ("ground_crop_box_length", C.c_double),
                ("edge_down_sample_submap", C.c_double), ("ground_down_sample_submap", C.c_double),
                ("ground_down_sample", C.c_double)]


class FeatureConfig(Struct):
    """tloam_feature_config: the `feature:` block of config/mapping/feature.yaml."""
    _c_name_ = "tloam_feature_config"
    _fields_ = [("radius", C.c_double), ("K", C.c_int32), ("min_neigh", C.c_int32), ("planar_num", C.c_int32),
                ("sphere_num", C.c_int32), ("cvr_scan", C.c_double), ("cvr_submap", C.c_double),
                ("planar_scan_thres", C.c_double), ("planar_submap_thres", C.c_double),
                ("planar_vertic_thres", C.c_double)]


class SegConfig(Struct):
    """tloam_seg_config: the `velodyne`, `groundSeg` and `DCVC` blocks of config/mapping/segmentation.yaml."""
    _c_name_ = "tloam_seg_config"
    _fields_ = [("sensor_model", C.c_int32), ("reserved0", C.c_int32), ("scan_period", C.c_double),
                ("sensor_height", C.c_double), ("vertical_res", C.c_double), ("init_angle", C.c_double),
                ("sensor_min_range", C.c_double), ("sensor_max_range", C.c_double), ("near_dis", C.c_double),
                ("quadrant", C.c_int32), ("num_sec", C.c_int32), ("dis", C.c_double), ("max_iter", C.c_int32),
                ("ground_seed_num", C.c_int32), ("ring_min_num", C.c_int32), ("reserved1", C.c_int32),
                ("start_r", C.c_double), ("delta_r", C.c_double), ("delta_p", C.c_double), ("delta_a", C.c_double),
                ("min_seg", C.c_int32), ("reserved2", C.c_int32)]


class OdomConfig(Struct):
    """tloam_odom_config: the three stage configurations plus edge_down_sample (lidar_odometry.yaml:8)."""
    _c_name_ = "tloam_odom_config"
    _fields_ = [("seg", SegConfig), ("feature", FeatureConfig), ("submap", SubmapConfig), ("edge_down_sample", C.c_double)]


class MapConfig(Struct):
    """tloam_map_config: mapping_flag (lidar_odometry.yaml:21), the map's voxel (front_end.cpp:272), the HBM reserved."""
    _c_name_ = "tloam_map_config"
    _fields_ = [("enabled", C.c_int32), ("reserved0", C.c_int32), ("voxel", C.c_double), ("reserve_points", C.c_int64)]


class MapInfo(Struct):
    """tloam_map_info."""
    _c_name_ = "tloam_map_info"
    _fields_ = [("n_points", C.c_int64), ("n_frames", C.c_int64), ("last_first", C.c_int64), ("last_count", C.c_int64),
                ("capacity_points", C.c_int64), ("overflow_frames", C.c_int64)]

class VoxelMapConfig(Struct):
    """tloam_voxel_map_config: the merged voxel map's switch, voxel v, origin o, the HBM reserved."""
    _c_name_ = "tloam_voxel_map_config"
    _fields_ = [("enabled", C.c_int32), ("reserved0", C.c_int32), ("voxel", C.c_double), ("origin", C.c_double * 3),
                ("reserve_voxels", C.c_int64)]


class VoxelMapInfo(Struct):
    """tloam_voxel_map_info."""
    _c_name_ = "tloam_voxel_map_info"
    _fields_ = [("n_voxels", C.c_int64), ("n_points", C.c_int64), ("n_frames", C.c_int64), ("last_new", C.c_int64),
                ("capacity_voxels", C.c_int64), ("overflow_frames", C.c_int64)]

class ClosedMapConfig(Struct):
    """tloam_closed_map_config: the closed map's voxel v, origin o, the cloud slots that take part (bit side * 4 + kind), the HBM
    the first build reserves."""
    _c_name_ = "tloam_closed_map_config"
    _fields_ = [("voxel", C.c_double), ("origin", C.c_double * 3), ("cloud_mask", C.c_int32), ("reserved0", C.c_int32),
                ("reserve_voxels", C.c_int64)]


class ClosedMapInfo(Struct):
    """tloam_closed_map_info."""
    _c_name_ = "tloam_closed_map_info"
    _fields_ = [("n_keyframes", C.c_int64), ("added_keyframes", C.c_int64), ("empty_keyframes", C.c_int64),
                ("overflow_keyframes", C.c_int64), ("n_voxels", C.c_int64), ("n_points", C.c_int64),
                ("capacity_voxels", C.c_int64), ("pose_source", C.c_int32), ("launches", C.c_int32)]

class ClosedMapCarveConfig(Struct):
    """tloam_closed_map_carve_config: the longest ray, the margin in front of a return in which nothing is missed, the largest
    distance from a centroid to a ray that misses it, the cloud slots whose points are rays (0: the build's)."""
    _c_name_ = "tloam_closed_map_carve_config"
    _fields_ = [("max_range", C.c_double), ("end_margin", C.c_double), ("radius", C.c_double), ("ray_mask", C.c_int32),
                ("reserved0", C.c_int32)]


class ClosedMapCarveInfo(Struct):
    """tloam_closed_map_carve_info."""
    _c_name_ = "tloam_closed_map_carve_info"
    _fields_ = [("n_keyframes", C.c_int64), ("n_rays", C.c_int64), ("skipped_rays", C.c_int64), ("steps", C.c_int64),
                ("tested", C.c_int64), ("misses", C.c_int64), ("voxels_missed", C.c_int64), ("launches", C.c_int32),
                ("reserved0", C.c_int32)]

class ClosedMapExtendInfo(Struct):
    """tloam_closed_map_extend_info: what one extension of the closed map took and did."""
    _c_name_ = "tloam_closed_map_extend_info"
    _fields_ = [("first_keyframe", C.c_int64), ("n_keyframes", C.c_int64), ("added_keyframes", C.c_int64),
                ("empty_keyframes", C.c_int64), ("overflow_keyframes", C.c_int64), ("points", C.c_int64), ("new_voxels", C.c_int64),
                ("touched_voxels", C.c_int64), ("rays", C.c_int64), ("skipped_rays", C.c_int64), ("steps", C.c_int64),
                ("tested", C.c_int64), ("misses", C.c_int64), ("solved_voxels", C.c_int64), ("grown", C.c_int32),
                ("launches", C.c_int32)]

class ClosedMapSurfelConfig(Struct):
    """tloam_closed_map_surfel_config: the fewest points a voxel is solved from."""
    _c_name_ = "tloam_closed_map_surfel_config"
    _fields_ = [("min_points", C.c_int32), ("reserved0", C.c_int32)]


class ClosedMapSurfelInfo(Struct):
    """tloam_closed_map_surfel_info."""
    _c_name_ = "tloam_closed_map_surfel_info"
    _fields_ = [("n_keyframes", C.c_int64), ("n_points", C.c_int64), ("orphan_points", C.c_int64), ("solved_voxels", C.c_int64),
                ("launches", C.c_int32), ("reserved0", C.c_int32)]

class ClosedMapLocaliseConfig(Struct):
    """tloam_closed_map_localise_config: the truncation's schedule (max_residual0 * shrink^k, floored at min_residual), the
    gate on the surfels (max_sigma, min_planarity), the step tolerances, the Cholesky's pivot ratio, the iteration limit and the
    fewest used points."""
    _c_name_ = "tloam_closed_map_localise_config"
    _fields_ = [("max_residual0", C.c_double), ("shrink", C.c_double), ("min_residual", C.c_double), ("max_sigma", C.c_double),
                ("min_planarity", C.c_double), ("step_tol_t", C.c_double), ("step_tol_r", C.c_double),
                ("min_pivot_ratio", C.c_double), ("max_iterations", C.c_int32), ("min_matches", C.c_int32)]


class ClosedMapLocaliseInfo(Struct):
    """tloam_closed_map_localise_info."""
    _c_name_ = "tloam_closed_map_localise_info"
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("matched", C.c_int64), ("used", C.c_int64), ("rms", C.c_double),
                ("launches", C.c_int32), ("prepared", C.c_int32)]


class ClosedMapLocaliseRecord(Struct):
    """tloam_closed_map_localise_record: one executed iteration."""
    _c_name_ = "tloam_closed_map_localise_record"
    _fields_ = [("pose_colmajor", C.c_double * 16), ("tau", C.c_double), ("cost", C.c_double), ("d", C.c_double * 6),
                ("matched", C.c_int64), ("used", C.c_int64)]


LOCALISE_CONVERGED, LOCALISE_MAX_ITERATIONS, LOCALISE_DEGENERATE = 0, 1, 2
LOCALISE_MAX_BATCH = 32


class ClosedMapRelocaliseConfig(Struct):
    """tloam_closed_map_relocalise_config: how many keyframes are localised from, the Scan Context distance above which a
    candidate is skipped, and the acceptance of the winner.  The defaults are choices, not measurements."""
    _c_name_ = "tloam_closed_map_relocalise_config"
    _fields_ = [("num_candidates", C.c_int32), ("reserved0", C.c_int32), ("max_dist", C.c_double),
                ("min_used_ratio", C.c_double), ("max_rms", C.c_double)]


class ClosedMapRelocaliseInfo(Struct):
    """tloam_closed_map_relocalise_info."""
    _c_name_ = "tloam_closed_map_relocalise_info"
    _fields_ = [("status", C.c_int32), ("n_hypotheses", C.c_int32), ("best", C.c_int32), ("launches", C.c_int32),
                ("keyframe", C.c_int64), ("shift", C.c_int32), ("reserved0", C.c_int32), ("dist", C.c_double), ("yaw", C.c_double),
                ("localise", ClosedMapLocaliseInfo)]
    _drop_ = ("reserved0",)


class ClosedMapRelocaliseHypothesis(Struct):
    """tloam_closed_map_relocalise_hypothesis."""
    _c_name_ = "tloam_closed_map_relocalise_hypothesis"
    _fields_ = [("keyframe", C.c_int64), ("shift", C.c_int32), ("skipped", C.c_int32), ("dist", C.c_double), ("yaw", C.c_double),
                ("prior_colmajor", C.c_double * 16), ("pose_colmajor", C.c_double * 16), ("localise", ClosedMapLocaliseInfo)]


RELOCALISE_FOUND, RELOCALISE_NOT_FOUND = 0, 1


class ClosedMapDiffConfig(Struct):
    """tloam_closed_map_diff_config: the rays' longest range, end margin and radius (the carve's meaning), the residual within
    which a point lies on a surfel, the distance within which a centroid explains it, and the carve gate (min_miss, miss_ratio,
    carve_gate).  The defaults are choices, not measurements."""
    _c_name_ = "tloam_closed_map_diff_config"
    _fields_ = [("max_range", C.c_double), ("end_margin", C.c_double), ("radius", C.c_double), ("plane_tol", C.c_double),
                ("near", C.c_double), ("min_miss", C.c_int64), ("miss_ratio", C.c_double), ("carve_gate", C.c_int32),
                ("reserved0", C.c_int32)]


class ClosedMapDiffInfo(Struct):
    """tloam_closed_map_diff_info."""
    _c_name_ = "tloam_closed_map_diff_info"
    _fields_ = [("n_points", C.c_int64), ("n_invalid", C.c_int64), ("n_surface", C.c_int64), ("n_occupied", C.c_int64),
                ("n_new", C.c_int64), ("rays", C.c_int64), ("skipped_rays", C.c_int64), ("steps", C.c_int64), ("tested", C.c_int64),
                ("through", C.c_int64), ("voxels_through", C.c_int64), ("voxels_hit", C.c_int64), ("scans", C.c_int64),
                ("launches", C.c_int32), ("prepared", C.c_int32), ("cleared", C.c_int32), ("reserved0", C.c_int32)]

DIFF_ACCUMULATE = 1   # TLOAM_DIFF_ACCUMULATE: the call adds to the stored counts
DIFF_INVALID, DIFF_SURFACE, DIFF_OCCUPIED, DIFF_NEW = 0, 1, 2, 3


class ClosedMapRaycastConfig(Struct):
    """tloam_closed_map_raycast_config: the longest segment, the hit radius in voxel sizes, the fewest points of a voxel a ray
    can hit, the carve gate (min_miss, miss_ratio, carve_gate) and which test a voxel is put to (planes: 0 the centroid test
    alone, 1 the plane test where the voxel is eligible, 2 the plane test alone).  The defaults are
    choices, not measurements."""
    _c_name_ = "tloam_closed_map_raycast_config"
    _fields_ = [("max_range", C.c_double), ("radius_cells", C.c_double), ("min_count", C.c_int64), ("min_miss", C.c_int64),
                ("miss_ratio", C.c_double), ("planes", C.c_int32), ("carve_gate", C.c_int32)]


class ClosedMapRaycastInfo(Struct):
    """tloam_closed_map_raycast_info."""
    _c_name_ = "tloam_closed_map_raycast_info"
    _fields_ = [("rays", C.c_int64), ("skipped", C.c_int64), ("missed", C.c_int64), ("hits_centroid", C.c_int64),
                ("hits_plane", C.c_int64), ("steps", C.c_int64), ("tested", C.c_int64), ("launches", C.c_int32),
                ("prepared", C.c_int32)]

RAYCAST_SKIPPED, RAYCAST_MISS, RAYCAST_HIT_CENTROID, RAYCAST_HIT_PLANE = 0, 1, 2, 3   # TLOAM_RAYCAST_*


class FreeConfig(Struct):
    """tloam_closed_map_free_config: the rays' longest range and end margin (the carve's meaning), the most bytes a grid may
    take, which voxels count as occupied when the grid is read (min_count and the carve gate: min_miss, miss_ratio, carve_gate),
    and the keyframe clouds whose points are rays.  The defaults are choices, not measurements."""
    _c_name_ = "tloam_closed_map_free_config"
    _fields_ = [("max_range", C.c_double), ("end_margin", C.c_double), ("max_bytes", C.c_int64), ("min_count", C.c_int64),
                ("min_miss", C.c_int64), ("miss_ratio", C.c_double), ("ray_mask", C.c_int32), ("carve_gate", C.c_int32)]


class FreeInfo(Struct):
    """tloam_closed_map_free_info."""
    _c_name_ = "tloam_closed_map_free_info"
    _fields_ = [("lo_cells", C.c_int64 * 3), ("n_bricks", C.c_int64 * 3), ("bytes", C.c_int64), ("keyframes", C.c_int64),
                ("scans", C.c_int64), ("free_cells", C.c_int64), ("bricks_nonzero", C.c_int64), ("rays", C.c_int64),
                ("skipped_rays", C.c_int64), ("cells_marked", C.c_int64), ("cells_outside", C.c_int64), ("launches", C.c_int32),
                ("reserved0", C.c_int32)]


OCCUPANCY_INVALID, OCCUPANCY_UNKNOWN, OCCUPANCY_FREE, OCCUPANCY_OCCUPIED = 0, 1, 2, 3   # TLOAM_OCCUPANCY_*


class ClearanceConfig(Struct):
    """tloam_closed_map_clearance_config: the truncation distance of the field (R = ceil(max_distance / voxel) cells, 1 .. 128,
    checked at the build), the longest segment a path check walks, the most bytes the field's two buffers may take, and whether
    an UNKNOWN cell (and everything outside the box) is an obstacle.  The defaults are choices, not
    measurements."""
    _c_name_ = "tloam_closed_map_clearance_config"
    _fields_ = [("max_distance", C.c_double), ("max_segment", C.c_double), ("max_bytes", C.c_int64),
                ("unknown_is_obstacle", C.c_int32), ("reserved0", C.c_int32)]


class ClearanceInfo(Struct):
    """tloam_closed_map_clearance_info."""
    _c_name_ = "tloam_closed_map_clearance_info"
    _fields_ = [("lo_cells", C.c_int64 * 3), ("n_cells", C.c_int64 * 3), ("bytes", C.c_int64), ("obstacle_cells", C.c_int64),
                ("finite_cells", C.c_int64), ("sum_d2", C.c_int64), ("max_d2", C.c_int64), ("radius_cells", C.c_int32),
                ("launches", C.c_int32)]


CLEARANCE_BEYOND, CLEARANCE_OUTSIDE = 0xFFFF, 0xFFFE   # TLOAM_CLEARANCE_BEYOND, _OUTSIDE
CLEARANCE_SKIPPED, CLEARANCE_CLEAR, CLEARANCE_BLOCKED, CLEARANCE_LEFT_BOX = 0, 1, 2, 3   # a segment's status


class RouteConfig(Struct):
    """tloam_closed_map_route_config: the most bytes the cost field and its tile flags may take, the most rounds of the tiled
    relaxation a build may run, and how many rounds are enqueued between two waits of the host.  The
    defaults are choices, not measurements."""
    _c_name_ = "tloam_closed_map_route_config"
    _fields_ = [("max_bytes", C.c_int64), ("max_rounds", C.c_int32), ("rounds_per_wait", C.c_int32)]


class RouteInfo(Struct):
    """tloam_closed_map_route_info; tile_updates, rounds, launches and waits are diagnostics that may differ from run to run."""
    _c_name_ = "tloam_closed_map_route_info"
    _fields_ = [("lo_cells", C.c_int64 * 3), ("n_cells", C.c_int64 * 3), ("bytes", C.c_int64), ("need", C.c_int64),
                ("goals_accepted", C.c_int64), ("goals_rejected", C.c_int64), ("traversable_cells", C.c_int64),
                ("reached_cells", C.c_int64), ("sum_cost", C.c_int64), ("max_cost", C.c_int64), ("tile_updates", C.c_int64),
                ("rounds", C.c_int32), ("launches", C.c_int32), ("waits", C.c_int32), ("reserved0", C.c_int32)]


ROUTE_UNREACHED, ROUTE_BLOCKED, ROUTE_OUTSIDE = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD   # TLOAM_ROUTE_UNREACHED, _BLOCKED, _OUTSIDE
ROUTE_PATH_OUTSIDE, ROUTE_PATH_REACHED, ROUTE_PATH_UNREACHED, ROUTE_PATH_BLOCKED, ROUTE_PATH_TRUNCATED = 0, 1, 2, 3, 4
ROUTE_DIAGNOSTICS = ("tile_updates", "rounds", "launches", "waits")   # the info fields that may differ from run to run


class FrontierConfig(Struct):
    """tloam_closed_map_frontier_config: the most bytes the label field, its tile flags and the cluster table may take, the
    fewest cells of a kept cluster, how many cells around a cluster's cells the cost join looks, the most rounds of the tiled
    labelling and how many rounds are enqueued between two waits of the host.  The defaults are choices,
    not measurements."""
    _c_name_ = "tloam_closed_map_frontier_config"
    _fields_ = [("max_bytes", C.c_int64), ("min_cells", C.c_int32), ("reach", C.c_int32), ("max_rounds", C.c_int32),
                ("rounds_per_wait", C.c_int32)]


class FrontierCluster(Struct):
    """tloam_closed_map_frontier_cluster: 64 bytes, no implicit padding"""
    _c_name_ = "tloam_closed_map_frontier_cluster"
    _fields_ = [("sum", C.c_int64 * 3), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("root", C.c_uint32), ("cells", C.c_uint32),
                ("unknown_faces", C.c_uint32), ("reserved", C.c_uint32)]


class FrontierInfo(Struct):
    """tloam_closed_map_frontier_info; tile_updates, rounds, launches and waits are diagnostics that may differ from run to run."""
    _c_name_ = "tloam_closed_map_frontier_info"
    _fields_ = [("lo_cells", C.c_int64 * 3), ("n_cells", C.c_int64 * 3), ("bytes", C.c_int64), ("free_cells", C.c_int64),
                ("unknown_cells", C.c_int64), ("occupied_cells", C.c_int64), ("frontier_cells", C.c_int64), ("clusters", C.c_int64),
                ("clusters_kept", C.c_int64), ("cells_kept", C.c_int64), ("largest", C.c_int64), ("unknown_faces", C.c_int64),
                ("tile_updates", C.c_int64), ("rounds", C.c_int32), ("launches", C.c_int32), ("waits", C.c_int32),
                ("reserved0", C.c_int32)]


# TLOAM_FRONTIER_FREE, _UNKNOWN, _OCCUPIED, _OUTSIDE, _ALL
FRONTIER_FREE, FRONTIER_UNKNOWN, FRONTIER_OCCUPIED, FRONTIER_OUTSIDE, FRONTIER_ALL = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC, 0xFFFFFFFF
FRONTIER_DIAGNOSTICS = ("tile_updates", "rounds", "launches", "waits")   # the info fields that may differ from run to run
# a cluster record as numpy reads an array of them
FRONTIER_CLUSTER_DTYPE = [("sum", "<i8", 3), ("lo", "<i4", 3), ("hi", "<i4", 3), ("root", "<u4"), ("cells", "<u4"),
                          ("unknown_faces", "<u4"), ("reserved", "<u4")]


class ViewConfig(Struct):
    """tloam_closed_map_view_config: the longest ray of a view (it sizes the bit window too), the most bytes the global form's
    windows of one chunk may take, the largest window the LDS form takes and which form runs -- 0 auto, 1 LDS, 2 global
    (DESIGN.md section 33).  The defaults are choices, not measurements."""
    _c_name_ = "tloam_closed_map_view_config"
    _fields_ = [("max_range", C.c_double), ("max_bytes", C.c_int64), ("lds_bytes", C.c_int32), ("form", C.c_int32)]


class ViewRecord(Struct):
    """tloam_closed_map_view_record: a view's gain and counts, 64 bytes, no implicit padding"""
    _c_name_ = "tloam_closed_map_view_record"
    _fields_ = [("unknown_cells", C.c_int64), ("unknown_visits", C.c_int64), ("free_visits", C.c_int64), ("steps", C.c_int64),
                ("rays_skipped", C.c_int32), ("rays_occupied", C.c_int32), ("rays_left_box", C.c_int32), ("rays_ended", C.c_int32),
                ("origin_label", C.c_uint32), ("reserved0", C.c_uint32), ("reserved1", C.c_int64)]


class ViewInfo(Struct):
    """tloam_closed_map_view_info, of the last call; form, blocks_per_view, launches and waits are diagnostics."""
    _c_name_ = "tloam_closed_map_view_info"
    _fields_ = [("views", C.c_int64), ("rays", C.c_int64), ("window_side", C.c_int64), ("window_bytes", C.c_int64),
                ("chunks", C.c_int64), ("steps", C.c_int64), ("unknown_visits", C.c_int64), ("unknown_cells", C.c_int64),
                ("beyond_window", C.c_int64), ("form", C.c_int32), ("blocks_per_view", C.c_int32), ("launches", C.c_int32),
                ("waits", C.c_int32)]


VIEW_FORM_AUTO, VIEW_FORM_LDS, VIEW_FORM_GLOBAL = 0, 1, 2
VIEW_DIAGNOSTICS = ("chunks", "form", "blocks_per_view", "launches", "waits")   # the info fields that depend on the form that ran
# a view's record as numpy reads an array of them
VIEW_GAIN_DTYPE = [("unknown_cells", "<i8"), ("unknown_visits", "<i8"), ("free_visits", "<i8"), ("steps", "<i8"),
                   ("rays_skipped", "<i4"), ("rays_occupied", "<i4"), ("rays_left_box", "<i4"), ("rays_ended", "<i4"),
                   ("origin_label", "<u4"), ("reserved0", "<u4"), ("reserved1", "<i8")]


SNAPSHOT_CLOUDS = 1   # TLOAM_SNAPSHOT_CLOUDS: the keyframes' eight clouds go into the snapshot too


class ClosedMapSnapshotInfo(Struct):
    """tloam_closed_map_snapshot_info: what a closed map snapshot says it holds."""
    _c_name_ = "tloam_closed_map_snapshot_info"
    _fields_ = [("format_version", C.c_int32), ("flags", C.c_int32), ("n_keyframes_database", C.c_int64),
                ("n_keyframes_map", C.c_int64), ("n_voxels", C.c_int64), ("n_points", C.c_int64), ("has_carve", C.c_int32),
                ("has_surfels", C.c_int32), ("has_clouds", C.c_int32), ("n_rings", C.c_int32), ("n_sectors", C.c_int32),
                ("reserved0", C.c_int32), ("cloud_points", C.c_int64), ("voxel", C.c_double), ("origin", C.c_double * 3),
                ("bytes", C.c_uint64)]

    def as_dict(self):
        out = {name: getattr(self, name) for name, _ in self._fields_ if name not in ("origin", "reserved0")}
        out["origin"] = tuple(self.origin)
        return out


class DeskewConfig(Struct):
    """tloam_deskew_config: the deskew's switch, its time source (0 azimuth, 1 per-point times), the sweep's direction (+1
    counter-clockwise seen from +z), the azimuth it starts at and the sweep fraction the pose describes."""
    _c_name_ = "tloam_deskew_config"
    _fields_ = [("enabled", C.c_int32), ("time_source", C.c_int32), ("direction", C.c_int32), ("reserved0", C.c_int32),
                ("start_azimuth", C.c_double), ("ref_fraction", C.c_double)]


class DeskewInfo(Struct):
    """tloam_deskew_info."""
    _c_name_ = "tloam_deskew_info"
    _fields_ = [("frames_deskewed", C.c_int64), ("last_frame", C.c_int64), ("last_twist", C.c_double * 6),
                ("last_max_shift", C.c_double), ("next_motion_colmajor", C.c_double * 16)]


class PlaceConfig(Struct):
    """tloam_place_config: place recognition's switch, the Scan Context grid (rings x sectors within max_radius, z +
    height_offset), the search (num_candidates ring-key neighbours older than exclude_recent keyframes, a loop below
    dist_thres), the keyframe policy (kf_dist, kf_angle) and the HBM reserved."""
    _c_name_ = "tloam_place_config"
    _fields_ = [("enabled", C.c_int32), ("n_rings", C.c_int32), ("n_sectors", C.c_int32), ("num_candidates", C.c_int32),
                ("exclude_recent", C.c_int32), ("reserved0", C.c_int32), ("max_radius", C.c_double),
                ("height_offset", C.c_double), ("kf_dist", C.c_double), ("kf_angle", C.c_double), ("dist_thres", C.c_double),
                ("reserve_keyframes", C.c_int64)]


class PlaceInfo(Struct):
    """tloam_place_info."""
    _c_name_ = "tloam_place_info"
    _fields_ = [("n_keyframes", C.c_int64), ("n_loops", C.c_int64), ("last_keyframe_frame", C.c_int64),
                ("capacity_keyframes", C.c_int64)]

class PlaceLoop(Struct):
    """tloam_place_loop: one loop record."""
    _c_name_ = "tloam_place_loop"
    _fields_ = [("query_keyframe", C.c_int64), ("query_frame", C.c_int64), ("match_keyframe", C.c_int64),
                ("match_frame", C.c_int64), ("shift", C.c_int32), ("reserved0", C.c_int32), ("dist", C.c_double),
                ("yaw", C.c_double)]

    def as_dict(self):
        return {"query": int(self.query_keyframe), "query_frame": int(self.query_frame), "match": int(self.match_keyframe),
                "match_frame": int(self.match_frame), "shift": int(self.shift), "d": float(self.dist), "yaw": float(self.yaw)}


class LoopInfo(Struct):
    """tloam_loop_info."""
    _c_name_ = "tloam_loop_info"
    _fields_ = [("n_constraints", C.c_int64), ("n_accepted", C.c_int64), ("arena_points", C.c_int64),
                ("arena_capacity_points", C.c_int64)]

class GraphConfig(Struct):
    """tloam_graph_config: the pose-graph optimisation's iteration limits and tolerances, and the sigmas the context's graph
    weights its chain (odometry) and loop edges with."""
    _c_name_ = "tloam_graph_config"
    _fields_ = [("max_iterations", C.c_int32), ("max_cg_iterations", C.c_int32), ("step_tol", C.c_double),
                ("cg_tol", C.c_double), ("odom_sigma_t", C.c_double), ("odom_sigma_r", C.c_double),
                ("loop_sigma_t", C.c_double), ("loop_sigma_r", C.c_double)]


class GraphEdge(Struct):
    """tloam_graph_edge: (i, j, Z = rigid_inverse(P_i) P_j column-major, six inverse variances)."""
    _c_name_ = "tloam_graph_edge"
    _fields_ = [("i", C.c_int64), ("j", C.c_int64), ("rel_pose_colmajor", C.c_double * 16), ("weight", C.c_double * 6)]


GRAPH_STOP = {0: "not_run", 1: "step", 2: "iterations", 3: "cost", 4: "cg_limit"}


class GraphInfo(Struct):
    """tloam_graph_info."""
    _c_name_ = "tloam_graph_info"
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


class GraphRobustConfig(Struct):
    """tloam_graph_robust_config: the robust mode of the pose graph, GNC-TLS on the loop edges."""
    _c_name_ = "tloam_graph_robust_config"
    _fields_ = [("enabled", C.c_int32), ("max_outer", C.c_int32), ("noise_chi2", C.c_double), ("mu_factor", C.c_double)]


GRAPH_ROBUST_STOP = {0: "off", 1: "all_inliers", 2: "binary", 3: "outer_limit"}


class GraphRobustInfo(Struct):
    """tloam_graph_robust_info."""
    _c_name_ = "tloam_graph_robust_info"
    _fields_ = [("outer_iterations", C.c_int32), ("stop_reason", C.c_int32), ("gn_iterations", C.c_int64),
                ("cg_iterations", C.c_int64), ("rejected", C.c_int64), ("kept", C.c_int64), ("undecided", C.c_int64),
                ("mu_first", C.c_double), ("mu_last", C.c_double), ("max_chi2_first", C.c_double)]

    def as_dict(self):
        return {"outer_iterations": int(self.outer_iterations), "stop_reason": int(self.stop_reason),
                "stop": GRAPH_ROBUST_STOP[int(self.stop_reason)], "gn_iterations": int(self.gn_iterations),
                "cg_iterations": int(self.cg_iterations), "rejected": int(self.rejected), "kept": int(self.kept),
                "undecided": int(self.undecided), "mu_first": float(self.mu_first), "mu_last": float(self.mu_last),
                "max_chi2_first": float(self.max_chi2_first)}


class TlsConfig(Struct):
    """tloam_tls_config: the 16 keys of the `TLS:` block (config/mapping/lidar_odometry.yaml:23-39)."""
    _c_name_ = "tloam_tls_config"
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


class LoopConfig(Struct):
    """tloam_loop_config: loop verification's switch, the target window around the match keyframe, the initial guess (0: the
    loop record's yaw, 1: the stored poses), the score's inlier distance and the acceptance bounds, the arena reserved, and the
    coarse stage's TLS configuration."""
    _c_name_ = "tloam_loop_config"
    _fields_ = [("enabled", C.c_int32), ("window", C.c_int32), ("init_mode", C.c_int32), ("reserved0", C.c_int32),
                ("inlier_dist", C.c_double), ("min_overlap", C.c_double), ("max_rmse", C.c_double),
                ("reserve_points", C.c_int64), ("coarse", TlsConfig)]


class CtxInfo(Struct):
    """tloam_ctx_info."""
    _c_name_ = "tloam_ctx_info"
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("device_cus", C.c_int32), ("comm_mode", C.c_int32),
                ("rank", C.c_int32), ("nranks", C.c_int32), ("rccl_comm_count", C.c_int32), ("rccl_comm_rank", C.c_int32),
                ("fallbacks_taken", C.c_int32), ("fallback_events", C.c_int32), ("k3_grid", C.c_int32), ("k3_single", C.c_int32),
                ("one_launch_solve", C.c_int32), ("loopback", C.c_int32), ("direct_set", C.c_int32), ("set_stale", C.c_int32),
                ("k3_wide", C.c_int32)]


class GridInfo(Struct):
    """tloam_grid_info."""
    _c_name_ = "tloam_grid_info"
    _fields_ = [("dim", (C.c_int32 * 3) * 4), ("n", C.c_int32 * 4), ("ncell", C.c_int64 * 4), ("cell", C.c_double * 4),
                ("scan_path", C.c_int32), ("table_elem_bytes", C.c_int32)]


GRID_SCAN_NONE, GRID_SCAN_SMALL, GRID_SCAN_TILES, GRID_SCAN_SINGLE_PASS, GRID_SCAN_GENERIC = range(5)


class Stats(Struct):
    """tloam_stats."""
    _c_name_ = "tloam_stats"
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


class LoopConstraint(Struct):
    """tloam_loop_constraint: one verified pair."""
    _c_name_ = "tloam_loop_constraint"
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


class OdomStats(Struct):
    """tloam_odom_stats."""
    _c_name_ = "tloam_odom_stats"
    _fields_ = [("match", Stats), ("frame", C.c_int64), ("n_ground", C.c_int64), ("n_edge", C.c_int64),
                ("n_general", C.c_int64), ("n_edge_ds", C.c_int64), ("n_ground_ds", C.c_int64),
                ("n_planar_scan", C.c_int64), ("n_sphere_scan", C.c_int64), ("n_planar_submap", C.c_int64),
                ("n_sphere_submap", C.c_int64), ("h2d_bytes", C.c_int64), ("d2h_bytes", C.c_int64), ("host_syncs", C.c_int64)]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_[1:]}
        d["match"] = self.match.as_dict()
        return d


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)


class TloamHipError(RuntimeError):
    pass


def _signatures():
    """{entry point: (restype, argtypes)}: one line per function include/tloam_hip.h declares"""
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    sz = C.c_size_t
    return {
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
        "tloam_closed_map_clearance_default_config": (None, [C.POINTER(ClearanceConfig)]),
        "tloam_closed_map_clearance_configure": (C.c_int, [vp, C.POINTER(ClearanceConfig)]),
        "tloam_closed_map_clearance_build": (C.c_int, [vp, C.POINTER(ClearanceInfo)]),
        "tloam_closed_map_get_clearance_info": (C.c_int, [vp, C.POINTER(ClearanceInfo)]),
        "tloam_closed_map_read_clearance": (C.c_int, [vp, sz, sz, C.POINTER(C.c_uint16)]),
        "tloam_closed_map_clearance_points": (C.c_int, [vp, dp, sz, dp, C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), dp,
                                                        C.POINTER(C.c_int64)]),
        "tloam_closed_map_clearance_segments": (C.c_int, [vp, dp, dp, sz, dp, C.c_double, C.POINTER(C.c_uint8),
                                                          C.POINTER(C.c_uint16), dp, C.POINTER(C.c_int64)]),
        "tloam_closed_map_clearance_columns": (C.c_int, [vp, C.c_double, C.c_double, C.c_int64, C.POINTER(C.c_uint8),
                                                         C.POINTER(C.c_uint16), sz, C.POINTER(sz), C.POINTER(sz)]),
        "tloam_closed_map_route_default_config": (None, [C.POINTER(RouteConfig)]),
        "tloam_closed_map_route_configure": (C.c_int, [vp, C.POINTER(RouteConfig)]),
        "tloam_closed_map_route_build": (C.c_int, [vp, dp, sz, dp, C.c_double, C.POINTER(RouteInfo)]),
        "tloam_closed_map_get_route_info": (C.c_int, [vp, C.POINTER(RouteInfo)]),
        "tloam_closed_map_read_route": (C.c_int, [vp, sz, sz, C.POINTER(C.c_uint32)]),
        "tloam_closed_map_route_points": (C.c_int, [vp, dp, sz, dp, C.POINTER(C.c_uint32), dp, C.POINTER(C.c_int64)]),
        "tloam_closed_map_route_paths": (C.c_int, [vp, dp, sz, dp, sz, C.POINTER(C.c_uint8), C.POINTER(C.c_int32),
                                                   C.POINTER(C.c_uint32), dp]),
        "tloam_closed_map_route_columns": (C.c_int, [vp, C.c_double, C.c_double, C.c_int64, dp, sz, dp, C.c_double,
                                                     C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), C.POINTER(C.c_uint32), sz,
                                                     C.POINTER(sz), C.POINTER(sz), C.POINTER(RouteInfo)]),
        "tloam_closed_map_frontier_default_config": (None, [C.POINTER(FrontierConfig)]),
        "tloam_closed_map_frontier_configure": (C.c_int, [vp, C.POINTER(FrontierConfig)]),
        "tloam_closed_map_frontier_build": (C.c_int, [vp, C.POINTER(FrontierInfo)]),
        "tloam_closed_map_get_frontier_info": (C.c_int, [vp, C.POINTER(FrontierInfo)]),
        "tloam_closed_map_read_frontier": (C.c_int, [vp, sz, sz, C.POINTER(C.c_uint32)]),
        "tloam_closed_map_frontier_clusters": (C.c_int, [vp, sz, C.c_void_p, C.POINTER(sz)]),
        "tloam_closed_map_read_frontier_cells": (C.c_int, [vp, C.c_uint32, sz, dp, C.POINTER(C.c_uint32), C.POINTER(sz)]),
        "tloam_closed_map_frontier_points": (C.c_int, [vp, dp, sz, dp, C.POINTER(C.c_uint32), C.POINTER(C.c_int32),
                                                       C.POINTER(C.c_int64)]),
        "tloam_closed_map_frontier_costs": (C.c_int, [vp, sz, C.POINTER(C.c_uint32), dp, C.POINTER(sz)]),
        "tloam_closed_map_frontier_columns": (C.c_int, [vp, C.c_double, C.c_double, C.c_int64, C.POINTER(C.c_uint32), sz, C.c_void_p,
                                                        C.POINTER(sz), C.POINTER(FrontierInfo)]),
        "tloam_closed_map_view_default_config": (None, [C.POINTER(ViewConfig)]),
        "tloam_closed_map_view_configure": (C.c_int, [vp, C.POINTER(ViewConfig)]),
        "tloam_closed_map_view_gain": (C.c_int, [vp, dp, sz, dp, sz, C.c_void_p, C.POINTER(ViewInfo)]),
        "tloam_closed_map_view_cells": (C.c_int, [vp, dp, dp, sz, sz, dp, C.POINTER(sz), C.c_void_p]),
        "tloam_closed_map_frontier_gains": (C.c_int, [vp, dp, sz, sz, C.c_void_p, C.POINTER(C.c_uint32), dp, C.POINTER(sz)]),
        "tloam_closed_map_get_view_info": (C.c_int, [vp, C.POINTER(ViewInfo)]),
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


SIGNATURES = _signatures()
EXPORTED_SYMBOLS = tuple(SIGNATURES)

_lib = None


def load_library():
    """dlopen libtloam_hip.so (built by tloam_amd/build.py) and give every entry point its signature.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TloamHipError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in HBM (effective if HIP is not up yet)
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError if the ABI lost a symbol
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L
