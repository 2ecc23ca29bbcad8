"""Sequence replay: KITTI Velodyne `.bin` scans in, a KITTI-format trajectory out -- the path either side of
scanMatching that BASELINE.json configs[0]/[1] name literally, ready for real KITTI-00 when the
data is present:

    read_velodyne_bin                 readVelodyneToO3d                      read_file.hpp:307-327
      -> label_scan                   (stand-in, see below; the default)
         or tloam_segment             Segmentation::spinOnce                 segmentation.cpp:40-93        [device]
      -> tloam_extract_planar_sphere  featureExtract::extractPlanarSphere    feature_extract.cpp:133-197   [device]
      -> tloam_set_source_frame / tloam_scan_match                           front_end.cpp:314-322          [device]
      -> tloam_submap_update          FrontEnd::updateSubmap                 front_end.cpp:201-275          [device]
      -> format_pose_line             FrontEnd::savePose                     front_end.cpp:169-179

`label_scan` is NOT the reference's segmentation (DCVC clustering + ground fitting, src/models/segmentation -- out of
scope): it is a small geometric labeller -- ground by height over the lowest returns, edge = tall,
isolated columns of a 2-D occupancy grid, the rest handed to the PCA feature extraction -- that only exists so that
the stages around it can be driven end to end.  Trajectories produced with it are therefore not comparable with the
reference's doc/tloam_XX.txt beyond plausibility.

`segmenter="device"` swaps in the reference's segmentation node on the device (`tloam_segment`):
ground = its /ground_points, edge = /edge_points, the PCA features come from /general_points.  Everything downstream
stays as it is, `_voxel_first` included (the stand-in for FrontEnd::processCloud's VoxelDownSample of the edge and
ground clouds, front_end.cpp:183,186).  A frame the node publishes nothing for (TLOAM_E_TOO_FEW_POINTS) raises.

`pipeline="device"` replaces all of the above with one `tloam_odometry_frame` per scan: the
reference's front end -- the segmentation node, processCloud's VoxelDownSample (averages, not `_voxel_first`), no
`at_least()` padding -- with every cloud in HBM; a frame the device skips (TLOAM_E_TOO_FEW_POINTS) is left out and listed.
With a map configuration it also keeps the global map on the device and can write it as PCD.

Host-side glue only (numpy + the C ABI through tloam_amd.registration); no oracle, no CPU fallback of any device stage."""
from __future__ import annotations

import glob
import os
import time

import numpy as np

from . import kitti_io, map_io
from .synth import Frame


def _voxel_first(xyz: np.ndarray, size: float) -> np.ndarray:
    """one point (the first in input order) per occupied voxel -- a cheap stand-in for the per-scan VoxelDownSample of
    the segmentation stage (edge 0.1 m, ground 0.3 m: lidar_odometry.yaml:6,8)"""
    if len(xyz) == 0:
        return xyz
    key = np.floor(xyz / size).astype(np.int64)
    key = (key[:, 0] * 73856093) ^ (key[:, 1] * 19349663) ^ (key[:, 2] * 83492791)
    _, first = np.unique(key, return_index=True)
    first.sort()
    return np.ascontiguousarray(xyz[first])


def label_scan(xyz: np.ndarray, sensor_height: float = 1.73, max_range: float = 60.0):
    """-> (ground, edge, other): see the module docstring.  sensor_height: segmentation.yaml:4."""
    r2 = xyz[:, 0] ** 2 + xyz[:, 1] ** 2
    xyz = xyz[(r2 > 1.0) & (r2 < max_range ** 2)]
    z0 = -sensor_height
    ground_m = xyz[:, 2] < z0 + 0.25
    rest = xyz[~ground_m]
    # 2-D occupancy columns of 0.4 m: vertical extent and number of occupied neighbours
    cell = 0.4
    ij = np.floor(rest[:, :2] / cell).astype(np.int64)
    off = ij.min(axis=0) if len(ij) else np.zeros(2, np.int64)
    ij -= off
    w = int(ij[:, 0].max()) + 3 if len(ij) else 3
    h = int(ij[:, 1].max()) + 3 if len(ij) else 3
    lin = (ij[:, 0] + 1) * h + (ij[:, 1] + 1)
    zmin = np.full(w * h, np.inf); zmax = np.full(w * h, -np.inf)
    np.minimum.at(zmin, lin, rest[:, 2]); np.maximum.at(zmax, lin, rest[:, 2])
    occ = np.isfinite(zmin).reshape(w, h)
    tall = ((zmax - zmin) > 1.2).reshape(w, h)
    nb = np.zeros((w, h), np.int32)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            if dx or dy:
                nb += np.roll(np.roll(occ, dx, 0), dy, 1)
    edge_col = tall & (nb <= 2)            # poles, trunks, corners: tall and isolated
    is_edge = edge_col.reshape(-1)[lin]
    return (_voxel_first(xyz[ground_m], 0.3), _voxel_first(rest[is_edge], 0.1), np.ascontiguousarray(rest[~is_edge]))


def segment_scan(H, xyz: np.ndarray, seg_cfg=None):
    """-> (ground, edge, general) from the device segmentation node, ground / edge voxel-thinned like label_scan's"""
    S = H.segment(xyz, seg_cfg)
    if S["status"] != 0:
        raise RuntimeError("tloam_segment: the node publishes nothing for this scan (TLOAM_E_TOO_FEW_POINTS)")
    return (_voxel_first(np.ascontiguousarray(xyz[S["ground"]]), 0.3), _voxel_first(np.ascontiguousarray(xyz[S["edge"]]), 0.1),
            np.ascontiguousarray(xyz[S["general"]]))


def features_of_scan(H, xyz: np.ndarray, feature_cfg=None, sensor_height: float = 1.73, segmenter: str = "label_scan",
                     seg_cfg=None):
    """One raw scan -> the clouds FrontEnd hands on (front_end.cpp:183-198): scan-side Frame (planar_scan, ground,
    edge, sphere_scan) and the submap-side selections (planar_submap, sphere_submap).  PCA lists on the device.
    segmenter: "label_scan" (the stand-in, default) or "device" (tloam_segment)."""
    if segmenter == "label_scan":
        ground, edge, other = label_scan(xyz, sensor_height)
    elif segmenter == "device":
        ground, edge, other = segment_scan(H, xyz, seg_cfg)
    else:
        raise ValueError(f"unknown segmenter {segmenter!r}")
    ps, pm, ss, sm = H.extract_planar_sphere(other, feature_cfg)
    sel = lambda idx: np.ascontiguousarray(other[np.asarray(idx, np.int64) % max(len(other), 1)]) if len(other) else other  # noqa: E731
    planar_scan, planar_submap, sphere_scan, sphere_submap = sel(ps), sel(pm), sel(ss), sel(sm)

    def at_least(a, pool, n=10):   # the path needs >= 10 points per cloud (registration.cpp:928-929)
        return a if len(a) >= n or len(pool) < n else np.ascontiguousarray(pool[:: max(len(pool) // 64, 1)][:max(n, 64)])
    planar_scan, planar_submap = at_least(planar_scan, other), at_least(planar_submap, other)
    sphere_scan, sphere_submap = at_least(sphere_scan, other), at_least(sphere_submap, other)
    return Frame(planar_scan, ground, edge, sphere_scan), planar_submap, sphere_submap


def list_scans(path: str):
    """<path>/velodyne/*.bin (KITTI odometry layout), or <path>/*.bin"""
    for d in (os.path.join(path, "velodyne"), path):
        files = sorted(glob.glob(os.path.join(d, "*.bin")))
        if files:
            return files
    return []


def _read_scan(path):
    return np.asarray(path, np.float64).reshape(-1, 3) if isinstance(path, np.ndarray) else kitti_io.read_velodyne_bin(path)[0]


def replay_device(H, scan_files, out_poses: str | None = None, odom_cfg=None, init_pose=None, max_frames=None,
                  map_cfg=None, out_map: str | None = None, deskew_cfg=None, place_cfg=None, loop_cfg=None):
    """pipeline="device": one tloam_odometry_frame per scan.  Frames the device skips
    (TLOAM_E_TOO_FEW_POINTS) are left out of the poses and listed in the stats as `skipped` (their positions in
    `scan_files`); `frame_of_pose` gives each pose's position.
    map_cfg (a MapConfig): the global map is configured with it before the run; the stats get its
    `map` info, and out_map names a PCD file the map is written to (tloam_amd/map_io.py).
    deskew_cfg (a DeskewConfig, azimuth mode: `.bin` scans carry no per-point times): the frames deskew their scans under the
    constant-velocity motion; the stats get its `deskew` info.
    place_cfg (a PlaceConfig): place recognition picks keyframes and searches them for loops; the
    stats get its `place` info and the `loops` found (read once, after the last frame).
    loop_cfg (a LoopConfig): the keyframes keep their clouds and the pending loops are verified once, after the last frame
    (DESIGN.md section 17); the stats get its `loop` info and the `constraints`."""
    files = scan_files[: max_frames] if max_frames else scan_files
    if deskew_cfg is not None:
        if deskew_cfg.enabled and deskew_cfg.time_source != 0:
            raise ValueError("replay_device deskews in azimuth mode only (time_source 0): scan files carry no times")
        H.deskew_configure(deskew_cfg)
    if map_cfg is not None:
        H.map_configure(map_cfg)
    if place_cfg is not None:
        H.place_configure(place_cfg)
    if loop_cfg is not None:
        H.loop_configure(loop_cfg)
    H.odometry_reset(init_pose, odom_cfg)
    poses, at, skipped, t_frame, iters = [], [], [], [], 0
    out = open(out_poses, "w") if out_poses else None
    try:
        for f, path in enumerate(files):
            xyz = _read_scan(path)
            t0 = time.perf_counter()
            rc, T, st = H.odometry_frame(xyz)
            t1 = time.perf_counter()
            if rc == -2:
                skipped.append(f)
                continue
            if rc not in (0, -7):
                raise RuntimeError(f"frame {f}: odometry_frame status {rc}")
            iters += st["match"]["gn_sweeps"]
            poses.append(T)
            at.append(f)
            if out:
                out.write(kitti_io.format_pose_line(T))
            if st["frame"] > 0:
                t_frame.append((t1 - t0) * 1e3)
    finally:
        if out:
            out.close()
    m = lambda v: round(float(np.mean(v)), 4) if v else None  # noqa: E731
    stats = {"frames": len(poses), "skipped": skipped, "frame_of_pose": at, "ms_odometry_frame": m(t_frame),
             "gn_iters_per_frame": round(iters / max(len(poses) - 1, 1), 2)}
    if deskew_cfg is not None:
        info = H.deskew_info()
        stats["deskew"] = {"frames_deskewed": info["frames_deskewed"], "last_max_shift": info["last_max_shift"]}
    if place_cfg is not None:
        stats["place"] = H.place_info()
        stats["loops"] = H.place_loops() if place_cfg.enabled else []
    if loop_cfg is not None:
        if loop_cfg.enabled:
            H.loop_verify_pending()
        stats["loop"] = H.loop_info()
        stats["constraints"] = H.loop_constraints()
    if map_cfg is not None:
        stats["map"] = H.map_info()
        if out_map:
            map_io.write_pcd(out_map, H.map_read())
    return poses, stats


def replay(H, scan_files, out_poses: str | None = None, feature_cfg=None, sensor_height: float = 1.73, max_frames=None,
           sync=None, segmenter: str = "label_scan", seg_cfg=None, pipeline: str = "host", odom_cfg=None, init_pose=None):
    """FrontEnd::updateLidarOdometry (front_end.cpp:278-337) over a list of `.bin` scans on the device.  Returns the
    poses (map <- sensor, 4x4) and per-stage host-to-host timings in ms.  A scan may also be given as an (N, 3) array.
    segmenter: see features_of_scan.  pipeline: "host" (the stages driven from here, the default) or "device" (the whole
    frame in one call, replay_device: the reference's front end -- segmentation, processCloud's voxel grids, no padding;
    feature_cfg / sensor_height / segmenter / seg_cfg / sync do not apply, odom_cfg / init_pose do)."""
    if pipeline == "device":
        return replay_device(H, scan_files, out_poses, odom_cfg, init_pose, max_frames)
    if pipeline != "host":
        raise ValueError(f"unknown pipeline {pipeline!r}")
    poses, t_feat, t_match, t_submap, iters = [], [], [], [], 0
    files = scan_files[: max_frames] if max_frames else scan_files
    out = open(out_poses, "w") if out_poses else None
    try:
        for f, path in enumerate(files):
            xyz = np.asarray(path, np.float64).reshape(-1, 3) if isinstance(path, np.ndarray) else kitti_io.read_velodyne_bin(path)[0]
            t0 = time.perf_counter()
            frame, planar_submap, sphere_submap = features_of_scan(H, xyz, feature_cfg, sensor_height, segmenter, seg_cfg)
            t1 = time.perf_counter()
            if f == 0:                                   # first frame: the submap IS the scan (front_end.cpp:283-304)
                H.submap_init(planar_submap, sphere_submap, frame.edge, frame.ground)
                T = np.eye(4)
                t2 = t1
            else:
                pred = poses[-1] @ (np.linalg.inv(poses[-2]) @ poses[-1] if len(poses) > 1 else np.eye(4))  # :329-330
                H.set_input_source(frame)
                rc, T, st = H.scan_match(pred)
                if rc not in (0, -7):
                    name = os.path.basename(path) if isinstance(path, str) else "array"
                    raise RuntimeError(f"frame {f} ({name}): scan_match status {rc}")
                iters += st["gn_sweeps"]
                t2 = time.perf_counter()
                H.submap_update(T, planar_submap, sphere_submap, frame.edge, frame.ground)
            if sync:
                sync()
            t3 = time.perf_counter()
            poses.append(T)
            if out:
                out.write(kitti_io.format_pose_line(T))
            if f > 0:
                t_feat.append((t1 - t0) * 1e3); t_match.append((t2 - t1) * 1e3); t_submap.append((t3 - t2) * 1e3)
    finally:
        if out:
            out.close()
    m = lambda v: round(float(np.mean(v)), 4) if v else None  # noqa: E731
    return poses, {"frames": len(poses), "ms_features_incl_labeller": m(t_feat), "ms_set_source_plus_scan_match": m(t_match),
                   "ms_submap_update": m(t_submap), "gn_iters_per_frame": round(iters / max(len(poses) - 1, 1), 2)}
