"""What the global map adds to the odometry frame: one 120 k-return ray-cast HDL-64E sequence
(tloam_amd/synth_hdl64.py, seed 3) through tloam_odometry_frame with mapping on and with mapping off, in two contexts,
alternating frame by frame, host call to host return after a warm-up.  Prints the median / p90 ms per frame of each, the
map's growth per frame, and what the same step costs a host that does it on the CPU: the oracle's pc_transform +
pc_voxel_down_sample (oracle/submap_oracle.c, the C statements of Open3D's Transform and VoxelDownSample) on the same
scans and poses.  Run it under rocprofv3 --kernel-trace --stats for the kernels' own times.

    python scripts/map_time.py [frames] [out.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from oracle import binding as ob  # noqa: E402
from tloam_amd import registration as reg, synth_hdl64 as G  # noqa: E402

WARM = 3
frames = int(sys.argv[1]) if len(sys.argv) > 1 else 24
out_path = sys.argv[2] if len(sys.argv) > 2 else None
scans, _ = G.sequence(frames, seed=3)
# the ray-cast street has nothing round: a wider PCA radius and a lower cvr_submap give the sphere lists their ten points
# (tests/test_gpu_odometry_frame.py)
cfg = reg.default_odom_config(feature__radius=0.5, feature__cvr_submap=0.05)

on, off = reg.HipRegistration(), reg.HipRegistration()
on.map_configure(reg.default_map_config(enabled=1))
on.odometry_reset(None, cfg)
off.odometry_reset(None, cfg)
t_on, t_off, t_cpu, growth, d2h_on, d2h_off, syncs = [], [], [], [], [], [], set()
for f, xyz in enumerate(scans):
    t0 = time.perf_counter()
    rc_a, Ta, sa = on.odometry_frame(xyz)
    t1 = time.perf_counter()
    rc_b, Tb, sb = off.odometry_frame(xyz)
    t2 = time.perf_counter()
    assert rc_a == 0 and rc_b == 0 and Ta.tobytes() == Tb.tobytes(), (f, rc_a, rc_b)
    if f == 0:
        continue   # (:304: the first frame adds nothing)
    c0 = time.perf_counter()
    cpu = ob.pc_voxel_down_sample(ob.pc_transform(Ta, xyz), 1.0)   # the host-side step a front end would otherwise run
    c1 = time.perf_counter()
    info = on.map_info()
    assert info["last_count"] == len(cpu), f
    growth.append(info["last_count"])
    if f >= WARM:
        t_on.append((t1 - t0) * 1e3); t_off.append((t2 - t1) * 1e3); t_cpu.append((c1 - c0) * 1e3)
        d2h_on.append(sa["d2h_bytes"]); d2h_off.append(sb["d2h_bytes"]); syncs.add(sa["host_syncs"])
t_on, t_off, t_cpu = np.array(t_on), np.array(t_off), np.array(t_cpu)
med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
p90 = lambda v: round(float(np.percentile(v, 90)), 4)  # noqa: E731
info = on.map_info()
res = {
    "frames_timed": len(t_on), "points_per_scan": int(np.mean([len(s) for s in scans])),
    "mapping_on_ms_median": med(t_on), "mapping_on_ms_p90": p90(t_on),
    "mapping_off_ms_median": med(t_off), "mapping_off_ms_p90": p90(t_off),
    "added_ms_median": round(float(np.median(t_on - t_off)), 4),
    "cpu_transform_voxel_ms_median": med(t_cpu), "cpu_transform_voxel_ms_p90": p90(t_cpu),
    "map_points_per_frame": growth, "map_points": info["n_points"], "map_frames": info["n_frames"],
    "map_capacity_points": info["capacity_points"],
    "host_syncs_mapping_on": sorted(syncs),
    "d2h_bytes_mapping_on_mean": float(np.mean(d2h_on)), "d2h_bytes_mapping_off_mean": float(np.mean(d2h_off)),
}
on.close()
off.close()
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
