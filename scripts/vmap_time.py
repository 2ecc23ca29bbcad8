"""What the merged voxel map adds to the odometry frame: one 120 k-return ray-cast HDL-64E sequence
(tloam_amd/synth_hdl64.py, seed 3) through tloam_odometry_frame with the voxel map on and with it off, in two contexts,
alternating frame by frame, host call to host return after a warm-up.  Prints the median / p90 ms per frame of each, the
voxels each frame creates, and the map's size against the append map's (which a third context keeps on the same scans,
untimed).  Run it under rocprofv3 --kernel-trace --stats for the kernels' own times.

    python scripts/vmap_time.py [frames] [out.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from tloam_amd import registration as reg, synth_hdl64 as G  # noqa: E402

WARM = 3
frames = int(sys.argv[1]) if len(sys.argv) > 1 else 24
out_path = sys.argv[2] if len(sys.argv) > 2 else None
scans, _ = G.sequence(frames, seed=3)
# the ray-cast street has nothing round: a wider PCA radius and a lower cvr_submap give the sphere lists their ten points
# (tests/test_gpu_odometry_frame.py)
cfg = reg.default_odom_config(feature__radius=0.5, feature__cvr_submap=0.05)

on, off, app = reg.HipRegistration(), reg.HipRegistration(), reg.HipRegistration()
on.voxel_map_configure(reg.default_voxel_map_config(enabled=1))
app.map_configure(reg.default_map_config(enabled=1))
for H in (on, off, app):
    H.odometry_reset(None, cfg)
t_on, t_off, new, d2h_on, d2h_off, syncs = [], [], [], [], [], set()
for f, xyz in enumerate(scans):
    t0 = time.perf_counter()
    rc_a, Ta, sa = on.odometry_frame(xyz)
    t1 = time.perf_counter()
    rc_b, Tb, sb = off.odometry_frame(xyz)
    t2 = time.perf_counter()
    rc_c, Tc, _ = app.odometry_frame(xyz)
    assert rc_a == 0 and rc_b == 0 and rc_c == 0 and Ta.tobytes() == Tb.tobytes() == Tc.tobytes(), (f, rc_a, rc_b, rc_c)
    if f == 0:
        continue   # (the first frame adds nothing)
    new.append(on.voxel_map_info()["last_new"])
    if f >= WARM:
        t_on.append((t1 - t0) * 1e3); t_off.append((t2 - t1) * 1e3)
        d2h_on.append(sa["d2h_bytes"]); d2h_off.append(sb["d2h_bytes"]); syncs.add(sa["host_syncs"])
t_on, t_off = np.array(t_on), np.array(t_off)
med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
p90 = lambda v: round(float(np.percentile(v, 90)), 4)  # noqa: E731
vi, mi = on.voxel_map_info(), app.map_info()
t0 = time.perf_counter()
cen, cnt = on.voxel_map_read()
t_read = (time.perf_counter() - t0) * 1e3
t0 = time.perf_counter()
bc, _ = on.voxel_map_read_box((-20, -20, -5), (20, 20, 5), 1)
t_box = (time.perf_counter() - t0) * 1e3
res = {
    "frames_timed": len(t_on), "points_per_scan": int(np.mean([len(s) for s in scans])),
    "vmap_on_ms_median": med(t_on), "vmap_on_ms_p90": p90(t_on),
    "vmap_off_ms_median": med(t_off), "vmap_off_ms_p90": p90(t_off),
    "added_ms_median": round(float(np.median(t_on - t_off)), 4),
    "new_voxels_per_frame": new, "n_voxels": vi["n_voxels"], "n_points": vi["n_points"], "n_frames": vi["n_frames"],
    "capacity_voxels": vi["capacity_voxels"],
    # rows in HBM: key + N + Qx + Qy + Qz (40 B per voxel) and the table (4 B per slot, load <= 1/2), at capacity
    "vmap_hbm_bytes_used": 40 * vi["n_voxels"], "vmap_hbm_bytes_reserved": 40 * vi["capacity_voxels"] + 8 * vi["capacity_voxels"],
    "append_map_points": mi["n_points"], "append_map_hbm_bytes_used": 24 * mi["n_points"],
    "read_all_ms": round(t_read, 4), "read_box_ms": round(t_box, 4), "read_box_voxels": len(bc),
    "host_syncs_vmap_on": sorted(syncs),
    "d2h_bytes_vmap_on_mean": float(np.mean(d2h_on)), "d2h_bytes_vmap_off_mean": float(np.mean(d2h_off)),
}
for H in (on, off, app):
    H.close()
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
