"""What place recognition adds to the odometry frame: one 120 k-return ray-cast HDL-64E sequence
(tloam_amd/synth_hdl64.py, seed 3) through tloam_odometry_frame with place recognition on and with it off, in two contexts,
alternating frame by frame, host call to host return after a warm-up.  Every frame is a keyframe (kf_dist 0.5 m against a
1.2 m step) and, from the third on, is searched (exclude_recent 2): the worst case of the frame's path.  Also times
tloam_place_add_scan, which waits for its launches, on the same scans.  Prints the median / p90 ms of each.  Run it under
rocprofv3 --kernel-trace --stats for the kernels' own times.

    python scripts/place_time.py [frames] [out.json]"""
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
scans, poses = G.sequence(frames, seed=3)
# (tests/test_gpu_odometry_frame.py: the street has nothing round)
cfg = reg.default_odom_config(feature__radius=0.5, feature__cvr_submap=0.05)
place = dict(kf_dist=0.5, exclude_recent=2)

on, off, add = reg.HipRegistration(), reg.HipRegistration(), reg.HipRegistration()
on.place_configure(enabled=1, **place)
add.place_configure(enabled=1, **place)
for H in (on, off):
    H.odometry_reset(None, cfg)
t_on, t_off, t_add, d2h_on, d2h_off, syncs = [], [], [], [], [], set()
for f, xyz in enumerate(scans):
    t0 = time.perf_counter()
    rc_a, Ta, sa = on.odometry_frame(xyz)
    t1 = time.perf_counter()
    rc_b, Tb, sb = off.odometry_frame(xyz)
    t2 = time.perf_counter()
    add.place_add_scan(xyz, poses[f], f)
    t3 = time.perf_counter()
    assert rc_a == 0 and rc_b == 0 and Ta.tobytes() == Tb.tobytes(), (f, rc_a, rc_b)
    if f >= WARM:
        t_on.append((t1 - t0) * 1e3); t_off.append((t2 - t1) * 1e3); t_add.append((t3 - t2) * 1e3)
        d2h_on.append(sa["d2h_bytes"]); d2h_off.append(sb["d2h_bytes"]); syncs.add(sa["host_syncs"])
t_on, t_off = np.array(t_on), np.array(t_off)
med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
p90 = lambda v: round(float(np.percentile(v, 90)), 4)  # noqa: E731
t0 = time.perf_counter()
info = on.place_info()   # (waits for the last keyframe's launches)
t_info = (time.perf_counter() - t0) * 1e3
res = {
    "frames_timed": len(t_on), "points_per_scan": int(np.mean([len(s) for s in scans])),
    "place_on_ms_median": med(t_on), "place_on_ms_p90": p90(t_on),
    "place_off_ms_median": med(t_off), "place_off_ms_p90": p90(t_off),
    "added_ms_median": round(float(np.median(t_on - t_off)), 4),
    "add_scan_ms_median": med(t_add), "add_scan_ms_p90": p90(t_add),
    "info_after_last_frame_ms": round(t_info, 4),
    "keyframes": info["n_keyframes"], "loops": info["n_loops"], "capacity_keyframes": info["capacity_keyframes"],
    "add_scan_keyframes": add.place_info()["n_keyframes"],
    "host_syncs_place_on": sorted(syncs),
    "d2h_bytes_place_on_mean": float(np.mean(d2h_on)), "d2h_bytes_place_off_mean": float(np.mean(d2h_off)),
}
for H in (on, off, add):
    H.close()
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
