"""What the deskew adds to the odometry frame: one 120 k-return swept HDL-64E sequence
(tloam_amd/synth_sweep.py, seed 3, 0.8 m and 0.03 rad per frame) through the odometry frame with deskew off, on in azimuth mode
and on in timed mode, in three contexts, alternating frame by frame, host call to host return after a warm-up.  Prints the
median / p90 ms per frame of each and what each frame moved.  Run it under rocprofv3 --kernel-trace --stats for the kernel's
own time.

    python scripts/deskew_time.py [frames] [out.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from tloam_amd import registration as reg, synth_sweep as SW  # noqa: E402

WARM = 3
TWIST = np.array([0.8, 0.0, 0.0, 0.0, 0.0, 0.03])
frames = int(sys.argv[1]) if len(sys.argv) > 1 else 24
out_path = sys.argv[2] if len(sys.argv) > 2 else None
scans, times, poses, _ = SW.sequence(frames, TWIST, seed=3)
# the ray-cast street has nothing round: a wider PCA radius and a lower cvr_submap (tests/test_gpu_odometry_frame.py)
cfg = reg.default_odom_config(feature__radius=0.5, feature__cvr_submap=0.05)

off, az, tm = reg.HipRegistration(), reg.HipRegistration(), reg.HipRegistration()
az.deskew_configure(reg.default_deskew_config(enabled=1))
tm.deskew_configure(reg.default_deskew_config(enabled=1, time_source=1))
for H in (off, az, tm):
    H.odometry_reset(None, cfg)
t_off, t_az, t_tm, shift, syncs, h2d, skipped = [], [], [], [], set(), {}, []
for f, xyz in enumerate(scans):
    t0 = time.perf_counter()
    rc_a, _, sa = off.odometry_frame(xyz)
    t1 = time.perf_counter()
    rc_b, _, sb = az.odometry_frame(xyz)
    t2 = time.perf_counter()
    rc_c, _, sc = tm.odometry_frame(xyz, times[f])
    t3 = time.perf_counter()
    assert rc_a in (0, -2, -7) and rc_b in (0, -2, -7) and rc_c in (0, -2, -7), (f, rc_a, rc_b, rc_c)
    if -2 in (rc_a, rc_b, rc_c):   # a frame one of them skipped (too few points in a cloud) is not timed
        skipped.append((f, rc_a, rc_b, rc_c))
        continue
    if f >= 2:
        shift.append(round(az.deskew_info()["last_max_shift"], 4))
    if f >= max(WARM, 2):
        t_off.append((t1 - t0) * 1e3); t_az.append((t2 - t1) * 1e3); t_tm.append((t3 - t2) * 1e3)
        syncs.update((sb["host_syncs"], sc["host_syncs"]))
        h2d = {"off": sa["h2d_bytes"], "azimuth": sb["h2d_bytes"], "timed": sc["h2d_bytes"], "n": len(xyz)}
t_off, t_az, t_tm = np.array(t_off), np.array(t_az), np.array(t_tm)
med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
p90 = lambda v: round(float(np.percentile(v, 90)), 4)  # noqa: E731
res = {
    "frames_timed": len(t_off), "points_per_scan": int(np.mean([len(s) for s in scans])),
    "off_ms_median": med(t_off), "off_ms_p90": p90(t_off),
    "azimuth_ms_median": med(t_az), "azimuth_ms_p90": p90(t_az),
    "timed_ms_median": med(t_tm), "timed_ms_p90": p90(t_tm),
    "azimuth_added_ms_median": round(float(np.median(t_az - t_off)), 4),
    "timed_added_ms_median": round(float(np.median(t_tm - t_off)), 4),
    "max_shift_m_per_frame": shift, "host_syncs_deskew_on": sorted(syncs), "h2d_bytes_last_frame": h2d,
    "skipped_frames": skipped,
    "frames_deskewed": {"azimuth": az.deskew_info()["frames_deskewed"], "timed": tm.deskew_info()["frames_deskewed"]},
}
for H in (off, az, tm):
    H.close()
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
