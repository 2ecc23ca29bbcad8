"""Tracking with the deskew off, on in azimuth mode and on in timed mode, against the generator:
12-frame swept sequences (tloam_amd/synth_sweep.py, 0.8 m and 0.03 rad per frame), seeds 3 and 5, moving from the first frame
(rest 0) and after two frames at rest (rest 2).  Prints the translation error of every frame.

    python scripts/deskew_track.py [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from conftest import pose_delta  # noqa: E402
from tloam_amd import registration as reg, synth_sweep as SW  # noqa: E402

TWIST = np.array([0.8, 0.0, 0.0, 0.0, 0.0, 0.03])
# the ray-cast street has nothing round: a wider PCA radius and a lower cvr_submap (tests/test_gpu_odometry_frame.py)
cfg = reg.default_odom_config(feature__radius=0.5, feature__cvr_submap=0.05)


def run(scans, times, dc):
    H = reg.HipRegistration()
    if dc is not None:
        H.deskew_configure(dc)
    H.odometry_reset(None, cfg)
    poses = []
    for f, xyz in enumerate(scans):
        rc, T, _ = H.odometry_frame(xyz, times[f] if dc is not None and dc.time_source == 1 else None)
        poses.append(T if rc in (0, -7) else None)
    H.close()
    return poses


out = {}
for rest in (0, 2):
    for seed in (3, 5):
        scans, times, truth, _ = SW.sequence(12, TWIST, seed=seed, rest_frames=rest)
        for name, dc in (("off", None), ("azimuth", reg.default_deskew_config(enabled=1)),
                         ("timed", reg.default_deskew_config(enabled=1, time_source=1))):
            d = [pose_delta(a, b) if a is not None else (np.nan, np.nan) for a, b in zip(run(scans, times, dc), truth)]
            dt = [round(x[0], 4) for x in d]
            dr = [round(x[1], 5) for x in d]
            key = f"rest{rest}_seed{seed}_{name}"
            out[key] = {"mean_t": round(float(np.nanmean(dt)), 4), "max_t": float(np.nanmax(dt)),
                        "max_t_from_3": float(np.nanmax(dt[3:])), "max_r": float(np.nanmax(dr)), "dt": dt}
            print(key, json.dumps(out[key]), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
