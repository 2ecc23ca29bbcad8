"""The odometry frame (tloam_odometry_frame) against the stage chain driven from Python (tloam_segment -> numpy gathers ->
tloam_voxel_down_sample x 2 -> tloam_extract_planar_sphere -> numpy gathers -> tloam_set_source_frame -> tloam_scan_match ->
tloam_submap_update) on the same frames of a 120 k-return ray-cast HDL-64E sequence (tloam_amd/synth_hdl64.py, seed 3),
host call to host return per frame after a warm-up.  The two run in two contexts, alternating frame by frame.  Prints the
median / p90 ms per frame of each and the fused frame's copy / wait counters; the chain's are counted from its calls' code
(DESIGN.md section 12).  Run it under rocprofv3 --kernel-trace --stats for the kernels' own times.

    python scripts/odom_time.py [frames] [out.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from tloam_amd import registration as reg, synth_hdl64 as G  # noqa: E402
from tloam_amd.synth import Frame  # noqa: E402

WARM = 3
frames = int(sys.argv[1]) if len(sys.argv) > 1 else 24
out_path = sys.argv[2] if len(sys.argv) > 2 else None
scans, _ = G.sequence(frames, seed=3)
# the ray-cast street has nothing round: a wider PCA radius and a lower cvr_submap give the sphere lists their ten points
# (tests/test_gpu_odometry_frame.py)
cfg = reg.default_odom_config(feature__radius=0.5, feature__cvr_submap=0.05)


class Chain:
    """the stage chain with its host glue; h2d / d2h bytes are those the Python side moves through the calls"""
    def __init__(self):
        self.H = reg.HipRegistration()
        self.f = 0
        self.last = self.pred = np.eye(4)

    def frame(self, xyz):
        H = self.H
        S = H.segment(xyz, cfg.seg)
        ground, edge, general = xyz[S["ground"]], xyz[S["edge"]], xyz[S["general"]]
        ps, pm, ss, sm = H.extract_planar_sphere(general, cfg.feature)
        sel = lambda idx: np.ascontiguousarray(general[idx])  # noqa: E731
        up = 24 * (len(xyz) + len(general) + len(edge) + len(ground))
        down = 4 * (len(xyz) + len(S["ground"]) + len(S["object"]) + 2 * len(S["segmented"]) + len(S["edge"]) + len(S["general"]))
        down += 12 * (len(pm) + len(sm))   # the ranked lists: flatness + index
        if self.f == 0:
            H.submap_init(sel(pm), sel(sm), edge, ground, cfg.submap)
            T = np.eye(4)
        else:
            e_ds = H.voxel_down_sample(edge, cfg.edge_down_sample)
            g_ds = H.voxel_down_sample(ground, cfg.submap.ground_down_sample)
            H.set_input_source(Frame(sel(ps), g_ds, e_ds, sel(ss)))
            rc, T, st = H.scan_match(self.pred)
            H.submap_update(T, sel(pm), sel(sm), e_ds, g_ds)
            step = np.linalg.inv(self.last) @ T
            self.pred, self.last = T @ step, T
            up += 24 * (len(ps) + len(ss) + len(e_ds) + len(g_ds) + len(pm) + len(e_ds) + len(g_ds))
            down += 24 * (len(e_ds) + len(g_ds))
        self.f += 1
        return T, up, down


A = reg.HipRegistration()
A.odometry_reset(None, cfg)
B = Chain()
ta, tb, stats, up_b, down_b = [], [], [], [], []
for f, xyz in enumerate(scans):
    t0 = time.perf_counter()
    rc, Ta, st = A.odometry_frame(xyz)
    t1 = time.perf_counter()
    Tb, up, down = B.frame(xyz)
    t2 = time.perf_counter()
    assert rc == 0, (f, rc)
    if f >= WARM:
        ta.append((t1 - t0) * 1e3); tb.append((t2 - t1) * 1e3)
        stats.append(st); up_b.append(up); down_b.append(down)
ta, tb = np.array(ta), np.array(tb)
res = {
    "frames_timed": len(ta), "points_per_scan": int(np.mean([len(s) for s in scans])),
    "fused_ms_median": round(float(np.median(ta)), 4), "fused_ms_p90": round(float(np.percentile(ta, 90)), 4),
    "chain_ms_median": round(float(np.median(tb)), 4), "chain_ms_p90": round(float(np.percentile(tb, 90)), 4),
    "fused_h2d_bytes_mean": float(np.mean([s["h2d_bytes"] for s in stats])),
    "fused_d2h_bytes_mean": float(np.mean([s["d2h_bytes"] for s in stats])),
    "fused_host_syncs": sorted({s["host_syncs"] for s in stats}),
    "chain_h2d_bytes_mean": float(np.mean(up_b)), "chain_d2h_bytes_mean": float(np.mean(down_b)),
    "chain_host_syncs": 11,
    "pose_gap_m_last": float(np.linalg.norm(Ta[:3, 3] - Tb[:3, 3])),
}
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
