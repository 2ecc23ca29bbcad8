"""The cost of one verified loop on the device: on out-and-back street 1 (16 + 16 keyframes with true poses,
full-density clouds through the public stage calls, as tests/test_gpu_loop.py), every loop record verified through
tloam_loop_verify_pair from its Scan Context start, host to host, after one warm-up pass; and the device memory the two child
contexts take (hipMemGetInfo through torch, before the first verification and after).  Run it under
`rocprofv3 --kernel-trace --stats` for the kernel times.  Needs an MI355X.

    python scripts/loop_time.py [out.json] [--reps N]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]
from loop_thres import FEATURE, N_OUT, EX, THIN, lists  # noqa: E402
from tloam_amd import registration as reg  # noqa: E402
from tloam_amd import synth_revisit as RV  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    path = args[0] if args else os.path.join(ROOT, "profiles", "loop_time.json")
    import torch
    cfg = reg.default_odom_config(**{f"feature__{k}": v for k, v in FEATURE.items()})
    thin, poses, _ = RV.out_and_back(N_OUT, seed=1, **THIN)
    full, _, _ = RV.out_and_back(N_OUT, seed=1)
    H = reg.HipRegistration()
    kf = [lists(H, xyz, cfg) for xyz in full]
    H.place_configure(enabled=1, exclude_recent=EX)
    H.loop_configure(enabled=1)
    for f, (s, T) in enumerate(zip(thin, poses)):
        H.place_add_scan(s, T, f)
        H.place_set_keyframe_clouds(f, *kf[f])
    loops = H.place_loops()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    first = H.loop_verify_pair(loops[0]["query"], loops[0]["match"], _rz(loops[0]["yaw"]))
    free1 = torch.cuda.mem_get_info()[0]
    times, pts = [], []
    for _ in range(reps):
        for L in loops:
            t0 = time.perf_counter()
            c = H.loop_verify_pair(L["query"], L["match"], _rz(L["yaw"]))
            times.append((time.perf_counter() - t0) * 1e3)
            pts.append((c["points"], c["coarse"]["n_corr"], c["fine"]["outer_iterations"]))
    H.close()
    out = {"loops": len(loops), "reps": reps, "ms_per_verified_loop_median": float(np.median(times)),
           "ms_p10": float(np.percentile(times, 10)), "ms_p90": float(np.percentile(times, 90)),
           "source_points": [int(min(p[0] for p in pts)), int(max(p[0] for p in pts))],
           "child_contexts_device_MiB": (free0 - free1) / 2**20, "first_status": first["status"]}
    print(json.dumps(out, indent=1))
    json.dump(out, open(path, "w"), indent=1)


def _rz(yaw):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    return T


if __name__ == "__main__":
    main()
