"""Where place recognition's default dist_thres comes from: the best d of every searched keyframe on the
generator's sequences (tloam_amd/synth_revisit.py, 32 of the 64 rings, 600 azimuth steps), split into true revisits (an
old-enough keyframe lies within 3 m) and non-revisits, with the true-pose search of tests/place_np.py (which the device equals
bit for bit, tests/test_gpu_place.py).  Four out-and-back passes of 20 + 20 keyframes and four one-way passes of 40, seeds 0-3,
exclude_recent 10.  Runs on the CPU.

    python scripts/place_thres.py [out.json]"""
import json
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import place_np as P  # noqa: E402
from tloam_amd import synth_revisit as RV  # noqa: E402

THIN = dict(n_az=600, rings=np.arange(0, 64, 2))
EX = 10


def job(task):
    kind, seed = task
    if kind == "out_and_back":
        scans, poses, _ = RV.out_and_back(20, seed=seed, **THIN)
    else:
        scans, poses = RV.one_way(40, seed=seed, **THIN)
    db = P.PlaceDB(exclude_recent=EX, dist_thres=-1.0)   # (records nothing: the best pair of every search is kept here)
    rev, non = [], []
    for f, (s, T) in enumerate(zip(scans, poses)):
        db.add(s, T, f)
        best = db.search(f)
        if best is None:
            continue
        d, shift, m = best
        near = any(np.linalg.norm(poses[k][:3, 3] - T[:3, 3]) < 3.0 for k in range(f - EX + 1))
        right = bool(np.linalg.norm(poses[m][:3, 3] - T[:3, 3]) < 3.0)
        yaw_err = abs((P.yaw_of(shift, 60) - RV.relative_yaw(T, poses[m]) + np.pi) % (2 * np.pi) - np.pi)
        (rev if near else non).append({"d": d, "match_right": right, "yaw_err": yaw_err})
    return kind, seed, rev, non


if __name__ == "__main__":
    tasks = [(k, s) for k in ("out_and_back", "one_way") for s in range(4)]
    with Pool(min(8, len(tasks))) as pool:
        res = pool.map(job, tasks)
    rev = [r for _, _, rv, _ in res for r in rv]
    non = [r for _, _, _, nn in res for r in nn]
    rd, nd = np.array([r["d"] for r in rev]), np.array([r["d"] for r in non])
    out = {"revisits": len(rev), "non_revisits": len(non),
           "revisit_d_min": float(rd.min()), "revisit_d_median": float(np.median(rd)), "revisit_d_max": float(rd.max()),
           "non_revisit_d_min": float(nd.min()), "non_revisit_d_median": float(np.median(nd)),
           "non_revisit_d_max": float(nd.max()),
           "revisit_best_match_right": sum(r["match_right"] for r in rev),
           "revisit_yaw_err_max": float(max(r["yaw_err"] for r in rev)),
           "per_sequence": {f"{k}_{s}": {"revisit_d": [round(r["d"], 4) for r in rv], "non_revisit_d": [round(r["d"], 4) for r in nn]}
                            for k, s, rv, nn in res}}
    print(json.dumps({k: v for k, v in out.items() if k != "per_sequence"}))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)
