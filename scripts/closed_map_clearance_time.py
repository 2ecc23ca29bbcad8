"""The cost of the closed map's clearance on the device: tloam_closed_map_clearance_build at R = 4, 8 and
20 cells, _clearance_points of a 120 k-return scan, _clearance_segments of 100 k segments of 10 m and a column field, host to
host (each the median of five after a warm-up), over the free-space grid at its default configuration (60 m rays, the auto box),
on the inputs of scripts/closed_map_free_time.py:
  static   the static pass of tests/carve_scenes.py (8 keyframes, 0.5 m voxels, mask 0x10);
  32, 200  the inputs of scripts/closed_map_time.py (1 m voxels, mask 0xF0).
Beside them, on one core of the host: scipy.ndimage.distance_transform_edt over the same obstacle cells (the numpy restatement's
transform at R = 8 where scipy does not import), which is what a caller had to run before.

Every size is a child process of its own under a time limit, and the first one that fails ends the run.  Run one size under
`rocprofv3 --kernel-trace --stats -- python scripts/closed_map_clearance_time.py --size K` for the kernels' own times
(profiles/closed_map_clearance_kernel_stats.csv).  Needs an MI355X.

    python scripts/closed_map_clearance_time.py [out.json]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SIZES = ("static", "32", "200")
LIMIT_S = {"static": 300, "32": 360, "200": 420}
REPS = 5
RADII = (4, 8, 20)
N_SEGMENTS, SEGMENT_M = 100000, 10.0


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def median_of(call):
    call()   # warm-up
    ms = [timed(call) for _ in range(REPS)]
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def host_transform(obstacle):
    """the transform a caller had to run on the host -> (what ran, seconds)"""
    try:
        from scipy import ndimage
        t0 = time.perf_counter()
        ndimage.distance_transform_edt(~obstacle)
        return "scipy.ndimage.distance_transform_edt", time.perf_counter() - t0
    except ImportError:
        import closed_map_clearance_np as KN
        t0 = time.perf_counter()
        KN.transform(obstacle, 8, False)
        return "tests/closed_map_clearance_np.py transform, R = 8", time.perf_counter() - t0


def one_size(size):
    from closed_map_relocalise_time import pass_input, static_input
    from tloam_amd import registration as reg
    H, scan, pose = static_input(reg) if size == "static" else pass_input(reg, int(size))
    built = H.closed_map_info()
    voxel = 0.5 if size == "static" else 1.0   # (what static_input / pass_input configure)
    free = H.closed_map_free_build()
    out = {"size": size, "keyframes": built["n_keyframes"], "voxels": built["n_voxels"], "voxel": voxel, "n_bricks": free["n_bricks"],
           "free_cells": free["free_cells"], "builds": []}
    for wrap in (1, 0):
        for R in RADII:
            H.closed_map_clearance_configure(max_distance=R * voxel, unknown_is_obstacle=wrap)
            first = H.closed_map_clearance_build()
            field = H.closed_map_clearance_field().tobytes()
            ms = median_of(H.closed_map_clearance_build)
            info = H.closed_map_clearance_info()
            assert info == first and H.closed_map_clearance_field().tobytes() == field   # every build gives the same bytes
            out["builds"].append({"R": R, "unknown_is_obstacle": wrap, "cells": int(np.prod(info["n_cells"])), "bytes": info["bytes"],
                                  "obstacle_cells": info["obstacle_cells"], "finite_cells": info["finite_cells"],
                                  "sum_d2": info["sum_d2"], "max_d2": info["max_d2"], "launches": info["launches"],
                                  "build_ms_median": ms[0], "build_ms_min": ms[1], "build_ms_max": ms[2],
                                  "cells_per_s_whole_call": float(np.prod(info["n_cells"])) / (ms[0] * 1e-3)})
    # the queries, on the last field (R = 20, only voxels are obstacles)
    info = H.closed_map_clearance_info()
    pms = median_of(lambda: H.closed_map_clearance_points(scan, pose))
    state, d2, _, counts = H.closed_map_clearance_points(scan, pose)
    rng = np.random.default_rng(7)
    lo = voxel * np.asarray(info["lo_cells"], np.float64)
    hi = lo + voxel * np.asarray(info["n_cells"], np.float64)
    mid, half = 0.5 * (lo + hi), 0.25 * (hi - lo)
    S = rng.uniform(mid - half, mid + half, (N_SEGMENTS, 3))
    d = rng.normal(size=(N_SEGMENTS, 3))
    d[:, 2] *= 0.1
    E = S + SEGMENT_M * d / np.linalg.norm(d, axis=1)[:, None]
    sms = median_of(lambda: H.closed_map_clearance_segments(S, E, voxel))
    status, least, _, scounts = H.closed_map_clearance_segments(S, E, voxel)
    cms = median_of(lambda: H.closed_map_clearance_columns(0.0, 2.0))
    fms = median_of(lambda: H.closed_map_free_columns(0.0, 2.0))
    obstacle = H.closed_map_clearance_field() == 0
    H.close()
    what, seconds = host_transform(obstacle)
    out.update({"points": len(scan), "points_ms_median": pms[0], "points_counts": [int(x) for x in counts],
                "points_finite": int((d2 < 0xFFFE).sum()),
                "segments": N_SEGMENTS, "segment_m": SEGMENT_M, "segments_radius_m": voxel, "segments_ms_median": sms[0],
                "segments_counts": [int(x) for x in scounts], "columns_ms_median": cms[0], "free_columns_ms_median": fms[0],
                "host_transform": what, "host_transform_s": seconds})
    return out


def main():
    if "--size" in sys.argv:   # a child: one size, one JSON line
        print("RESULT " + json.dumps(one_size(sys.argv[sys.argv.index("--size") + 1])), flush=True)
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "closed_map_clearance_time.json")
    out = {"reps": REPS, "sizes": []}
    for size in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), "--size", size]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT_S[size])
            text, rc = p.stdout, p.returncode
        except subprocess.TimeoutExpired:
            text, rc = "", 124
        rows = [ln for ln in text.splitlines() if ln.startswith("RESULT ")]
        if rc != 0 or not rows:   # a fault, an abort, a time limit or a failed check: nothing more is started on the device
            print(f"size {size}: exit status {rc}; stopping", flush=True)
            json.dump(out, open(path, "w"), indent=1)
            sys.exit(1)
        r = json.loads(rows[-1][7:])
        print(json.dumps(r), flush=True)
        out["sizes"].append(r)
        json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
