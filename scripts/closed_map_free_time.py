"""The cost of the closed map's free space on the device: tloam_closed_map_free_reset,
_free_add_keyframes and _free_add_scan host to host (each the median of five after a warm-up; the grid is reset, untimed, before
every timed add, so that every add starts from zero words and pays its atomics), at the default configuration (60 m rays, the
auto box), on the inputs of scripts/closed_map_diff_time.py:
  static   the static pass of tests/carve_scenes.py (8 keyframes, 0.5 m voxels, mask 0x10), the scan taken midway between
           keyframes 3 and 4;
  32, 200  the inputs of scripts/closed_map_time.py and scripts/closed_map_carve_time.py (1 m voxels, mask 0xF0), the scan at
           frame 3's pose.
The scan is a 120 k-return one.  Beside each, in the same process: a carve of the same map (host to host: the walk to hold the
free walk against), the occupancy of the scan's points, the read of the free cells and a column grid.  An add over a grid that
already holds its bits (no atomic is issued: every flush finds its bits set) is timed too.

Every size is a child process of its own under a time limit, and the first one that fails ends the run.  Run one size under
`rocprofv3 --kernel-trace --stats -- python scripts/closed_map_free_time.py --size K` for the kernels' own times
(profiles/closed_map_free_kernel_stats.csv).  Needs an MI355X.

    python scripts/closed_map_free_time.py [out.json]"""
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
LIMIT_S = {"static": 240, "32": 300, "200": 360}
REPS = 5


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def median_after_reset(H, call):
    """the median of REPS timed calls, each on a freshly zeroed grid"""
    ms = []
    for _ in range(REPS):
        H.closed_map_free_reset()
        ms.append(timed(call))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def one_size(size):
    from closed_map_relocalise_time import pass_input, static_input
    from tloam_amd import registration as reg
    H, scan, pose = static_input(reg) if size == "static" else pass_input(reg, int(size))
    built = H.closed_map_info()
    carve = H.closed_map_carve()   # warm-up
    cms = [timed(H.closed_map_carve) for _ in range(REPS)]
    first = H.closed_map_free_build()   # warm-up (the allocation)
    words = H.closed_map_free_words().tobytes()
    rms = [timed(H.closed_map_free_reset) for _ in range(REPS)]
    kms = median_after_reset(H, H.closed_map_free_add_keyframes)
    info = H.closed_map_free_info()
    assert info == first and H.closed_map_free_words().tobytes() == words   # every build gives the same bytes
    H.closed_map_free_reset()
    H.closed_map_free_add_scan(scan, pose)   # warm-up (the scan's buffer)
    sms = median_after_reset(H, lambda: H.closed_map_free_add_scan(scan, pose))
    sinfo = H.closed_map_free_info()
    again = [timed(lambda: H.closed_map_free_add_scan(scan, pose)) for _ in range(REPS)]   # the bits are there: no atomic
    assert H.closed_map_free_info()["free_cells"] == sinfo["free_cells"]
    H.closed_map_free_build()
    H.closed_map_occupancy(scan, pose)   # warm-up
    oms = [timed(lambda: H.closed_map_occupancy(scan, pose)) for _ in range(REPS)]
    counts = H.closed_map_occupancy(scan, pose)[2]
    cells = H.closed_map_free_cells()
    fms = [timed(H.closed_map_free_cells) for _ in range(REPS)]
    lms = [timed(lambda: H.closed_map_free_columns(0.0, 2.0)) for _ in range(REPS)]
    H.close()
    cmed, kmed, smed = float(np.median(cms)), kms[0], sms[0]
    walked, swalked = info["cells_marked"] + info["cells_outside"], sinfo["cells_marked"] + sinfo["cells_outside"]
    return {"size": size, "keyframes": built["n_keyframes"], "voxels": built["n_voxels"],
            "n_bricks": info["n_bricks"], "grid_bytes": info["bytes"], "reset_ms_median": float(np.median(rms)),
            "rays": info["rays"], "skipped_rays": info["skipped_rays"], "cells_marked": info["cells_marked"],
            "cells_outside": info["cells_outside"], "free_cells": info["free_cells"], "bricks_nonzero": info["bricks_nonzero"],
            "add_keyframes_ms_median": kmed, "add_keyframes_ms_min": kms[1], "add_keyframes_ms_max": kms[2],
            "cells_per_s_whole_call": walked / (kmed * 1e-3),
            "carve_steps": carve["steps"], "carve_ms_median": cmed, "carve_steps_per_s_whole_call": carve["steps"] / (cmed * 1e-3),
            "scan_points": len(scan), "scan_skipped_rays": sinfo["skipped_rays"], "scan_cells_marked": sinfo["cells_marked"],
            "scan_cells_outside": sinfo["cells_outside"], "scan_free_cells": sinfo["free_cells"],
            "add_scan_ms_median": smed, "add_scan_ms_min": sms[1], "add_scan_ms_max": sms[2],
            "scan_cells_per_s_whole_call": swalked / (smed * 1e-3), "add_scan_bits_already_set_ms_median": float(np.median(again)),
            "occupancy_ms_median": float(np.median(oms)), "occupancy_counts": [int(x) for x in counts],
            "read_free_cells": len(cells), "read_free_ms_median": float(np.median(fms)), "columns_ms_median": float(np.median(lms))}


def main():
    if "--size" in sys.argv:   # a child: one size, one JSON line
        print("RESULT " + json.dumps(one_size(sys.argv[sys.argv.index("--size") + 1])), flush=True)
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "closed_map_free_time.json")
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
