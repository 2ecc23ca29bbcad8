"""The cost of the closed map's view gain on the device: tloam_closed_map_view_gain of V = 1, 8, 32 and
256 views -- the kept frontier clusters' approach points (closed_map_frontier_costs' after a route from one goal), recycled -- under
a 16 x 360 firing pattern at max_range 20, with each form forced in turn and the global form at one block a view against the
library's own choice, host to host (each the median of five after a warm-up); then the explorer's one call,
_frontier_gains, on the inputs of scripts/closed_map_frontier_time.py:
  static   the static pass of tests/carve_scenes.py (8 keyframes, 0.5 m voxels, mask 0x10);
  32, 200  the inputs of scripts/closed_map_time.py (1 m voxels, mask 0xF0).
Beside them, in the same session: the numpy restatement (tests/closed_map_view_np.py) of one view on one core, its record
asserted equal to the device's, and a ray-cast of the same pattern from the same pose.  There is no gate.

Every size is a child process of its own under a time limit, and the first one that fails ends the run.  Needs an MI355X.

    python scripts/closed_map_view_time.py [out.json]"""
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
LIMIT_S = {"static": 300, "32": 300, "200": 300}
REPS = 5
R_CELLS = 4
VIEWS = (1, 8, 32, 256)
RINGS, N_AZ, MAX_RANGE = 16, 360, 20.0
FORMS = (("lds", 1, None), ("global, 1 block a view", 2, "1"), ("global, auto", 2, None))


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def median_of(call):
    call()   # warm-up
    ms = [timed(call) for _ in range(REPS)]
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def blocks(n):
    os.environ.pop("TLOAM_VIEW_BLOCKS", None)
    if n is not None:
        os.environ["TLOAM_VIEW_BLOCKS"] = n


def one_size(size, host=True):
    from closed_map_relocalise_time import pass_input, static_input
    from tloam_amd import registration as reg
    from tloam_amd.raycast import lidar_pattern
    H, scan, pose = static_input(reg) if size == "static" else pass_input(reg, int(size))
    built = H.closed_map_info()
    voxel = 0.5 if size == "static" else 1.0   # (what static_input / pass_input configure)
    H.closed_map_free_configure(carve_gate=0)
    H.closed_map_free_build()
    info = H.closed_map_frontier_build()
    H.closed_map_clearance_configure(max_distance=R_CELLS * voxel, unknown_is_obstacle=1)
    clear = H.closed_map_clearance_build()
    lo = np.asarray(clear["lo_cells"], np.int64)
    cen = H.closed_map_free_cells()
    cells = np.floor(cen / voxel).astype(np.int64) - lo
    goal = ((cells[np.argmin(cells.sum(axis=1))] + lo).astype(np.float64) + 0.5)[None] * voxel
    H.closed_map_route_build(goal, 0.0)
    cost, approach = H.closed_map_frontier_costs()
    approach = approach[np.isfinite(approach).all(axis=1)]
    assert len(approach) >= 1
    ends = lidar_pattern(RINGS, N_AZ, np.deg2rad(-15.0), np.deg2rad(15.0), MAX_RANGE - 0.5)
    out = {"size": size, "keyframes": built["n_keyframes"], "voxels": built["n_voxels"], "voxel": voxel,
           "cells": int(np.prod(info["n_cells"])), "unknown_cells": info["unknown_cells"], "clusters_kept": info["clusters_kept"],
           "approach_points": int(len(approach)), "rays": int(len(ends)), "max_range": MAX_RANGE, "rows": []}
    for V in VIEWS:
        P = np.tile(np.eye(4), (V, 1, 1))
        P[:, :3, 3] = approach[np.arange(V) % len(approach)]
        first = None
        for name, form, per_view in FORMS:
            blocks(per_view)
            H.closed_map_view_configure(max_range=MAX_RANGE, form=form)
            rec = H.closed_map_view_gain(P, ends)
            if first is None:
                first = rec.tobytes()
            assert rec.tobytes() == first                                  # every form gives the same bytes
            ms = median_of(lambda: H.closed_map_view_gain(P, ends))
            vinfo = H.closed_map_view_info()
            assert vinfo["beyond_window"] == 0
            out["rows"].append({"views": V, "form": name, "blocks_per_view": vinfo["blocks_per_view"], "chunks": vinfo["chunks"],
                                "launches": vinfo["launches"], "window_side": vinfo["window_side"], "window_bytes": vinfo["window_bytes"],
                                "steps": vinfo["steps"], "unknown_visits": vinfo["unknown_visits"], "unknown_cells": vinfo["unknown_cells"],
                                "ms_median": ms[0], "ms_min": ms[1], "ms_max": ms[2],
                                "cells_per_s": vinfo["steps"] / (ms[0] * 1e-3) if ms[0] > 0 else None})
        blocks(None)
    # the explorer's one call, the form left to the library
    H.closed_map_view_configure(max_range=MAX_RANGE)
    out["frontier_gains_ms_median"] = median_of(lambda: H.closed_map_frontier_gains(ends))[0]
    out["frontier_gains_form"] = H.closed_map_view_info()["form"]
    gains = H.closed_map_frontier_gains(ends)[0]
    out["gains"] = [int(g) for g in gains["unknown_cells"]]
    out["clusters_cells"] = [int(c) for c in H.closed_map_frontier_clusters()[0]["cells"]]
    # beside them: a ray-cast of the same pattern from the first view's pose, and the restatement of that view on one core
    P0 = np.eye(4)
    P0[:3, 3] = approach[0]
    H.closed_map_surfels()                                                  # (the cast's plane tests read them)
    H.closed_map_raycast_configure(max_range=MAX_RANGE)
    out["raycast_ms_median"] = median_of(lambda: H.closed_map_raycast(ends, P0))[0]
    out["raycast_steps"] = H.closed_map_raycast_info()["steps"]
    if host:
        import closed_map_view_np as WN
        field = H.closed_map_frontier_field()
        Vn = WN.ViewNP(field, info["lo_cells"], (0.0, 0.0, 0.0), voxel, MAX_RANGE)
        t0 = time.perf_counter()
        want, _ = Vn.gain(P0, ends)
        out["host_view_s"] = time.perf_counter() - t0
        out["host"] = "tests/closed_map_view_np.py, one view, one core, the field already read back"
        assert want.tobytes() == H.closed_map_view_gain(P0, ends).tobytes()
    else:
        out["host"] = "not run"
    H.close()
    return out


def main():
    if "--size" in sys.argv:   # a child: one size, one JSON line
        print("RESULT " + json.dumps(one_size(sys.argv[sys.argv.index("--size") + 1], "--no-host" not in sys.argv)), flush=True)
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "closed_map_view_time.json")
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
