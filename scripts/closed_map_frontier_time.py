"""The cost of the closed map's frontiers on the device: tloam_closed_map_frontier_build over the free-space
grid with the carve gate off and on, with the build's rounds, launches and waits and the clusters it finds; then the cost join
with a route built from one goal (the free cell nearest a corner of the box, unknown an obstacle, radius 0), and
_frontier_points of 100 k points, host to host (each the median of five after a warm-up), on the inputs of
scripts/closed_map_route_time.py:
  static   the static pass of tests/carve_scenes.py (8 keyframes, 0.5 m voxels, mask 0x10);
  32, 200  the inputs of scripts/closed_map_time.py (1 m voxels, mask 0xF0).
Beside each build, on one core of the host: scipy.ndimage.label with the full 3 x 3 x 3 structure over the same mask of frontier
cells; the script asserts that the two partitions are equal and that every label is its component's least index.  There is no
gate.

Every size is a child process of its own under a time limit, and the first one that fails ends the run.  Needs an MI355X.

    python scripts/closed_map_frontier_time.py [out.json]"""
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
N_POINTS = 100000
OUTSIDE = 0xFFFFFFFC


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def median_of(call):
    call()   # warm-up
    ms = [timed(call) for _ in range(REPS)]
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def host_label(field):
    """scipy's labelling of the device's own mask of frontier cells on one core -> (seconds, components), the partition and the
    least-index rule asserted; None where scipy does not import"""
    try:
        import scipy.ndimage as ndi
    except ImportError:
        return None
    front = field < OUTSIDE
    t0 = time.perf_counter()
    lab, n = ndi.label(front, structure=np.ones((3, 3, 3), int))
    t1 = time.perf_counter()
    if n:
        index = np.arange(field.size, dtype=np.int64).reshape(field.shape)
        least = np.asarray(ndi.minimum(index, lab, np.arange(1, n + 1))).astype(np.int64)
        assert np.array_equal(field[front].astype(np.int64), least[lab[front] - 1])    # the same partition, the least index
    return t1 - t0, int(n)


def one_size(size, host=True):
    from closed_map_relocalise_time import pass_input, static_input
    from tloam_amd import registration as reg
    H, scan, pose = static_input(reg) if size == "static" else pass_input(reg, int(size))
    built = H.closed_map_info()
    voxel = 0.5 if size == "static" else 1.0   # (what static_input / pass_input configure)
    H.closed_map_carve()
    out = {"size": size, "keyframes": built["n_keyframes"], "voxels": built["n_voxels"], "voxel": voxel,
           "rounds_per_wait": reg.default_closed_map_frontier_config().rounds_per_wait, "builds": []}
    rng = np.random.default_rng(7)
    for gate in (0, 1):
        H.closed_map_free_configure(carve_gate=gate)
        free = H.closed_map_free_build()
        first = H.closed_map_frontier_build()
        field = H.closed_map_frontier_field()
        clusters = H.closed_map_frontier_clusters()[0].tobytes()
        ms = median_of(H.closed_map_frontier_build)
        info = H.closed_map_frontier_info()
        same = {k: v for k, v in info.items() if k not in reg.FRONTIER_DIAGNOSTICS}
        assert same == {k: v for k, v in first.items() if k not in reg.FRONTIER_DIAGNOSTICS}
        assert H.closed_map_frontier_field().tobytes() == field.tobytes()                   # every build gives the same bytes
        assert H.closed_map_frontier_clusters()[0].tobytes() == clusters
        row = {"carve_gate": gate, "n_bricks": free["n_bricks"], "cells": int(np.prod(info["n_cells"])), "bytes": info["bytes"],
               **{k: info[k] for k in ("free_cells", "unknown_cells", "occupied_cells", "frontier_cells", "clusters", "clusters_kept",
                                       "cells_kept", "largest", "unknown_faces", "rounds", "tile_updates", "launches", "waits")},
               "build_ms_median": ms[0], "build_ms_min": ms[1], "build_ms_max": ms[2]}
        # the join with a route from one goal: the free cell nearest a corner of the box
        H.closed_map_clearance_configure(max_distance=R_CELLS * voxel, unknown_is_obstacle=1)
        clear = H.closed_map_clearance_build()
        lo = np.asarray(clear["lo_cells"], np.int64)
        cen = H.closed_map_free_cells()
        cells = np.floor(cen / voxel).astype(np.int64) - lo
        goal = ((cells[np.argmin(cells.sum(axis=1))] + lo).astype(np.float64) + 0.5)[None] * voxel
        route = H.closed_map_route_build(goal, 0.0)
        row["route_rounds"], row["route_max_cost"] = route["rounds"], route["max_cost"]
        row["costs_ms_median"] = median_of(H.closed_map_frontier_costs)[0]
        cost = H.closed_map_frontier_costs()[0]
        row["clusters_reached"] = int((cost < 0xFFFFFFFD).sum())
        # the query
        box_lo = voxel * lo.astype(np.float64)
        pts = rng.uniform(box_lo, box_lo + voxel * np.asarray(info["n_cells"], np.float64), (N_POINTS, 3))
        row["points"] = N_POINTS
        row["points_ms_median"] = median_of(lambda: H.closed_map_frontier_points(pts))[0]
        row["points_counts"] = [int(x) for x in H.closed_map_frontier_points(pts)[2]]
        got = host_label(field) if host else None
        if got is None:
            row["host"] = "not run"
        else:
            assert got[1] == info["clusters"]
            row.update({"host": "scipy.ndimage.label, 3 x 3 x 3 structure, one core", "host_label_s": got[0]})
        out["builds"].append(row)
    H.close()
    return out


def main():
    if "--size" in sys.argv:   # a child: one size, one JSON line
        print("RESULT " + json.dumps(one_size(sys.argv[sys.argv.index("--size") + 1], "--no-host" not in sys.argv)), flush=True)
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "closed_map_frontier_time.json")
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
