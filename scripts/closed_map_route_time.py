"""The cost of the route through the closed map on the device: tloam_closed_map_route_build towards one
goal at a corner of the free space at radius 0 and radius = voxel, over the clearance field at R = 20 cells under both settings
of unknown_is_obstacle, with the build's rounds, tile_updates and waits; then _route_points of 100 k points and _route_paths of
1 k starts to that goal, host to host (each the median of five after a warm-up), on the inputs of
scripts/closed_map_clearance_time.py:
  static   the static pass of tests/carve_scenes.py (8 keyframes, 0.5 m voxels, mask 0x10);
  32, 200  the inputs of scripts/closed_map_time.py (1 m voxels, mask 0xF0).
Beside each build, on one core of the host: scipy.sparse.csgraph.dijkstra over the same traversable cells, the construction of
its graph timed apart from the search.  A graph of more than GRAPH_CELLS traversable cells (26 edges a cell) is not built: the
row then says so.

Every size is a child process of its own under a time limit, and the first one that fails ends the run.  Run one size under
`rocprofv3 --kernel-trace --stats -- python scripts/closed_map_route_time.py --size K --no-host` for the kernels' own times
(profiles/closed_map_route_kernel_stats.csv).  Needs an MI355X.

    python scripts/closed_map_route_time.py [out.json]"""
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
LIMIT_S = {"static": 420, "32": 420, "200": 420}
REPS = 5
R_CELLS = 20
N_POINTS, N_PATHS = 100000, 1000
GRAPH_CELLS = 1000000
UNREACHED, BLOCKED, OUTSIDE = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def median_of(call):
    call()   # warm-up
    ms = [timed(call) for _ in range(REPS)]
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def host_dijkstra(trav, goal):
    """scipy's Dijkstra over the traversable cells (nz, ny, nx) from the local cell `goal` -> (graph seconds, search seconds,
    the field as the device writes it), or None where scipy does not import"""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import dijkstra
    except ImportError:
        return None
    t0 = time.perf_counter()
    nz, ny, nx = trav.shape
    idx = np.full(trav.shape, -1, np.int64)
    idx[trav] = np.arange(int(trav.sum()))
    rows, cols, w = [], [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dz, dy, dx) == (0, 0, 0):
                    continue
                a = (slice(max(0, -dz), nz - max(0, dz)), slice(max(0, -dy), ny - max(0, dy)), slice(max(0, -dx), nx - max(0, dx)))
                b = (slice(max(0, dz), nz - max(0, -dz)), slice(max(0, dy), ny - max(0, -dy)), slice(max(0, dx), nx - max(0, -dx)))
                ok = trav[a] & trav[b]
                rows.append(idx[a][ok])
                cols.append(idx[b][ok])
                w.append(np.full(int(ok.sum()), 2 + (dz != 0) + (dy != 0) + (dx != 0), np.int32))
    m = int(trav.sum())
    graph = coo_matrix((np.concatenate(w), (np.concatenate(rows), np.concatenate(cols))), shape=(m, m)).tocsr()
    t1 = time.perf_counter()
    d = dijkstra(graph, directed=True, indices=[int(idx[goal[2], goal[1], goal[0]])], min_only=True)
    t2 = time.perf_counter()
    field = np.full(trav.shape, BLOCKED, np.uint32)
    field[trav] = np.where(np.isfinite(d), d, UNREACHED).astype(np.uint32)
    return t1 - t0, t2 - t1, field


def one_size(size, host=True):
    from closed_map_relocalise_time import pass_input, static_input
    from tloam_amd import registration as reg
    H, scan, pose = static_input(reg) if size == "static" else pass_input(reg, int(size))
    built = H.closed_map_info()
    voxel = 0.5 if size == "static" else 1.0   # (what static_input / pass_input configure)
    free = H.closed_map_free_build()
    cen = H.closed_map_free_cells()
    out = {"size": size, "keyframes": built["n_keyframes"], "voxels": built["n_voxels"], "voxel": voxel, "n_bricks": free["n_bricks"],
           "free_cells": free["free_cells"], "rounds_per_wait": reg.default_closed_map_route_config().rounds_per_wait, "builds": []}
    rng = np.random.default_rng(7)
    for wrap in (1, 0):
        H.closed_map_clearance_configure(max_distance=R_CELLS * voxel, unknown_is_obstacle=wrap)
        clear = H.closed_map_clearance_build()
        d2 = H.closed_map_clearance_field()
        lo = np.asarray(clear["lo_cells"], np.int64)
        for radius in (0.0, voxel):
            need = max(int(np.ceil((radius / voxel) ** 2)), 1)
            # the goal: the free cell nearest a corner of the box among those a body of this radius may occupy
            cells = np.floor(cen / voxel).astype(np.int64) - lo
            ok = d2[cells[:, 2], cells[:, 1], cells[:, 0]] >= need
            goal_cell = cells[ok][np.argmin(cells[ok].sum(axis=1))]
            goal = ((goal_cell + lo).astype(np.float64) + 0.5)[None] * voxel
            first = H.closed_map_route_build(goal, radius)
            field = H.closed_map_route_field()
            ms = median_of(lambda: H.closed_map_route_build(goal, radius))
            info = H.closed_map_route_info()
            same = {k: v for k, v in info.items() if k not in reg.ROUTE_DIAGNOSTICS}
            assert same == {k: v for k, v in first.items() if k not in reg.ROUTE_DIAGNOSTICS}
            assert H.closed_map_route_field().tobytes() == field.tobytes()                    # every build gives the same bytes
            row = {"unknown_is_obstacle": wrap, "radius_m": radius, "need": info["need"], "cells": int(np.prod(info["n_cells"])),
                   "bytes": info["bytes"], "traversable_cells": info["traversable_cells"], "reached_cells": info["reached_cells"],
                   "sum_cost": info["sum_cost"], "max_cost": info["max_cost"], "rounds": info["rounds"],
                   "tile_updates": info["tile_updates"], "launches": info["launches"], "waits": info["waits"],
                   "build_ms_median": ms[0], "build_ms_min": ms[1], "build_ms_max": ms[2]}
            # the queries
            box_lo = voxel * lo.astype(np.float64)
            pts = rng.uniform(box_lo, box_lo + voxel * np.asarray(info["n_cells"], np.float64), (N_POINTS, 3))
            row["points"] = N_POINTS
            row["points_ms_median"] = median_of(lambda: H.closed_map_route_points(pts))[0]
            row["points_counts"] = [int(x) for x in H.closed_map_route_points(pts)[2]]
            reached = cen[H.closed_map_route_points(cen)[0] < OUTSIDE]
            starts = reached[rng.integers(0, len(reached), N_PATHS)]
            max_cells = info["max_cost"] // 3 + 1
            row["paths"], row["paths_max_cells"] = N_PATHS, max_cells
            row["paths_ms_median"] = median_of(lambda: H.closed_map_route_paths(starts, max_cells))[0]
            status, count, _, _ = H.closed_map_route_paths(starts, max_cells)
            row["paths_reached"], row["paths_waypoints"] = int((status == 1).sum()), int(count.sum())
            if not host:
                row["host"] = "not run (--no-host)"
            elif info["traversable_cells"] > GRAPH_CELLS:
                row["host"] = f"not run: {info['traversable_cells']} traversable cells, 26 edges each, are more than the {GRAPH_CELLS} a graph is built for"
            else:
                got = host_dijkstra(field != BLOCKED, goal_cell)
                if got is None:
                    row["host"] = "not run: scipy does not import"
                else:
                    assert got[2].tobytes() == field.tobytes()                                # scipy's distances are the device's
                    row.update({"host": "scipy.sparse.csgraph.dijkstra, one core", "host_graph_s": got[0], "host_dijkstra_s": got[1]})
            out["builds"].append(row)
    H.close()
    return out


def main():
    if "--size" in sys.argv:   # a child: one size, one JSON line
        print("RESULT " + json.dumps(one_size(sys.argv[sys.argv.index("--size") + 1], "--no-host" not in sys.argv)), flush=True)
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "closed_map_route_time.json")
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
