"""The cost of the pose graph's robust mode on the device: tloam_graph_solve_robust next to tloam_graph_solve
of the same graph, host to host, median of `--reps` calls after one warm-up of each, on tloam_amd/synth_graph.py's laps at
N = 200 with 4 false loop edges and at N = 1000 with 10 (`false_loops`), with the outer, Gauss-Newton and conjugate-gradient
iteration counts.  The kernels' own times come from a run of this script under the profiler, whose kernel statistics
`--kernel-stats` then reads into the result:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/graph_robust_time.py <scratch.json> --reps 1
    cp <dir>/.../*_kernel_stats.csv profiles/graph_robust_kernel_stats.csv
    python scripts/graph_robust_time.py [out.json] [--reps N] [--kernel-stats profiles/graph_robust_kernel_stats.csv]

Needs an MI355X."""
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tloam_amd import registration as reg  # noqa: E402
from tloam_amd import synth_graph as SG  # noqa: E402

SIZES = ((200, 4), (1000, 10))


def option(name, default=None):
    if name not in sys.argv:
        return default
    at = sys.argv.index(name)
    value = sys.argv[at + 1]
    del sys.argv[at:at + 2]
    return value


def median_ms(call, reps):
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def kernel_rows(path):
    """the graph kernels' rows of a rocprofv3 kernel statistics file"""
    rows = {}
    for row in csv.DictReader(open(path)):
        for k in ("k_graph_reweight", "k_graph_step"):
            if k + "(" in row["Name"]:
                rows[k] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                           "max_us": float(row["MaxNs"]) / 1e3, "total_ms": float(row["TotalDurationNs"]) / 1e6}
    return rows


def main():
    reps = int(option("--reps", 5))
    stats = option("--kernel-stats")
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "graph_robust_time.json")
    H = reg.HipRegistration()
    on = reg.default_graph_robust_config(enabled=1)
    out = {"reps": reps, "noise_chi2": on.noise_chi2, "mu_factor": on.mu_factor, "sizes": []}
    for n, n_bad in SIZES:
        g = SG.laps(n, seed=0)
        bad = SG.false_loops(g, n_bad, 0)
        a = (g["init"], g["i"], g["j"], g["Z"], g["w"])
        plain, pinfo = H.graph_solve(*a)                       # warm-up
        P, info, rinfo, scale, chi2 = H.graph_solve_robust(*a, rcfg=on)
        t_plain = median_ms(lambda: H.graph_solve(*a), reps)
        t_robust = median_ms(lambda: H.graph_solve_robust(*a, rcfg=on), reps)
        false_rejected = int(np.sum(scale[bad - (n - 1)] == 0.0))
        out["sizes"].append({
            "nodes": n, "loop_edges": info["n_loop_edges"], "false_edges": n_bad, "false_edges_rejected": false_rejected,
            "true_edges_rejected": rinfo["rejected"] - false_rejected,
            "plain": dict(t_plain, gn_iterations=pinfo["iterations"], cg_iterations=pinfo["cg_iterations"], stop=pinfo["stop"],
                          position_error_m=SG.position_error(plain, g["truth"])),
            "robust": dict(t_robust, outer_iterations=rinfo["outer_iterations"], gn_iterations=rinfo["gn_iterations"],
                           cg_iterations=rinfo["cg_iterations"], stop=rinfo["stop"], reweight_launches=rinfo["outer_iterations"] + 2,
                           mu=[rinfo["mu_first"], rinfo["mu_last"]], max_chi2_first=rinfo["max_chi2_first"],
                           position_error_m=SG.position_error(P, g["truth"])),
            "ms_per_gn_iteration": {"plain": t_plain["ms_median"] / max(pinfo["iterations"], 1),
                                    "robust": t_robust["ms_median"] / max(rinfo["gn_iterations"], 1)}})
    H.close()
    if stats:
        out["kernels_under_rocprofv3"] = dict(kernel_rows(stats), source=os.path.relpath(os.path.abspath(stats), ROOT))
    print(json.dumps(out, indent=1))
    json.dump(out, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
