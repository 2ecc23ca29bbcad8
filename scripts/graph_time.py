"""The cost of the keyframe pose-graph optimisation on the device: tloam_graph_solve host to host on
tloam_amd/synth_graph.py's laps at N = 200, 1000 and 4000 (about one KITTI sequence at 1 m keyframes), after one warm-up solve
per size, with the Gauss-Newton and conjugate-gradient iteration counts and the microseconds per conjugate-gradient iteration
(the whole call over the iterations: uploads, launches and records included).  Run it under `rocprofv3 --kernel-trace --stats`
for the kernel's own time.  Needs an MI355X.

    python scripts/graph_time.py [out.json] [--reps N]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tloam_amd import registration as reg  # noqa: E402
from tloam_amd import synth_graph as SG  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    if "--reps" in sys.argv:
        args = [a for a in args if a != sys.argv[sys.argv.index("--reps") + 1]]
    path = args[0] if args else os.path.join(ROOT, "profiles", "graph_time.json")
    H = reg.HipRegistration()
    out = {"reps": reps, "sizes": []}
    for n in (200, 1000, 4000):
        g = SG.laps(n, seed=0)
        a = (g["init"], g["i"], g["j"], g["Z"], g["w"])
        P, info = H.graph_solve(*a)   # warm-up
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            H.graph_solve(*a)
            ms.append((time.perf_counter() - t0) * 1e3)
        med = float(np.median(ms))
        out["sizes"].append({"nodes": n, "loop_edges": info["n_loop_edges"], "gn_iterations": info["iterations"],
                             "cg_iterations": info["cg_iterations"], "stop": info["stop"], "ms_median": med,
                             "ms_min": float(min(ms)), "ms_max": float(max(ms)),
                             "us_per_cg_iteration": 1e3 * med / max(info["cg_iterations"], 1),
                             "position_error_m": [SG.position_error(g["init"], g["truth"]), SG.position_error(P, g["truth"])],
                             "cost": [info["initial_cost"], info["final_cost"]]})
    H.close()
    print(json.dumps(out, indent=1))
    json.dump(out, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
