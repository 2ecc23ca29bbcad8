"""Which kernels the search-grid build launches, per scan path of its plan (tloam_amd/csrc/tl_grid_plan.hpp), and how often the
runtime's fill kernel runs (a reservation that moved shows there): each case below in a fresh context in a child process of its
own, meant to run under the profiler's kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/grid_plan_census.py
    python scripts/grid_plan_census.py --collect DIR [OUT.json]     # the per-kernel call counts of all the children, summed

TLOAM_HIP_LIB selects the library, as everywhere.  Two builds launch the same kernels iff their collected tables are equal."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from frame_forms_census import collect  # noqa: E402

KNN_BOXES = {  # cells per axis at radius 1.0, points
    "knn_25": ((25, 25, 25), 2000), "knn_26": ((26, 26, 26), 2000),                      # each side of the SMALL / TILES edge
    "knn_126x130x128": ((126, 130, 128), 66000), "knn_150x341x41": ((150, 341, 41), 66000), "knn_128": ((128, 128, 128), 66000),
}


def cases():
    from tloam_amd import synth
    out = {name: dict(how="knn", dims=dims, n=n) for name, (dims, n) in KNN_BOXES.items()}
    out["kitti_grids_ahead"] = dict(how="frame", n_src=synth.KITTI_SRC, n_tgt=synth.KITTI_TGT)          # built at the hand-over
    out["kitti"] = dict(out["kitti_grids_ahead"], env={"TLOAM_NO_GRID_AHEAD": "1"})                    # built inside the frame
    out["m1"] = dict(how="frame", n_src=synth.M1_SRC, n_tgt=synth.M1_TGT, env={"TLOAM_NO_GRID_AHEAD": "1"})
    out["pca"] = dict(how="pca")
    return out


def run_case(name):
    import numpy as np
    from tloam_amd import registration as reg
    from tloam_amd import synth
    case = cases()[name]
    H = reg.HipRegistration(reg.default_config())
    rng = np.random.default_rng(7)
    scan_path = -1
    if case["how"] == "knn":
        lo = np.array([-60.0, -70.0, -20.0])
        extent = np.array(case["dims"], float) - 0.5
        tgt = lo + rng.uniform(0, 1, (case["n"], 3)) * extent
        tgt[0], tgt[1] = lo, lo + extent
        H.set_target(2, tgt)
        for build in range(2):
            idx, d2, cnt = H.knn(2, tgt[:250] + 0.01, 1.0, 5)
        scan_path = H.grid_info()["scan_path"]
        assert cnt.max() > 0
    elif case["how"] == "pca":
        xyz = np.array([-30.0, -30.0, -2.0]) + rng.uniform(0, 1, (20000, 3)) * np.array([60.0, 60.0, 6.0])
        for build in range(2):
            out = H.pca_info(xyz)
        assert np.isfinite(out["flatness"]).any()
    else:
        sc = synth.make_scene(seed=18, n_src=case["n_src"], n_tgt=case["n_tgt"])
        for frame in range(2):
            H.set_frames(sc.source, sc.target)
            rc, T, st = H.scan_match(sc.T_pred)
            assert rc == 0 and np.isfinite(T).all()
        scan_path = H.grid_info()["scan_path"]
    print("CASE " + json.dumps(dict(case=name, pid=os.getpid(), scan_path=int(scan_path), fallbacks=int(H.info()["fallbacks_taken"]))), flush=True)
    H.close()
    return 0


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--collect":
        return collect(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    if len(sys.argv) > 2 and sys.argv[1] == "--case":
        return run_case(sys.argv[2])
    for name, case in cases().items():   # one at a time: a child has the GPU to itself, a failure ends the census
        env = dict(os.environ, **case.get("env", {}))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], env=env, timeout=180)
        if r.returncode != 0:
            print(f"case {name} failed with exit status {r.returncode}: stopping", flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
