"""The cost of a closed map build on the device: tloam_closed_map_build host to host (median of five after
a warm-up) at K = 32 keyframes (the out-and-back pass of tests/test_gpu_closed_map.py with its own poses) and at K = 200, 1000 and
4000 (tloam_amd/synth_graph.py's lap poses, the pass's target clouds repeated and attached through
tloam_place_set_keyframe_clouds), with the points, voxels and launches of the build, the same build without the wave's run
aggregation (TLOAM_CMAP_NO_RUNS), and the time of the numpy restatement (tests/voxel_map_np.py, one core) for the same input.

Every size is a child process of its own under a time limit, and the first one that fails ends the run.  Run one size under
`rocprofv3 --kernel-trace --stats -- python scripts/closed_map_time.py --size K` for the kernels' own times.  Needs an MI355X.

    python scripts/closed_map_time.py [out.json]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (32, 200, 1000, 4000)
LIMIT_S = {32: 240, 200: 240, 1000: 300, 4000: 420}
FEATURE = dict(radius=0.5, cvr_submap=0.05)
THIN = dict(n_az=600, rings=np.arange(0, 64, 2))
REPS = 5


def pass_clouds(reg):
    """the out-and-back pass: thinned scans, poses, and every scan's four target clouds through the public stage calls"""
    from tloam_amd import synth_revisit as RV
    thin, poses, _ = RV.out_and_back(16, seed=1, **THIN)
    full, _, _ = RV.out_and_back(16, seed=1)
    cfg = reg.default_odom_config(**{f"feature__{k}": v for k, v in FEATURE.items()})
    H = reg.HipRegistration()
    clouds = []
    for xyz in full:
        S = H.segment(xyz, cfg.seg)
        ground, edge, general = xyz[S["ground"]], xyz[S["edge"]], xyz[S["general"]]
        _, pm, _, sm = H.extract_planar_sphere(general, cfg.feature)
        clouds.append([np.ascontiguousarray(general[pm]), H.voxel_down_sample(ground, cfg.submap.ground_down_sample),
                       H.voxel_down_sample(edge, cfg.edge_down_sample), np.ascontiguousarray(general[sm])])
    H.close()
    return thin, poses, clouds


def one_size(K, cpu):
    from tloam_amd import registration as reg
    from tloam_amd import synth_graph as SG
    thin, poses, clouds = pass_clouds(reg)
    if K != len(poses):
        poses = list(SG.laps(K, seed=0)["truth"])
    H = reg.HipRegistration()
    H.place_configure(enabled=1, exclude_recent=8)
    H.loop_configure(enabled=1)
    for k in range(K):
        H.place_add_scan(thin[k % len(thin)], poses[k], k)
        H.place_set_keyframe_clouds(k, tgt=clouds[k % len(clouds)])
    info = H.closed_map_build(0)   # warm-up
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        H.closed_map_build(0)
        ms.append((time.perf_counter() - t0) * 1e3)
    out = {"keyframes": K, "points": info["n_points"], "voxels": info["n_voxels"], "launches": info["launches"],
           "runs": 0 if os.environ.get("TLOAM_CMAP_NO_RUNS") else 1, "ms_median": float(np.median(ms)), "ms_min": float(min(ms)),
           "ms_max": float(max(ms))}
    H.close()
    if cpu:
        import voxel_map_np as VN
        from oracle import binding as ob
        cats = [np.concatenate(c) for c in clouds]
        t0 = time.perf_counter()
        V = VN.VoxelMapNP()
        for k in range(K):
            V.add_frame(ob.pc_transform(poses[k], cats[k % len(cats)]))
        out["cpu_restatement_ms"] = (time.perf_counter() - t0) * 1e3
        assert len(V.keys) == info["n_voxels"] and int(V.N.sum()) == info["n_points"]
    return out


def main():
    if "--size" in sys.argv:   # a child: one size, one JSON line
        K = int(sys.argv[sys.argv.index("--size") + 1])
        print("RESULT " + json.dumps(one_size(K, "--cpu" in sys.argv)), flush=True)
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "closed_map_time.json")
    out = {"reps": REPS, "sizes": []}
    for K in SIZES:
        row = None
        for extra, env in ((["--cpu"], {}), ([], {"TLOAM_CMAP_NO_RUNS": "1"})):
            cmd = [sys.executable, os.path.abspath(__file__), "--size", str(K), *extra]
            p = subprocess.run(cmd, env={**os.environ, **env}, stdout=subprocess.PIPE, text=True, timeout=LIMIT_S[K])
            if p.returncode != 0:   # a fault, an abort or a failed check: nothing more is started on the device
                print(f"K = {K} {env}: exit status {p.returncode}; stopping", flush=True)
                json.dump(out, open(path, "w"), indent=1)
                sys.exit(1)
            r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            if row is None:
                row = r
            else:
                row["ms_median_without_runs"] = r["ms_median"]
            print(json.dumps(r), flush=True)
        out["sizes"].append(row)
        json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
