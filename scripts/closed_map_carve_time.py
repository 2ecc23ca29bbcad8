"""The cost of a carve of the closed map on the device: tloam_closed_map_carve host to host (median of five
after a warm-up) at K = 32 keyframes (the out-and-back pass of tests/test_gpu_closed_map.py with its own poses) and at K = 200 and
1000, made as scripts/closed_map_time.py makes them (tloam_amd/synth_graph.py's lap poses, the pass's target clouds repeated), at
the default configurations (1 m voxels, 60 m rays), with the rays, the cells visited and tested, the cells visited per second,
and for K = 32 the time of the numpy restatement (tests/closed_map_carve_np.py, one core) for the same input.

Every size is a child process of its own under a time limit, and the first one that fails ends the run.  Run one size under
`rocprofv3 --kernel-trace --stats -- python scripts/closed_map_carve_time.py --size K` for the kernels' own times.  Needs an MI355X.

    python scripts/closed_map_carve_time.py [out.json]"""
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

SIZES = (32, 200, 1000)
LIMIT_S = {32: 240, 200: 240, 1000: 300}
REPS = 5


def one_size(K, cpu):
    from closed_map_time import pass_clouds
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
    built = H.closed_map_build(0)
    info = H.closed_map_carve()   # warm-up
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        H.closed_map_carve()
        ms.append((time.perf_counter() - t0) * 1e3)
    med = float(np.median(ms))
    out = {"keyframes": K, "voxels": built["n_voxels"], "rays": info["n_rays"], "skipped_rays": info["skipped_rays"],
           "steps": info["steps"], "tested": info["tested"], "misses": info["misses"], "voxels_missed": info["voxels_missed"],
           "launches": info["launches"], "ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
           "steps_per_s": info["steps"] / (med * 1e-3)}
    if cpu:
        import closed_map_carve_np as CN
        kf = [[[np.zeros((0, 3))] * 4, clouds[k % len(clouds)]] for k in range(K)]
        V = CN.build_map(poses, kf)
        t0 = time.perf_counter()
        M, want = CN.carve(V, poses, kf, 0xF0)
        out["cpu_restatement_ms"] = (time.perf_counter() - t0) * 1e3
        assert H.closed_map_misses().tobytes() == M.tobytes() and all(info[k] == v for k, v in want.items())
    H.close()
    return out


def main():
    if "--size" in sys.argv:   # a child: one size, one JSON line
        K = int(sys.argv[sys.argv.index("--size") + 1])
        print("RESULT " + json.dumps(one_size(K, "--cpu" in sys.argv)), flush=True)
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "closed_map_carve_time.json")
    out = {"reps": REPS, "sizes": []}
    for K in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), "--size", str(K)] + (["--cpu"] if K == 32 else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT_S[K])
        if p.returncode != 0:   # a fault, an abort or a failed check: nothing more is started on the device
            print(f"K = {K}: exit status {p.returncode}; stopping", flush=True)
            json.dump(out, open(path, "w"), indent=1)
            sys.exit(1)
        r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(json.dumps(r), flush=True)
        out["sizes"].append(r)
        json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
