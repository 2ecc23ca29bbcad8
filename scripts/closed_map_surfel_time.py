"""The cost of a surfel pass over the closed map on the device: tloam_closed_map_surfels host to host
(median of five after a warm-up) at K = 32 keyframes (the out-and-back pass of tests/test_gpu_closed_map.py with its own poses)
and at K = 200 and 1000, made as scripts/closed_map_time.py makes them, at the default configurations (1 m voxels,
min_points 5).  Beside each: the same pass with plain atomics (TLOAM_SURFEL_NO_RUNS, read per pass: the two forms alternate in
one process), the closed map build of the same input, and the numpy restatement (tests/closed_map_surfel_np.py, one core), whose
sums and surfels the device's must equal bit for bit.

Every size is a child process of its own under a time limit.  A child reports its device times before it starts the restatement;
when the restatement does not end within the limit it is written down as "not measured".  A child that fails ends the run.  Run
one size under `rocprofv3 --kernel-trace --stats -- python scripts/closed_map_surfel_time.py --size K` for the kernels' own
times.  Needs an MI355X.

    python scripts/closed_map_surfel_time.py [out.json]"""
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
LIMIT_S = {32: 240, 200: 240, 1000: 420}
REPS = 5


class MapRows:
    """the device's closed map as the restatement reads one (keys, N, centroids): the build's own restatement is not timed here"""

    def __init__(self, cen, cnt, voxel):
        import voxel_map_np as VN
        self.voxel, self.origin, self.N = voxel, (0.0, 0.0, 0.0), cnt
        self.keys = VN.pack(np.floor(cen / voxel).astype(np.int64))
        self._cen = cen

    def centroids(self):
        return self._cen


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


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
    built = H.closed_map_build(0)   # warm-up
    build_ms = [timed(lambda: H.closed_map_build(0)) for _ in range(REPS)]
    info = H.closed_map_surfels()   # warm-up (and the allocation)
    os.environ["TLOAM_SURFEL_NO_RUNS"] = "1"
    H.closed_map_surfels()
    ms = {0: [], 1: []}
    for _ in range(REPS):           # the two forms in turn
        for runs in (1, 0):
            if runs:
                os.environ.pop("TLOAM_SURFEL_NO_RUNS", None)
            else:
                os.environ["TLOAM_SURFEL_NO_RUNS"] = "1"
            ms[runs].append(timed(H.closed_map_surfels))
    os.environ.pop("TLOAM_SURFEL_NO_RUNS", None)
    assert H.closed_map_surfels() == info
    out = {"keyframes": K, "voxels": built["n_voxels"], "points": info["n_points"], "orphan_points": info["orphan_points"],
           "solved_voxels": info["solved_voxels"], "launches": info["launches"],
           "ms_median": float(np.median(ms[1])), "ms_min": float(min(ms[1])), "ms_max": float(max(ms[1])),
           "plain_atomics_ms_median": float(np.median(ms[0])), "plain_atomics_ms_min": float(min(ms[0])),
           "plain_atomics_ms_max": float(max(ms[0])), "build_ms_median": float(np.median(build_ms)),
           "cpu_restatement_ms": "not measured"}
    S = H.closed_map_moments()
    nrm, ev, _ = H.closed_map_read_surfels()
    cen, cnt = H.closed_map_read()
    H.close()
    print("RESULT " + json.dumps(out), flush=True)
    if cpu:
        import closed_map_surfel_np as SN
        kf = [[[np.zeros((0, 3))] * 4, clouds[k % len(clouds)]] for k in range(K)]
        V = MapRows(cen, cnt, 1.0)
        t0 = time.perf_counter()
        Sw, nw, ew, want = SN.surfels(V, poses, kf, 0xF0)
        out["cpu_restatement_ms"] = (time.perf_counter() - t0) * 1e3
        assert S.tobytes() == Sw.tobytes() and nrm.tobytes() == nw.tobytes() and ev.tobytes() == ew.tobytes()
        assert all(info[k] == v for k, v in want.items())
        print("RESULT " + json.dumps(out), flush=True)


def last_result(text):
    rows = [ln for ln in (text or "").splitlines() if ln.startswith("RESULT ")]
    return json.loads(rows[-1][7:]) if rows else None


def main():
    if "--size" in sys.argv:   # a child: one size, a JSON line after the device part and one after the restatement
        one_size(int(sys.argv[sys.argv.index("--size") + 1]), "--cpu" in sys.argv)
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "closed_map_surfel_time.json")
    out = {"reps": REPS, "sizes": []}
    for K in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), "--size", str(K), "--cpu"]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT_S[K])
            text, rc = p.stdout, p.returncode
        except subprocess.TimeoutExpired as e:   # (the device part is over once a RESULT line is out)
            text, rc = e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout, 0
        r = last_result(text)
        if rc != 0 or r is None:   # a fault, an abort or a failed check: nothing more is started on the device
            print(f"K = {K}: exit status {rc}; stopping", flush=True)
            json.dump(out, open(path, "w"), indent=1)
            sys.exit(1)
        print(json.dumps(r), flush=True)
        out["sizes"].append(r)
        json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
