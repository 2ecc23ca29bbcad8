"""The cost of the batched localiser and of the relocalisation on the device, host to host, with a full
120 k-return scan at the default configurations, on
  static   the static pass of tests/relocalise_scenes.py (8 keyframes with their real descriptors, 0.5 m voxels, mask 0x10), the
           scan taken midway between keyframes 3 and 4;
  32       the K = 32 input of scripts/closed_map_time.py (1 m voxels, mask 0xF0), the scan that of frame 3.
Per size: tloam_closed_map_relocalise (median of REPS after a warm-up), and tloam_closed_map_localise_batch at B = 1, 8 and 32
beside B single tloam_closed_map_localise calls from the same priors.  The two forms are timed in the same process, interleaved
(batch, singles, batch, singles, ...), so that a drift of the box lands on both.  The priors are offsets growing from
0.05 m / 0.002 rad; a batch is checked to return the single calls' bytes before anything is timed.

Every size is a child process of its own under a time limit; a child that fails ends the run.  Run one size under
`rocprofv3 --kernel-trace --stats -- python scripts/closed_map_relocalise_time.py --size K` for the kernels' own times.  Needs an
MI355X.

    python scripts/closed_map_relocalise_time.py [out.json]"""
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

SIZES = ("static", "32")
LIMIT_S = {"static": 240, "32": 300}
REPS = 7
BATCHES = (1, 8, 32)


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def static_input(reg):
    import carve_scenes as CS
    import localise_scenes as LS
    import relocalise_scenes as RS
    from tloam_amd import synth_hdl64 as G
    poses, clouds, scans, _ = RS.static()
    truth = LS.midway(poses[3], poses[4])
    scan = G.scan(G.make_street(1), truth, seed=LS.SCAN_SEED)[0]
    H = reg.HipRegistration()
    H.place_configure(enabled=1, **RS.PLACE)
    H.loop_configure(enabled=1)
    for k in range(len(poses)):
        H.place_add_scan(scans[k], poses[k], k)
        H.place_set_keyframe_clouds(k, *clouds[k])
    H.closed_map_configure(voxel=CS.STATIC["voxel"], cloud_mask=CS.MASK)
    H.closed_map_build(2, poses)
    return H, scan, truth


def pass_input(reg, K):
    from closed_map_time import pass_clouds
    from tloam_amd import synth_graph as SG
    from tloam_amd import synth_revisit as RV
    thin, poses, clouds = pass_clouds(reg)
    scan = RV.out_and_back(16, seed=1)[0][3]
    if K != len(poses):
        poses = list(SG.laps(K, seed=0)["truth"])
    H = reg.HipRegistration()
    H.place_configure(enabled=1, exclude_recent=8)
    H.loop_configure(enabled=1)
    for k in range(K):
        H.place_add_scan(thin[k % len(thin)], poses[k], k)
        H.place_set_keyframe_clouds(k, tgt=clouds[k % len(clouds)])
    H.closed_map_build(0)
    return H, scan, np.asarray(poses[3], np.float64)


def one_size(size):
    import closed_map_localise_np as LN
    import localise_scenes as LS
    from tloam_amd import registration as reg
    H, scan, truth = static_input(reg) if size == "static" else pass_input(reg, int(size))
    built, surf = H.closed_map_info(), H.closed_map_surfels()
    out = {"size": size, "keyframes": built["n_keyframes"], "voxels": built["n_voxels"], "solved_voxels": surf["solved_voxels"],
           "scan_points": len(scan), "batches": []}
    pose, info = H.closed_map_relocalise(scan)   # warm-up (the allocations and the records)
    ms = [timed(lambda: H.closed_map_relocalise(scan)) for _ in range(REPS)]
    hyps = H.closed_map_relocalise_hypotheses()
    out["relocalise"] = {"status": info["status"], "n_hypotheses": info["n_hypotheses"], "best": info["best"],
                         "keyframe": info["keyframe"], "shift": info["shift"], "launches": info["launches"],
                         "iterations": [h["localise"]["iterations"] for h in hyps], "used": [h["localise"]["used"] for h in hyps],
                         "error_m_rad": list(LN.pose_error(pose, truth)) if pose is not None else None,
                         "ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}
    for B in BATCHES:
        priors = np.array([LS.offset(truth, 0.05 + 0.02 * h, 0.002 + 0.001 * h) for h in range(B)])
        singles = lambda: [H.closed_map_localise(scan, p) for p in priors]   # noqa: E731
        batch = lambda: H.closed_map_localise_batch(scan, priors)            # noqa: E731
        want, got = singles(), batch()
        assert all(got[0][h].tobytes() == want[h][0].tobytes() and got[1][h] == want[h][1] for h in range(B))
        tb, ts = [], []
        for _ in range(REPS):   # interleaved
            tb.append(timed(batch))
            ts.append(timed(singles))
        out["batches"].append({"B": B, "iterations": [i["iterations"] for i in got[1]], "launches": got[1][0]["launches"],
                               "batch_ms_median": float(np.median(tb)), "batch_ms_min": float(min(tb)), "batch_ms_max": float(max(tb)),
                               "singles_ms_median": float(np.median(ts)), "singles_ms_min": float(min(ts)),
                               "singles_ms_max": float(max(ts))})
    H.close()
    print("RESULT " + json.dumps(out), flush=True)


def last_result(text):
    rows = [ln for ln in (text or "").splitlines() if ln.startswith("RESULT ")]
    return json.loads(rows[-1][7:]) if rows else None


def main():
    if "--size" in sys.argv:   # a child: one size, one JSON line
        one_size(sys.argv[sys.argv.index("--size") + 1])
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "closed_map_relocalise_time.json")
    out = {"reps": REPS, "sizes": []}
    for size in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), "--size", size]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT_S[size])
            text, rc = p.stdout, p.returncode
        except subprocess.TimeoutExpired as e:
            text, rc = e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout, 124
        r = last_result(text)
        if rc != 0 or r is None:   # a fault, an abort, a time limit or a failed check: nothing more is started on the device
            print(f"size {size}: exit status {rc}; stopping", flush=True)
            json.dump(out, open(path, "w"), indent=1)
            sys.exit(1)
        print(json.dumps(r), flush=True)
        out["sizes"].append(r)
        json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
