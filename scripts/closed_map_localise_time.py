"""The cost of localising a scan in the closed map on the device: tloam_closed_map_localise host to host
(median of five after a warm-up) with a full 120 k-return scan, at the default configuration, on
  static   the static pass of tests/carve_scenes.py (8 keyframes, 0.5 m voxels, mask 0x10), the scan taken midway between
           keyframes 3 and 4 and started 0.3 m / 0.02 rad off;
  32, 200  the inputs of scripts/closed_map_time.py (1 m voxels, mask 0xF0), the scan that of frame 3 started the same way.
           At K = 200 the map is the pass's clouds laid along two laps: it times the launches, it is not a scene.
Beside each: one linearise call (one sweep), the executed iteration count, and the numpy restatement
(tests/closed_map_localise_np.py, one core) with whether it ends at the same status, iteration count and pose (1e-9).

Every size is a child process of its own under a time limit.  A child reports its device times before it starts the restatement;
when the restatement does not end within the limit it is written down as "not measured".  A child that fails ends the run.  Run
one size under `rocprofv3 --kernel-trace --stats -- python scripts/closed_map_localise_time.py --size K` for the kernels' own
times.  Needs an MI355X.

    python scripts/closed_map_localise_time.py [out.json]"""
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
LIMIT_S = {"static": 240, "32": 300, "200": 360}
REPS = 5
START = (0.3, 0.02)


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def static_input(reg):
    import carve_scenes as CS
    import localise_scenes as LS
    from tloam_amd import synth_hdl64 as G
    poses, clouds = CS.static_pass()
    truth = LS.midway(poses[3], poses[4])
    scan = G.scan(G.make_street(1), truth, seed=LS.SCAN_SEED)[0]
    H = reg.HipRegistration()
    H.place_configure(enabled=1, exclude_recent=8)
    H.loop_configure(enabled=1)
    dummy = np.random.default_rng(5).uniform(-20.0, 20.0, (200, 3))
    for k in range(len(poses)):
        H.place_add_scan(dummy, np.eye(4), k)
        H.place_set_keyframe_clouds(k, *clouds[k])
    H.closed_map_configure(voxel=CS.STATIC["voxel"], cloud_mask=CS.MASK)
    H.closed_map_build(2, poses)
    return H, scan, LS.offset(truth, *START), CS.STATIC["voxel"]


def pass_input(reg, K):
    import localise_scenes as LS
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
    return H, scan, LS.offset(np.asarray(poses[3]), *START), 1.0


def one_size(size, cpu):
    from tloam_amd import registration as reg
    H, scan, prior, voxel = static_input(reg) if size == "static" else pass_input(reg, int(size))
    built, surf = H.closed_map_info(), H.closed_map_surfels()
    pose, info = H.closed_map_localise(scan, prior)   # warm-up (the allocations and the records)
    ms = [timed(lambda: H.closed_map_localise(scan, prior)) for _ in range(REPS)]
    lin = [timed(lambda: H.closed_map_linearise(scan, prior, 1.0)) for _ in range(REPS)]
    again, info2 = H.closed_map_localise(scan, prior)
    assert again.tobytes() == pose.tobytes() and info2 == {**info, "prepared": 0}
    out = {"size": size, "keyframes": built["n_keyframes"], "voxels": built["n_voxels"], "solved_voxels": surf["solved_voxels"],
           "scan_points": len(scan), "status": info["status"], "iterations": info["iterations"], "matched": info["matched"],
           "used": info["used"], "rms": info["rms"], "launches": info["launches"],
           "ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)),
           "linearise_ms_median": float(np.median(lin)), "cpu_restatement_ms": "not measured", "cpu_agrees": "not measured"}
    S = H.closed_map_moments()
    nrm, ev, _ = H.closed_map_read_surfels()
    cen, cnt = H.closed_map_read()
    H.close()
    print("RESULT " + json.dumps(out), flush=True)
    if cpu:
        import closed_map_localise_np as LN
        from closed_map_surfel_time import MapRows
        V = MapRows(cen, cnt, voxel)
        t0 = time.perf_counter()
        T = LN.Target(V, S, nrm, ev)
        wpose, winfo, _ = LN.localise(T, scan, prior)
        out["cpu_restatement_ms"] = (time.perf_counter() - t0) * 1e3
        out["cpu_agrees"] = bool((winfo["status"], winfo["iterations"], winfo["matched"], winfo["used"]) ==
                                 (info["status"], info["iterations"], info["matched"], info["used"]) and
                                 max(LN.pose_error(wpose, pose)) < 1e-9)
        print("RESULT " + json.dumps(out), flush=True)


def last_result(text):
    rows = [ln for ln in (text or "").splitlines() if ln.startswith("RESULT ")]
    return json.loads(rows[-1][7:]) if rows else None


def main():
    if "--size" in sys.argv:   # a child: one size, a JSON line after the device part and one after the restatement
        one_size(sys.argv[sys.argv.index("--size") + 1], "--cpu" in sys.argv)
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "closed_map_localise_time.json")
    out = {"reps": REPS, "start_m_rad": list(START), "sizes": []}
    for size in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), "--size", size, "--cpu"]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT_S[size])
            text, rc = p.stdout, p.returncode
        except subprocess.TimeoutExpired as e:   # (the device part is over once a RESULT line is out)
            text, rc = e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout, 0
        r = last_result(text)
        if rc != 0 or r is None:   # a fault, an abort or a failed check: nothing more is started on the device
            print(f"size {size}: exit status {rc}; stopping", flush=True)
            json.dump(out, open(path, "w"), indent=1)
            sys.exit(1)
        print(json.dumps(r), flush=True)
        out["sizes"].append(r)
        json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
