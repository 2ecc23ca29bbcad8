"""The cost of a ray-cast through the closed map on the device: tloam_closed_map_raycast host to host
(median of five after a warm-up) with a 64 x 1800 firing pattern out to 80 m (115 200 rays), at the default configuration, on
the three inputs of scripts/closed_map_diff_time.py:
  static   the static pass of tests/carve_scenes.py (8 keyframes, 0.5 m voxels, mask 0x10), cast from the pose midway between
           keyframes 3 and 4;
  32, 200  the inputs of scripts/closed_map_time.py (1 m voxels, mask 0xF0), cast from frame 3's pose.
Beside each, in the same process: a diff of the 120 k-return scan on the same map (host to host: the figure to hold the cast
against), and the numpy restatement (tests/closed_map_raycast_np.py, one core) with whether its statuses, ranges, ids and
counters are the device's.

Every size is a child process of its own under a time limit.  A child reports its device times before it starts the restatement;
when the restatement does not end within the limit it is written down as "not measured".  A child that fails ends the run.  Run
one size under `rocprofv3 --kernel-trace --stats -- python scripts/closed_map_raycast_time.py --size K` for k_cast_rays' own time
(profiles/closed_map_raycast_kernel_stats.csv).  Needs an MI355X.

    python scripts/closed_map_raycast_time.py [out.json]"""
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
PATTERN = dict(rings=64, n_az=1800, elev_lo=-0.43, elev_hi=0.035, length=80.0)   # an HDL-64's fan, every ray 80 m


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def one_size(size, cpu):
    import carve_scenes as CS
    from closed_map_relocalise_time import pass_input, static_input   # (they hand out the generator's pose as it is)
    from tloam_amd import raycast as RC
    from tloam_amd import registration as reg
    H, scan, pose = static_input(reg) if size == "static" else pass_input(reg, int(size))
    voxel = CS.STATIC["voxel"] if size == "static" else 1.0   # (the pass's maps are built at the default configuration)
    built, surf = H.closed_map_info(), H.closed_map_surfels()
    ends = RC.lidar_pattern(**PATTERN)
    status, ranges, ids, info = H.closed_map_raycast(ends, pose, want_ids=True)   # warm-up (the allocations and the records)
    ms = [timed(lambda: H.closed_map_raycast(ends, pose)) for _ in range(REPS)]
    ims = [timed(lambda: H.closed_map_raycast(ends, pose, want_ids=True)) for _ in range(REPS)]
    again = H.closed_map_raycast(ends, pose, want_ids=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:3], (status, ranges, ids)))
    assert again[3] == {**info, "prepared": 0, "launches": 1}
    H.closed_map_diff(scan, pose)   # warm-up
    dms = [timed(lambda: H.closed_map_diff(scan, pose)) for _ in range(REPS)]
    dinfo = H.closed_map_diff_info()
    med, dmed = float(np.median(ms)), float(np.median(dms))
    out = {"size": size, "keyframes": built["n_keyframes"], "voxels": built["n_voxels"], "solved_voxels": surf["solved_voxels"],
           "rays": len(ends), **{k: info[k] for k in ("skipped", "missed", "hits_centroid", "hits_plane", "steps", "tested")},
           "launches": again[3]["launches"], "upload_bytes": int(ends.nbytes), "download_bytes": 9 * len(ends),
           "ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)), "with_ids_ms_median": float(np.median(ims)),
           "steps_per_s_whole_call": info["steps"] / (med * 1e-3),
           "diff_points": len(scan), "diff_steps": dinfo["steps"], "diff_ms_median": dmed,
           "diff_steps_per_s_whole_call": dinfo["steps"] / (dmed * 1e-3),
           "cpu_restatement_ms": "not measured", "cpu_agrees": "not measured"}
    S = H.closed_map_moments()
    nrm, ev, _ = H.closed_map_read_surfels()
    cen, cnt = H.closed_map_read()
    H.close()
    print("RESULT " + json.dumps(out), flush=True)
    if cpu:
        import closed_map_localise_np as LN
        import closed_map_raycast_np as RN
        from closed_map_surfel_time import MapRows
        V = MapRows(cen, cnt, voxel)
        T = LN.Target(V, S, nrm, ev)
        t0 = time.perf_counter()
        want = RN.cast(T, V, ends, pose)
        out["cpu_restatement_ms"] = (time.perf_counter() - t0) * 1e3
        out["cpu_agrees"] = bool(want["status"].tobytes() == status.tobytes() and want["ranges"].tobytes() == ranges.tobytes() and
                                 want["ids"].tobytes() == ids.tobytes() and all(info[k] == v for k, v in want["info"].items()))
        print("RESULT " + json.dumps(out), flush=True)


def last_result(text):
    rows = [ln for ln in (text or "").splitlines() if ln.startswith("RESULT ")]
    return json.loads(rows[-1][7:]) if rows else None


def main():
    if "--size" in sys.argv:   # a child: one size, a JSON line after the device part and one after the restatement
        one_size(sys.argv[sys.argv.index("--size") + 1], "--cpu" in sys.argv)
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "closed_map_raycast_time.json")
    out = {"reps": REPS, "pattern": PATTERN, "sizes": []}
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
