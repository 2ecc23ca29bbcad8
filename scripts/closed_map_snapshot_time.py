"""The cost of the closed map's snapshot on the device: tloam_closed_map_save and tloam_closed_map_load host
to host (median of five after a warm-up), without and with the keyframes' clouds, at the static pass of tests/carve_scenes.py
(8 keyframes, 0.5 m voxels) and at scripts/closed_map_time.py's K = 32 and K = 200 inputs (1 m voxels).  Beside them what a user
pays today to get the same state into a context: tloam_place_configure and tloam_loop_configure, then tloam_place_add_scan and
tloam_place_set_keyframe_clouds per keyframe, then the build, the carve and the surfel pass -- with the scans, the clouds and the
poses already in memory, which a second session would first have to produce again by replaying the run.

The expectation to confirm or refute: a load without clouds costs well under that rebuild.  Every load is checked: the loaded
context saves the blob it was loaded from.  Each size is a child process of its own under a time limit, and the first one that
fails ends the run.  Needs an MI355X.

    python scripts/closed_map_snapshot_time.py [out.json]"""
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
LIMIT_S = {"static": 240, "32": 240, "200": 300}
REPS = 5


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def inputs(size, reg):
    """-> (place scans, poses, per keyframe (src, tgt) clouds, closed map configuration, carve configuration)"""
    if size == "static":
        import carve_scenes as CS
        import relocalise_scenes as RS
        poses, clouds, scans, _ = RS.static()
        return scans, list(poses), [(c[0], c[1]) for c in clouds], dict(voxel=CS.STATIC["voxel"], cloud_mask=CS.MASK), \
            dict(max_range=CS.STATIC["max_range"])
    from closed_map_time import pass_clouds
    from tloam_amd import synth_graph as SG
    K = int(size)
    thin, poses, clouds = pass_clouds(reg)
    if K != len(poses):
        poses = list(SG.laps(K, seed=0)["truth"])
    return [thin[k % len(thin)] for k in range(K)], poses, [(None, clouds[k % len(clouds)]) for k in range(K)], {}, {}


def one_size(size):
    from tloam_amd import registration as reg
    scans, poses, clouds, cmap_cfg, carve_cfg = inputs(size, reg)
    A = reg.HipRegistration()

    def rebuild():
        A.place_configure(enabled=1, exclude_recent=8)
        A.loop_configure(enabled=1)
        for k in range(len(poses)):
            A.place_add_scan(scans[k], poses[k], k)
            A.place_set_keyframe_clouds(k, src=clouds[k][0], tgt=clouds[k][1])
        A.closed_map_build(0)
        A.closed_map_carve()
        A.closed_map_surfels()

    A.closed_map_configure(**cmap_cfg)
    A.closed_map_carve_configure(**carve_cfg)
    rebuild()   # warm-up
    rebuild_ms = [timed(rebuild) for _ in range(REPS)]
    info, sinfo = A.closed_map_info(), A.closed_map_surfel_info()
    out = {"size": size, "keyframes": info["n_keyframes"], "voxels": info["n_voxels"], "points": info["n_points"],
           "solved_voxels": sinfo["solved_voxels"], "rebuild": stats(rebuild_ms)}
    B = reg.HipRegistration()
    for clouds_too in (False, True):
        blob = A.closed_map_save(clouds=clouds_too)   # warm-up
        save_ms = [timed(lambda: A.closed_map_save(clouds=clouds_too)) for _ in range(REPS)]
        assert A.closed_map_save(clouds=clouds_too) == blob
        B.closed_map_load(blob)                       # warm-up (and the allocations of a first load)
        load_ms = [timed(lambda: B.closed_map_load(blob)) for _ in range(REPS)]
        assert B.closed_map_save(clouds=clouds_too) == blob
        probe = reg.closed_map_probe(blob)
        out["with_clouds" if clouds_too else "without_clouds"] = {"bytes": len(blob), "cloud_points": probe["cloud_points"],
                                                                  "save": stats(save_ms), "load": stats(load_ms)}
    A.close(); B.close()
    out["load_without_clouds_over_rebuild"] = out["without_clouds"]["load"]["ms_median"] / out["rebuild"]["ms_median"]
    return out


def main():
    if "--size" in sys.argv:   # a child: one size, one JSON line
        print("RESULT " + json.dumps(one_size(sys.argv[sys.argv.index("--size") + 1])), flush=True)
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "closed_map_snapshot_time.json")
    out = {"reps": REPS, "sizes": []}
    for size in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), "--size", size]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT_S[size])
            rc, text = p.returncode, p.stdout
        except subprocess.TimeoutExpired:
            rc, text = 124, ""
        rows = [ln for ln in text.splitlines() if ln.startswith("RESULT ")]
        if rc != 0 or not rows:   # a fault, an abort, a hang or a failed check: nothing more is started on the device
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
