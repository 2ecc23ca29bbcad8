"""The cost of extending the closed map in place: tloam_closed_map_extend host to host, by one keyframe
and by eight, onto maps of K = 32, 200 and 1000 keyframes with surfels and a carve (median of five after a warm-up; the keyframes
are made as scripts/closed_map_time.py makes them, the default configurations, 1 m voxels).  An extend changes the map it is
timed on, so the repetitions chain: each adds its keyframes to the map the one before left, which is K + 54 keyframes at the end
(six extends by one, then six by eight) -- the expectation under test is that an extend costs what its new points cost, not what
the map holds.  Beside it, in the same process and at the same K, what there was before for the same state:
tloam_closed_map_build + _surfels + _carve over all keyframes.

Every size is a child process of its own under a time limit; a child that fails ends the run.  After the sizes, one more child
(K = 200) runs under `rocprofv3 --kernel-trace --stats` and its kernel statistics are kept as
profiles/closed_map_extend_kernel_stats.csv (left out, and said so, where rocprofv3 is not installed).  Needs an MI355X.

    python scripts/closed_map_extend_time.py [out.json]"""
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SIZES = (32, 200, 1000)
STEPS = (1, 8)
LIMIT_S = {32: 240, 200: 240, 1000: 420}
REPS = 5
STATS_K = 200


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def one_size(K):
    from closed_map_time import pass_clouds
    from tloam_amd import registration as reg
    from tloam_amd import synth_graph as SG
    thin, poses, clouds = pass_clouds(reg)
    total = K + (REPS + 1) * sum(STEPS)
    poses = list(SG.laps(total, seed=0)["truth"])
    H = reg.HipRegistration()
    H.place_configure(enabled=1, exclude_recent=8)
    H.loop_configure(enabled=1)

    def add(k):
        H.place_add_scan(thin[k % len(thin)], poses[k], k)
        H.place_set_keyframe_clouds(k, tgt=clouds[k % len(clouds)])

    def full():
        H.closed_map_build(0)
        H.closed_map_surfels()
        H.closed_map_carve()

    for k in range(K):
        add(k)
    full()   # warm-up (and the allocations)
    full_ms = [timed(full) for _ in range(REPS)]
    built = H.closed_map_info()
    out = {"keyframes": K, "voxels": built["n_voxels"], "points": built["n_points"], "full_build_surfels_carve": stats(full_ms),
           "extend": []}
    at = K
    for step in STEPS:
        ms, infos = [], []
        for rep in range(REPS + 1):   # the first is the warm-up
            for k in range(at, at + step):
                add(k)
            at += step
            info = {}
            t = timed(lambda: info.update(H.closed_map_extend(0)))
            assert info["n_keyframes"] == step and info["first_keyframe"] == at - step
            if rep:
                ms.append(t)
                infos.append(info)
        out["extend"].append({"new_keyframes": step, **stats(ms), "points_median": float(np.median([i["points"] for i in infos])),
                              "new_voxels_median": float(np.median([i["new_voxels"] for i in infos])),
                              "touched_voxels_median": float(np.median([i["touched_voxels"] for i in infos])),
                              "rays_median": float(np.median([i["rays"] for i in infos])), "launches": infos[-1]["launches"],
                              "grown": int(sum(i["grown"] for i in infos)), "map_keyframes_after": at})
    # the state the chain left is the full build's over the same keyframes (the carve aside: it is compositional)
    rows, moments = H.closed_map_read(), H.closed_map_moments()
    H.closed_map_build(0)
    H.closed_map_surfels()
    again = H.closed_map_read()
    assert rows[0].tobytes() == again[0].tobytes() and rows[1].tobytes() == again[1].tobytes()
    assert moments.tobytes() == H.closed_map_moments().tobytes()
    H.close()
    print("RESULT " + json.dumps(out), flush=True)


def last_result(text):
    rows = [ln for ln in (text or "").splitlines() if ln.startswith("RESULT ")]
    return json.loads(rows[-1][7:]) if rows else None


def kernel_stats(path):
    """one child under rocprofv3's kernel trace -> where its statistics were kept, or why they were not"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return "not measured: rocprofv3 is not installed"
    with tempfile.TemporaryDirectory() as d:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "extend", "--", sys.executable,
               os.path.abspath(__file__), "--size", str(STATS_K)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=LIMIT_S[STATS_K])
        except subprocess.TimeoutExpired:
            return "not measured: the traced child ran into its time limit"
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not found:
            return f"not measured: exit status {p.returncode}"
        shutil.copyfile(found[0], path)
    return os.path.relpath(path, ROOT)


def main():
    if "--size" in sys.argv:   # a child: one size, one JSON line
        one_size(int(sys.argv[sys.argv.index("--size") + 1]))
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "closed_map_extend_time.json")
    out = {"reps": REPS, "sizes": []}
    for K in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), "--size", str(K)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT_S[K])
            text, rc = p.stdout, p.returncode
        except subprocess.TimeoutExpired:
            text, rc = "", 124
        r = last_result(text)
        if rc != 0 or r is None:   # a fault, an abort, a time limit or a failed check: nothing more is started on the device
            print(f"K = {K}: exit status {rc}; stopping", flush=True)
            json.dump(out, open(path, "w"), indent=1)
            sys.exit(1)
        print(json.dumps(r), flush=True)
        out["sizes"].append(r)
        json.dump(out, open(path, "w"), indent=1)
    out["kernel_stats"] = kernel_stats(os.path.join(os.path.dirname(path), "closed_map_extend_kernel_stats.csv"))
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
