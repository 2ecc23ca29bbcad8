"""Which kernels a frame launches, per launch form (tloam_amd/csrc/tl_forms.hpp): two frames in a fresh context for every case
below, each case in a child process of its own, meant to run under the profiler's kernel trace:

    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/frame_forms_census.py
    python scripts/frame_forms_census.py --collect DIR [OUT.json]     # the per-kernel call counts of all the children, summed

TLOAM_HIP_LIB selects the library, as everywhere.  Two builds launch the same kernels iff their collected tables are equal."""
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIFT = dict(planar_maxnum=1 << 30, ground_maxnum=1 << 30, edge_maxnum=1 << 30, sphere_maxnum=1 << 30)


def cases():
    from tloam_amd import synth
    out = {}
    for name, n_src in synth.BOUNDARY_SRC.items():
        out[name] = dict(n_src=n_src, over=LIFT if name.startswith(("lifted", "n131")) else {})
    out["small"] = dict(n_src=synth.SMALL_SRC, n_tgt=synth.SMALL_TGT)
    out["kitti"] = dict(n_src=synth.KITTI_SRC, n_tgt=synth.KITTI_TGT)
    out["kitti_stepwise"] = dict(out["kitti"], how="stepwise")
    out["prebuilt_solve"] = dict(how="prebuilt")
    for knob in ("TLOAM_NO_PERSISTENT_SOLVE", "TLOAM_NO_DEVICE_LOOP"):
        out["kitti_" + knob] = dict(out["kitti"], env={knob: "1"})
    for knob in ("TLOAM_NO_DIRECT_SET", "TLOAM_FUSED_LARGE"):
        out["n131073_" + knob] = dict(out["n131073"], env={knob: "1"})
    out["kitti_loopback_mailbox"] = dict(out["kitti"], how="loopback")
    return out


def run_case(name):
    import numpy as np
    from tloam_amd import registration as reg
    from tloam_amd import synth
    case = cases()[name]
    how = case.get("how", "frame")
    H = reg.HipRegistration(reg.default_config(**case.get("over", {})))
    if how == "prebuilt":
        sets, x_true, x_eval = synth.make_prebuilt(seed=4, n_plane=30_001, n_line=7_777, n_point=1_300)
        for rt in range(3):
            H.set_correspondences(rt, *sets[rt])
        for frame in range(2):
            x, st = H.solve(x_eval)
        rc = 0
    else:
        n_src = case["n_src"]
        sc = synth.make_scene(seed=18, n_src=n_src, n_tgt=case.get("n_tgt", tuple(max(n, 1500) for n in n_src)))
        if how == "loopback":
            H.comm_init_mailbox(0, 1, [H.comm_mailbox_export()])
        H.set_frames(sc.source, sc.target)
        for frame in range(2):
            if how == "stepwise":
                rc, done = H.sm_begin(sc.T_pred), False
                while rc == 0 and not done:
                    rc, done, st = H.sm_outer()
                rc2, T, st = H.sm_end()
                rc = rc or rc2
            else:
                rc, T, st = H.scan_match(sc.T_pred)
            assert np.isfinite(T).all()
    info = H.info()
    print("CASE " + json.dumps(dict(case=name, pid=os.getpid(), rc=int(rc), gn_sweeps=int(st["gn_sweeps"]),
                                    **{k: info[k] for k in ("k3_grid", "k3_single", "one_launch_solve", "direct_set")})), flush=True)
    H.close()
    return 0 if rc == 0 else 1


def collect(directory, out=None):
    table = {}
    for path in sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)):
        for row in csv.DictReader(open(path)):
            table[row["Name"]] = table.get(row["Name"], 0) + int(row["Calls"])
    txt = json.dumps(dict(sorted(table.items())), indent=1)
    if out:
        open(out, "w").write(txt + "\n")
    print(txt)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--collect":
        return collect(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    if len(sys.argv) > 2 and sys.argv[1] == "--case":
        return run_case(sys.argv[2])
    for name, case in cases().items():   # one at a time: a child has the GPU to itself, a failure ends the census
        env = dict(os.environ, **case.get("env", {}))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], env=env, timeout=120)
        if r.returncode != 0:
            print(f"case {name} failed with exit status {r.returncode}: stopping", flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
