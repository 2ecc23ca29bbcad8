"""Where loop verification's defaults come from: on out-and-back passes of tloam_amd/synth_revisit.py
(streets 0-3, 16 + 16 keyframes with true poses; descriptors from the thinned scans of tests/test_gpu_place.py, keyframe clouds
from the full-density scans through the public stage calls), the overlap and rmse of
  positives: every loop record (all true revisits), verified from its Scan Context start (Rz(yaw), no translation: ~1.3 m off);
  negatives: forced pairs whose true positions are >= 15 m apart, from the same kind of start (the true relative yaw);
and, for the coarse stage, the translation / rotation error of every positive per widening of the four distance thresholds.
Needs an MI355X.

    python scripts/loop_thres.py [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from tloam_amd import registration as reg  # noqa: E402
from tloam_amd import synth_revisit as RV  # noqa: E402

THIN = dict(n_az=600, rings=np.arange(0, 64, 2))
FEATURE = dict(radius=0.5, cvr_submap=0.05)
N_OUT, EX = 16, 8
WIDEN = (1.0, 2.0, 3.0, 4.0, 6.0)
DEFAULT = 2.0   # tloam_loop_default_config's widening


def lists(H, xyz, cfg):
    S = H.segment(xyz, cfg.seg)
    ground, edge, general = xyz[S["ground"]], xyz[S["edge"]], xyz[S["general"]]
    ps, pm, ss, sm = H.extract_planar_sphere(general, cfg.feature)
    e_ds = H.voxel_down_sample(edge, cfg.edge_down_sample)
    g_ds = H.voxel_down_sample(ground, cfg.submap.ground_down_sample)
    sel = lambda idx: np.ascontiguousarray(general[idx])  # noqa: E731
    return [sel(ps), g_ds, e_ds, sel(ss)], [sel(pm), g_ds, e_ds, sel(sm)]


def err(truth, T):
    e = np.linalg.inv(truth) @ T
    return float(np.linalg.norm(e[:3, 3])), float(np.arccos(np.clip((np.trace(e[:3, :3]) - 1) / 2, -1, 1)))


def rz(yaw):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    return T


def street(seed, widen):
    cfg = reg.default_odom_config(**{f"feature__{k}": v for k, v in FEATURE.items()})
    thin, poses, leg = RV.out_and_back(N_OUT, seed=seed, **THIN)
    full, _, _ = RV.out_and_back(N_OUT, seed=seed)
    S = reg.HipRegistration()
    kf = [lists(S, xyz, cfg) for xyz in full]
    S.close()
    out = {"seed": seed, "positives": [], "negatives": [], "coarse": {}}
    base = reg.default_config()
    for w in widen:
        over = {f"coarse__{k}": getattr(base, k) * w for k in ("edge_dist_thres", "sphere_dist_thres", "planar_dist_thres",
                                                               "ground_dist_thres")}
        H = reg.HipRegistration()
        H.place_configure(enabled=1, exclude_recent=EX)
        H.loop_configure(enabled=1, **over)
        for f, (s, T) in enumerate(zip(thin, poses)):
            H.place_add_scan(s, T, f)
            H.place_set_keyframe_clouds(f, *kf[f])
        H.loop_verify_pending()
        rows = []
        for c in H.loop_constraints():
            q, m = c["query"], c["match"]
            truth = np.linalg.inv(poses[m]) @ poses[q]
            dt, da = err(truth, c["rel_pose"])
            dt0, _ = err(truth, c["init"])
            rows.append({"q": q, "m": m, "status": c["status"], "init_m": dt0, "err_m": dt, "err_rad": da,
                         "overlap": c["overlap"], "rmse": c["rmse"], "coarse_outer": c["coarse"]["outer_iterations"]})
        out["coarse"][str(w)] = rows
        if w == DEFAULT:
            out["positives"] = rows
            for q in range(len(poses)):
                if leg[q] != 1:
                    continue
                for m in range(0, q, 3):
                    if np.linalg.norm(poses[q][:3, 3] - poses[m][:3, 3]) < 15.0:
                        continue
                    c = H.loop_verify_pair(q, m, rz(RV.relative_yaw(poses[q], poses[m])))
                    out["negatives"].append({"q": q, "m": m, "status": c["status"], "overlap": c["overlap"],
                                             "rmse": c["rmse"] if np.isfinite(c["rmse"]) else None})
        H.close()
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "loop_thres.json")
    streets = [street(s, WIDEN) for s in range(4)]
    pos = [r for s in streets for r in s["positives"] if r["status"] == 0]
    neg = [r for s in streets for r in s["negatives"] if r["status"] == 0]
    failed = [(s["seed"], r["q"], r["m"], r["status"]) for s in streets for r in s["positives"] if r["status"] != 0]
    summary = {"positives": len(pos), "negatives": len(neg), "positives_not_matched": failed,
               "pos_overlap_min": min(r["overlap"] for r in pos), "pos_rmse_max": max(r["rmse"] for r in pos),
               "neg_overlap_max": max(r["overlap"] for r in neg),
               "neg_rmse_min": min((r["rmse"] for r in neg if r["rmse"] is not None), default=None),
               "init_m": [min(r["init_m"] for r in pos), max(r["init_m"] for r in pos)]}
    for w in WIDEN:
        rows = [r for s in streets for r in s["coarse"][str(w)]]
        ok = [r for r in rows if r["status"] == 0]
        summary[f"widen_{w}"] = {"max_err_m": max(r["err_m"] for r in ok), "max_err_rad": max(r["err_rad"] for r in ok),
                                 "matched": len(ok), "of": len(rows)}
    print(json.dumps(summary, indent=1))
    json.dump({"summary": summary, "streets": streets}, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
