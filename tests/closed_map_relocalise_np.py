"""Relocalisation of a scan in the closed map without a prior restated in numpy: the candidate choice, the
priors and the pick.  The description and the search are tests/place_np.py's, the localiser is tests/closed_map_localise_np.py's;
neither is restated here.

Candidates: keyframes 0 .. K-1 of the closed map's build; the min(num_candidates, K) nearest in ring key (place_np.key_distance),
ties to the lower keyframe; each with its best column shift (the first of equal minima of place_np.shift_distances) and that d.
Hypothesis h:  yaw = place_np.yaw_of(shift, S);  c = cos(yaw), s = sin(yaw);  prior = P * Rz(yaw), P the build's pose of the keyframe:
    prior[:, 0] = c * P[:, 0] + s * P[:, 1],  prior[:, 1] = c * P[:, 1] - s * P[:, 0]   (rows 0 .. 2; no contraction),
    prior[:, 2] = P[:, 2],  prior[:, 3] = P[:, 3],  the fourth row is P's
and the localiser starts from the quaternion closed_map_localise_np.pose_from_matrix takes of it.  The candidate's column
j + shift matches the query's column j: a sensor turned by +a about its z sees every azimuth lowered by a, so shift = a / (2 pi / S)
and the query's heading is the keyframe's plus yaw -- Rz composes on the right.
skipped: d is not < max_dist; never localised from, its pose is its prior.
Pick, over the hypotheses not skipped and not DEGENERATE: the largest used, then the smaller cost of the last executed sweep, then
the lower index.  FOUND when the winner has used >= min_used_ratio * finite and rms <= max_rms, finite the number of scan points
with three finite coordinates."""
from __future__ import annotations

import math

import numpy as np

import closed_map_localise_np as LN
import place_np as PN

DEFAULTS = dict(num_candidates=8, max_dist=float("inf"), min_used_ratio=0.5, max_rms=float("inf"))
FOUND, NOT_FOUND = 0, 1
DESC_KEYS = ("n_rings", "n_sectors", "max_radius", "height_offset")


def candidates(rkeys, descs, qdesc, qrkey, K, num_candidates):
    """-> [(keyframe, shift, d)] in rank order"""
    dist = [PN.key_distance(qrkey, rkeys[k]) for k in range(K)]
    order = sorted(range(K), key=lambda k: (dist[k], k))[: min(num_candidates, K)]
    out = []
    for k in order:
        d = PN.shift_distances(qdesc, descs[k])
        s = int(np.argmin(d))
        out.append((k, s, float(d[s])))
    return out


def prior_of(P, yaw):
    """P * Rz(yaw), in the kernel's arithmetic"""
    P = np.asarray(P, np.float64).reshape(4, 4)
    c, s = math.cos(yaw), math.sin(yaw)
    Q = P.copy()
    for r in range(3):
        Q[r, 0] = c * P[r, 0] + s * P[r, 1]
        Q[r, 1] = c * P[r, 1] - s * P[r, 0]
    return Q


def pick(infos, costs, skipped=None):
    """infos: dicts with status and used; costs: the cost of each hypothesis's last executed sweep -> index or -1"""
    best = -1
    for h, i in enumerate(infos):
        if (skipped is not None and skipped[h]) or i["status"] == LN.DEGENERATE:
            continue
        if best < 0 or i["used"] > infos[best]["used"] or (i["used"] == infos[best]["used"] and costs[h] < costs[best]):
            best = h
    return best


def accepted(info, finite, min_used_ratio, max_rms):
    return float(info["used"]) >= min_used_ratio * float(finite) and info["rms"] <= max_rms


def hypotheses(rkeys, descs, poses, scan, place_cfg, cfg=None):
    """the hypotheses before the localiser: dicts of keyframe, shift, dist, yaw, skipped, prior"""
    cfg = dict(DEFAULTS, **(cfg or {}))
    pc = PN.cfg_of(**place_cfg)
    qdesc, qrkey, _ = PN.describe(scan, **{k: pc[k] for k in DESC_KEYS})
    out = []
    for k, s, d in candidates(rkeys, descs, qdesc, qrkey, len(poses), cfg["num_candidates"]):
        yaw = PN.yaw_of(s, pc["n_sectors"])
        out.append(dict(keyframe=k, shift=s, dist=d, yaw=yaw, skipped=int(not d < cfg["max_dist"]), prior=prior_of(poses[k], yaw)))
    return out


def relocalise(T, rkeys, descs, poses, scan, place_cfg, cfg=None, loc_cfg=None):
    """-> (pose or None, info, hypotheses).  T: the localiser's Target; rkeys, descs: the database's; poses: the build's"""
    cfg = dict(DEFAULTS, **(cfg or {}))
    scan = np.asarray(scan, np.float64).reshape(-1, 3)
    hyps = hypotheses(rkeys, descs, poses, scan, place_cfg, cfg)
    costs = []
    for H in hyps:
        if H["skipped"]:
            H["pose"], H["localise"], H["log"] = H["prior"].copy(), dict(status=LN.DEGENERATE, iterations=0, matched=0, used=0, rms=0.0), []
            costs.append(0.0)
            continue
        H["pose"], H["localise"], H["log"] = LN.localise(T, scan, H["prior"], loc_cfg)
        costs.append(H["log"][-1]["cost"])
    infos = [H["localise"] for H in hyps]
    best = pick(infos, costs, [H["skipped"] for H in hyps])
    finite = int(np.isfinite(scan).all(axis=1).sum())
    if best >= 0 and not accepted(infos[best], finite, cfg["min_used_ratio"], cfg["max_rms"]):
        best = -1
    info = dict(status=FOUND if best >= 0 else NOT_FOUND, n_hypotheses=len(hyps), best=best, keyframe=-1, shift=0, finite=finite)
    if best >= 0:
        info.update(keyframe=hyps[best]["keyframe"], shift=hyps[best]["shift"])
    return (hyps[best]["pose"] if best >= 0 else None), info, hyps
