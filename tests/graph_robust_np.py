"""numpy restatement of the robust mode of the keyframe pose-graph optimisation: graduated non-convexity
over a truncated least squares cost on the loop edges, around the solve of tests/graph_np.py (section 18), which is not changed.
Each loop edge (edges N-1 .. m-1) carries a scale s in [0, 1]; the chain is never scaled.  An outer iteration sets the scales from
the edges' statistics r_e = sum_a w0[a] e[a]^2 (base weights, a ascending) by the front end's rule (oracle_np.py :582-594), solves
from the current poses with the weights s * w0, and stops once every scale is 0 or 1."""
import numpy as np

import graph_np as GN

STOP_OFF, STOP_ALL_INLIERS, STOP_BINARY, STOP_OUTER_LIMIT = 0, 1, 2, 3
DEFAULTS = dict(noise_chi2=36.0, mu_factor=1.4, max_outer=100)


def config_ok(noise_chi2, mu_factor, max_outer):
    return bool(np.isfinite(noise_chi2) and noise_chi2 > 0.0 and np.isfinite(mu_factor) and mu_factor > 1.0 and
                int(max_outer) == max_outer and 1 <= max_outer <= 10000)


def loop_edges(n, E):
    return {k: v[n - 1:] for k, v in E.items()}


def edge_stat(P, L):
    """r_e of the loop edges L at the poses P, with L's (base) weights: the device's ((w e) e, a ascending)"""
    e = GN.residuals(P, L)
    r = np.zeros(len(e))
    for a in range(6):
        r = r + (L["w"][:, a] * e[:, a]) * e[:, a]
    return r


def scales(r, mu, c2):
    """the scale rule; a non-finite r fails both comparisons' keeps: it is rejected"""
    lo = mu / (mu + 1.0) * c2
    hi = (mu + 1.0) / mu * c2
    s = np.zeros(len(r))
    with np.errstate(invalid="ignore", divide="ignore"):
        keep = r <= lo
        mid = ~keep & (r < hi)
        s[keep] = 1.0
        s[mid] = np.minimum(np.maximum(np.sqrt(c2 * mu * (mu + 1.0) / r[mid]) - mu, 0.0), 1.0)   # (rounding at the two ends)
    return s


def solve_robust(poses, E, linear="pcg", noise_chi2=DEFAULTS["noise_chi2"], mu_factor=DEFAULTS["mu_factor"],
                 max_outer=DEFAULTS["max_outer"], **cfg):
    """-> (poses (N, 4, 4), info of the last inner solve (initial_cost the first's), robust info).  The robust info carries the
    loop edges' final scales and statistics and every inner solve's Gauss-Newton count (`gn_per_solve`)"""
    if not config_ok(noise_chi2, mu_factor, max_outer):
        raise ValueError("robust configuration out of range")
    c2 = float(noise_chi2)
    P, info = GN.solve(poses, E, linear=linear, **cfg)
    n, m = info["n_nodes"], info["n_edges"]
    L = loop_edges(n, E)
    nl = len(L["i"])
    R = dict(outer_iterations=0, stop_reason=STOP_ALL_INLIERS, gn_iterations=info["iterations"], cg_iterations=info["cg_iterations"],
             rejected=0, kept=nl, undecided=0, mu_first=0.0, mu_last=0.0, max_chi2_first=0.0, scale=np.ones(nl), chi2=np.zeros(nl),
             gn_per_solve=[info["iterations"]])
    if info["stop_reason"] == GN.STOP_NOT_RUN:
        return P, info, R
    r = edge_stat(P, L)
    R["chi2"] = r
    R["max_chi2_first"] = float(np.max(r))
    if np.max(r) <= c2:
        return P, info, R
    mu = c2 / (2.0 * float(np.max(r)) - c2)
    R["mu_first"] = mu
    first_cost = info["initial_cost"]
    R["stop_reason"] = STOP_OUTER_LIMIT
    for t in range(1, int(max_outer) + 1):
        s = scales(r, mu, c2)
        Es = dict(E)
        Es["w"] = np.concatenate([E["w"][: n - 1], s[:, None] * L["w"]])
        P, info = GN.solve(P, Es, linear=linear, **cfg)
        r = edge_stat(P, L)
        R["outer_iterations"], R["mu_last"] = t, mu
        R["gn_iterations"] += info["iterations"]
        R["cg_iterations"] += info["cg_iterations"]
        R["gn_per_solve"].append(info["iterations"])
        R["rejected"], R["kept"] = int(np.sum(s == 0.0)), int(np.sum(s == 1.0))
        R["undecided"] = nl - R["rejected"] - R["kept"]
        R["scale"], R["chi2"] = s, r
        if R["undecided"] == 0:
            R["stop_reason"] = STOP_BINARY
            break
        mu = mu * mu_factor
    info["initial_cost"] = first_cost
    return P, info, R
