"""Pose graphs with true poses, for the keyframe pose-graph optimisation of DESIGN.md section 18.

`laps(n, ...)`: n keyframes `spacing` apart along `n_laps` laps of a closed course (a circle with a gentle climb and pitch, so
that all six degrees of freedom are exercised).  Chain edge k measures rigid_inverse(T_k) * T_{k+1} with seeded noise, so the
chained initial guess drifts; every `loop_every`-th keyframe of the later laps has a loop edge to the keyframe one lap earlier,
with its own noise.  Weights are the inverse variances of that noise.  `open_chain`: the same without loop edges.
`false_loops(g, n_bad, seed)`: redirects some of a graph's loop edges to another place."""
from __future__ import annotations

import numpy as np


def _se3_exp(x):
    """(6,) (upsilon, omega) -> 4x4"""
    u, om = np.asarray(x[:3], float), np.asarray(x[3:], float)
    th = float(np.linalg.norm(om))
    Om = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    if th < 1e-8:
        a, b, c = 1.0, 0.5, 1.0 / 6.0
    else:
        a, b, c = np.sin(th) / th, (1.0 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * Om + b * (Om @ Om)
    T[:3, 3] = (np.eye(3) + b * Om + c * (Om @ Om)) @ u
    return T


def _inv(T):
    o = np.eye(4)
    o[:3, :3] = T[:3, :3].T
    o[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return o


def true_poses(n, n_laps=2, spacing=1.0, climb=0.5, pitch=0.05):
    per_lap = max(n // n_laps, 3)
    radius = per_lap * spacing / (2.0 * np.pi)
    out = []
    for k in range(n):
        a = 2.0 * np.pi * k / per_lap
        yaw, p = a + 0.5 * np.pi, pitch * np.sin(a)
        Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
        Ry = np.array([[np.cos(p), 0.0, np.sin(p)], [0.0, 1.0, 0.0], [-np.sin(p), 0.0, np.cos(p)]])
        T = np.eye(4)
        T[:3, :3] = Rz @ Ry
        T[:3, 3] = [radius * np.cos(a), radius * np.sin(a), climb * np.sin(2.0 * a)]
        out.append(T)
    return np.array(out), per_lap


def laps(n, seed=0, n_laps=2, spacing=1.0, loop_every=5, odom_sigma=(0.01, 0.001), loop_sigma=(0.02, 0.002)):
    """-> dict: truth (n, 4, 4), init (n, 4, 4) (the chained measurements from truth[0]), i, j (m,), Z (m, 4, 4), w (m, 6),
    n_loops; edges 0 .. n-2 are the chain"""
    rng = np.random.default_rng(7000 + seed)
    T, per_lap = true_poses(n, n_laps, spacing)
    so = np.array([odom_sigma[0]] * 3 + [odom_sigma[1]] * 3)
    sl = np.array([loop_sigma[0]] * 3 + [loop_sigma[1]] * 3)
    i, j, Z, w = [], [], [], []
    for k in range(n - 1):
        i.append(k); j.append(k + 1)
        Z.append(_inv(T[k]) @ T[k + 1] @ _se3_exp(rng.normal(0.0, 1.0, 6) * so))
        w.append(1.0 / (so * so))
    init = [T[0].copy()]
    for k in range(n - 1):
        init.append(init[-1] @ Z[k])
    n_loops = 0
    if loop_every > 0:
        for q in range(per_lap, n, loop_every):
            m = q - per_lap
            i.append(m); j.append(q)
            Z.append(_inv(T[m]) @ T[q] @ _se3_exp(rng.normal(0.0, 1.0, 6) * sl))
            w.append(1.0 / (sl * sl))
            n_loops += 1
    return {"truth": T, "init": np.array(init), "i": np.array(i, np.int64), "j": np.array(j, np.int64),
            "Z": np.array(Z).reshape(-1, 4, 4), "w": np.array(w).reshape(-1, 6), "n_loops": n_loops}


def open_chain(n, seed=0, **kw):
    return laps(n, seed, loop_every=0, **kw)


def false_loops(g, n_bad, seed=0, min_gap=20):
    """Makes `n_bad` randomly chosen loop edges of `g` false, in place: such an edge (i, j) keeps its ends and its weights, and
    measures rigid_inverse(truth[i]) * truth[k] for a random keyframe k at least `min_gap` keyframes from both i and j -- a place
    that looked like another.  -> their edge indices, ascending"""
    rng = np.random.default_rng(9000 + seed)
    n = len(g["truth"])
    first = n - 1
    bad = np.sort(first + rng.choice(g["n_loops"], size=n_bad, replace=False))
    g["Z"] = np.array(g["Z"], copy=True)
    for e in bad:
        i, j = int(g["i"][e]), int(g["j"][e])
        ks = np.array([k for k in range(n) if abs(k - i) >= min_gap and abs(k - j) >= min_gap])
        k = int(rng.choice(ks))
        g["Z"][e] = _inv(g["truth"][i]) @ g["truth"][k]
    return bad.astype(np.int64)


def position_error(P, truth):
    """largest |t - t_true| over the nodes"""
    P, truth = np.asarray(P).reshape(-1, 4, 4), np.asarray(truth).reshape(-1, 4, 4)
    return float(np.max(np.linalg.norm(P[:, :3, 3] - truth[:, :3, 3], axis=1)))
