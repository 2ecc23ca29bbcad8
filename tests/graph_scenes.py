"""Named hand-made pose graphs for the keyframe pose-graph optimisation (DESIGN.md sections 18 and 20): one per branch of
tl_graph.hip / tl_api_graph.hip that tloam_amd/synth_graph.py's laps never reach -- every split of the nodes over the 512
threads (N = 2, 3, a wave boundary, the switch of the chunk at 513 / 514, a partial last chunk at 1026), nodes with 150 and more
edge ends, loop edges that point backwards, touch the fixed node 0, are doubled or run beside a chain edge, far more edges than
nodes, a chain whose residuals are not 0 at the start, weights over eight decades, a loop edge of weight 0, every branch of
pose_from_matrix and exact half turns, a run that ends on the cost by a margin, poses 2e5 m from the origin, and robust runs over
741 loop edges and over one.  tests/test_graph_scenes.py checks every case on the CPU; tests/test_gpu_graph_edges.py runs every
case on the device against the restatement (tests/graph_np.py, tests/graph_robust_np.py).

A cost comparison near the iteration's fixed point would stop two correct implementations a step apart (section 18), so every
case comes with margin conditions (`margins`), checked on the restatement alone before the device is asked anything:
  (a) the direct and the PCG solve agree in `iterations`, `stop_reason` and `reverted`;
  (b) their poses agree within POSE_GAP (1e-10, a tenth of the device's bar; `far`: its measured bar, see `far_bar`);
  (c) no iteration's max |d| lies in [step_tol / 3, 3 step_tol];
  (d) where the cost comparison decides (max |d| >= step_tol), |new - cur| >= COST_GAP * cur (1e-8, ten times the 1e-9 to which
      the parity tests hold device and restatement costs together);
  (e) robust cases: the direct and PCG robust runs agree in `outer_iterations`, `stop_reason`, the kind of every scale and
      `gn_per_solve`; in every outer iteration no r lies within STAT_GAP (1e-5 relative, ten times the 1e-6 bar on chi2) of `lo`
      or `hi`, and no max r within STAT_GAP of `noise_chi2`.
A case that misses a condition is repaired here, by its seed or its own step_tol, never by a wider condition.

A case is Case(name, graph, cfg, robust): `graph` the dict of synth_graph.laps (truth, init, i, j, Z, w, n_loops) plus what the
case's tests need (`bad`: the false loop edges; `G`, `unshifted`: far's shift and the graph before it), `cfg` the overrides of
graph_np.DEFAULTS, `robust` whether the case is for section 20's mode."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import graph_np as GN
import graph_robust_np as GR

ODOM_SIGMA, LOOP_SIGMA = (0.01, 0.001), (0.02, 0.002)
POSE_GAP, COST_GAP, STAT_GAP = 1e-10, 1e-8, 1e-5
THREADS = 512   # k_graph_step's workgroup: a thread owns ceil((N - 1) / 512) consecutive nodes


class Case(NamedTuple):
    name: str
    graph: dict
    cfg: dict
    robust: bool


# ---- rigid helpers ---------------------------------------------------------------------------------------------------------
def exp1(x):
    return GN.se3_exp(np.asarray(x, float))[0]


def tidy(T):
    """one Newton step towards the nearest rotation, so that long products stay rigid to rounding; exact on an exact rotation"""
    T = np.array(T, float)
    R = T[..., :3, :3]
    T[..., :3, :3] = 0.5 * (R @ (3.0 * np.eye(3) - np.swapaxes(R, -1, -2) @ R))
    return T


def rigid_error(T):
    """largest of |R^T R - I|, |det R - 1| and the last row's distance from (0, 0, 0, 1)"""
    T = np.asarray(T, float).reshape(-1, 4, 4)
    R = T[:, :3, :3]
    return float(max(np.max(np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3))), np.max(np.abs(np.linalg.det(R) - 1.0)),
                     np.max(np.abs(T[:, 3] - np.array([0.0, 0.0, 0.0, 1.0])))))


def rot_z(a):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    return T


def quat_branch(R):
    """which branch pose_from_matrix (tl_se3.hpp) takes on a rotation: 0 `tr > 0`, 1 / 2 / 3 x / y / z dominant"""
    R = np.asarray(R, float)
    if R[0, 0] + R[1, 1] + R[2, 2] > 0.0:
        return 0
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    return 1 + i


def edges_of(g):
    return GN.as_edges(g["i"], g["j"], g["Z"], g["w"])


def args_of(g):
    return g["init"], g["i"], g["j"], g["Z"], g["w"]


def chunk_of(n):
    return -(-(n - 1) // THREADS)


def degree(g, k):
    return int(np.sum(g["i"] == k) + np.sum(g["j"] == k))


# ---- generators ------------------------------------------------------------------------------------------------------------
def _rng(seed, stream):
    return np.random.default_rng([18000, int(seed), stream])   # (a stream per ingredient: one's length moves no other)


def _weights(sigma, count):
    s = np.array([sigma[0]] * 3 + [sigma[1]] * 3)
    return np.tile(1.0 / (s * s), (count, 1))


def from_truth(T, loops, seed, loop_w=None, perturb=0.0):
    """The graph over the true poses T: chain measurements with noise 0.01 m / 0.001 rad, the loop edges `loops` ((i, j), either
    direction) with noise 0.02 m / 0.002 rad, weights the inverse variances unless loop_w(rng, count) -> (count, 6) gives the
    loops'; the initial guess is the chained measurements, each node but the first right-perturbed by exp(N(0, perturb))"""
    T = np.asarray(T, float)
    n, nl = len(T), len(loops)
    so, sl = np.array([ODOM_SIGMA[0]] * 3 + [ODOM_SIGMA[1]] * 3), np.array([LOOP_SIGMA[0]] * 3 + [LOOP_SIGMA[1]] * 3)
    cn = GN.se3_exp(_rng(seed, 2).normal(0.0, 1.0, (max(n - 1, 1), 6)) * so)
    ln = GN.se3_exp(_rng(seed, 3).normal(0.0, 1.0, (max(nl, 1), 6)) * sl)
    i, j = list(range(n - 1)), list(range(1, n))
    Z = [tidy(GN.inv(T[k]) @ T[k + 1] @ cn[k]) for k in range(n - 1)]
    init = [T[0].copy()]
    for k in range(n - 1):
        init.append(tidy(init[-1] @ Z[k]))
    for q, (a, b) in enumerate(loops):
        i.append(int(a)); j.append(int(b))
        Z.append(tidy(GN.inv(T[a]) @ T[b] @ ln[q]))
    w = np.concatenate([_weights(ODOM_SIGMA, n - 1), _weights(LOOP_SIGMA, nl) if loop_w is None else
                        np.asarray(loop_w(_rng(seed, 4), nl), float).reshape(nl, 6)])
    init = np.array(init)
    if perturb > 0.0:
        init[1:] = tidy(init[1:] @ GN.se3_exp(_rng(seed, 5).normal(0.0, perturb, (n - 1, 6))))
    return {"truth": T, "init": init, "i": np.array(i, np.int64), "j": np.array(j, np.int64),
            "Z": np.array(Z).reshape(-1, 4, 4), "w": w.reshape(-1, 6), "n_loops": nl}


def walk(n, loops, seed, loop_w=None, perturb=0.0):
    """A chain of n true poses: the first a random orientation (rotation vector N(0, 1.2) per axis) within +-50 m, each step
    exp((U(-1, 1)^3, N(0, 0.3)^3)), so that all three axes turn and every branch of pose_from_matrix occurs; then `from_truth`.
    Returns the dict of synth_graph.laps"""
    r = _rng(seed, 0)
    first = exp1(np.concatenate([np.zeros(3), r.normal(0.0, 1.2, 3)]))
    first[:3, 3] = r.uniform(-50.0, 50.0, 3)
    r = _rng(seed, 1)
    steps = GN.se3_exp(np.concatenate([r.uniform(-1.0, 1.0, (max(n - 1, 1), 3)), r.normal(0.0, 0.3, (max(n - 1, 1), 3))], axis=1))
    T = [first]
    for k in range(n - 1):
        T.append(tidy(T[-1] @ steps[k]))
    return from_truth(np.array(T), loops, seed, loop_w=loop_w, perturb=perturb)


def pairs(n, gap=2):
    return [(a, b) for a in range(n) for b in range(a + gap, n)]


# ---- the named cases: each -> (graph, cfg overrides) -----------------------------------------------------------------------------
TINY = {"n2_forward": (2, [(0, 1)]), "n2_backward": (2, [(1, 0)]), "n3": (3, [(0, 2), (2, 0), (1, 2)])}
SIZES = (65, 66, 513, 514, 1026)


def tiny(which, seed=0):
    n, loops = TINY[which]
    return walk(n, loops, seed), {}


# a case's own step_tol: the default 1e-7 leaves these graphs an iteration whose step (1e-7 .. 1e-5) changes the cost by 1e-9
# relative and less, either way -- condition (d) -- or a step within a factor 3 of it -- (c).  The value sits where the
# restatement's steps leave the widest gap: the step before it is above 3 step_tol and still changes the cost by 1e-5 relative
# and more, the step that ends the run is below step_tol / 3
SIZES_STEP_TOL = {65: 1e-5, 66: 1e-5, 513: 1e-4, 514: 1e-4, 1026: 1e-6}


def sizes(n, seed=0):
    return walk(n, [(k, k + n // 2) for k in range(0, n - n // 2, 9)], seed), {"step_tol": SIZES_STEP_TOL[n]}


def hub(seed=0):
    """node 7 joined to nodes 20 .. 169, alternating direction.  At the default step_tol the run ends on a cost rise of 6e-11
    relative at a step of 2.5e-7: reproducible, and not a fair thing to hold a device to; step_tol 1e-6 ends it on the step"""
    return walk(200, [(7, k) if k % 2 == 0 else (k, 7) for k in range(20, 170)], seed), {"step_tol": 1e-6}


def hub0(seed=0):
    """the same onto the fixed node 0, nodes 10 .. 159"""
    return walk(200, [(0, k) if k % 2 == 0 else (k, 0) for k in range(10, 160)], seed), {"step_tol": 3e-6}


def dense(seed=0):
    return walk(30, pairs(30), seed), {"step_tol": 1e-6}


DOUBLED_LOOPS = [(k, k + 60) for k in range(2, 60, 5)]   # 12
DOUBLED_BESIDE = 40


def doubled(seed=0, merged=False):
    """each of 12 loop edges twice, one after the other, then (k, k + 1) and (k + 1, k) beside chain edge k.  merged: every
    pair as one edge of twice the weight -- the same cost, so by the contract the same poses"""
    g = walk(120, DOUBLED_LOOPS + [(DOUBLED_BESIDE, DOUBLED_BESIDE + 1), (DOUBLED_BESIDE + 1, DOUBLED_BESIDE)], seed)
    n, nd = 120, len(DOUBLED_LOOPS)
    first = n - 1
    keep = list(range(first)) + [first + q for q in range(nd) for _ in range(1 if merged else 2)] + [first + nd, first + nd + 1]
    for k in ("i", "j", "Z", "w"):
        g[k] = np.array(g[k][keep], copy=True)
    if merged:
        g["w"][first:first + nd] *= 2.0
    g["n_loops"] = len(keep) - first
    return g, {"step_tol": 1e-5}


def backwards(seed=0):
    return walk(300, [(k + 100, k) for k in range(0, 197, 7)], seed), {"step_tol": 3e-5}


def perturbed(seed=0):
    """the chain's right-hand side is not 0 at the first iteration"""
    return walk(300, [(k, k + 100) for k in range(0, 197, 7)], seed, perturb=0.02), {"step_tol": 1e-6}


def aniso(seed=0):
    return walk(300, [(k, k + 100) for k in range(0, 197, 7)], seed, loop_w=lambda r, nl: 10.0 ** r.uniform(-2.0, 6.0, (nl, 6))), {"step_tol": 1e-6}


HALF_TURNS = (np.diag([1.0, -1.0, -1.0, 1.0]), np.diag([-1.0, 1.0, -1.0, 1.0]), np.diag([-1.0, -1.0, 1.0, 1.0]))


def zero_loop(seed=0):
    """One loop edge whose six weights are 0, on a chain that is exact: orientations I and the three half turns about the axes,
    positions and measurements in eighths, no noise.  Every chain residual is then exactly 0 in the restatement's matrices and
    in the device's quaternions, so the right-hand side is exactly 0: rz0 == 0, no PCG iteration, a step of exactly 0.  (With
    a noisy chain the chained guess leaves residuals of 1e-16, and none of that is exact.)  The loop edge disagrees with the
    chain by metres: a solver that read its measurement in spite of its weight would move"""
    n = 60
    r = _rng(seed, 0)
    turn = (np.eye(4),) + HALF_TURNS
    T = [np.eye(4)]
    for k in range(n - 1):
        S = turn[int(r.integers(0, 4))].copy()
        S[:3, 3] = r.integers(-8, 9, 3) / 8.0
        T.append(T[-1] @ S)
    T = np.array(T)
    i, j = list(range(n - 1)) + [10], list(range(1, n)) + [50]
    Z = [GN.inv(T[k]) @ T[k + 1] for k in range(n - 1)] + [tidy(GN.inv(T[10]) @ T[50] @ exp1([2.0, -1.0, 0.5, 0.3, -0.2, 0.4]))]
    w = np.concatenate([_weights(ODOM_SIGMA, n - 1), np.zeros((1, 6))])
    return {"truth": T, "init": T.copy(), "i": np.array(i, np.int64), "j": np.array(j, np.int64), "Z": np.array(Z),
            "w": w, "n_loops": 1}, {}


def half_turns(seed=0):
    """true orientations cycle through the three half turns about the axes, exactly at every fifth node (qw == 0, trace -1)
    and times a small rotation (N(0, 0.05) per axis) elsewhere; neighbours are half a turn apart, about every axis"""
    n = 90
    r = _rng(seed, 0)
    small = GN.se3_exp(np.concatenate([np.zeros((n, 3)), r.normal(0.0, 0.05, (n, 3))], axis=1))
    pos = np.cumsum(r.uniform(-1.0, 1.0, (n, 3)), axis=0)
    T = []
    for k in range(n):
        P = HALF_TURNS[k % 3] @ (np.eye(4) if k % 5 == 0 else small[k])
        P[:3, 3] = pos[k]
        T.append(P)
    loops = [(k, k + 45) if (k // 5) % 2 == 0 else (k + 45, k) for k in range(0, 40, 5)]   # 8
    return from_truth(np.array(T), loops, seed), {"step_tol": 1e-5}


def reverts(seed=0):
    """the last loop's measurement is wrong by a 2.5 rad turn about z: the run ends on the cost, by a margin"""
    g = walk(100, [(k, k + 50) for k in range(0, 50, 5)], seed)
    g["Z"][-1] = tidy(g["Z"][-1] @ rot_z(2.5))
    return g, {}


FAR_SHIFT = (1e5, -2e5, 3e3, 0.3, -0.2, 2.0)


def far(seed=0):
    """`perturbed` without the perturbation, every pose left-multiplied by G = exp(FAR_SHIFT): the measurements are relative
    and do not change, the coordinates are 2e5 m"""
    g = walk(300, [(k, k + 100) for k in range(0, 197, 7)], seed)
    G = exp1(FAR_SHIFT)
    shifted = dict(g, truth=tidy(G @ g["truth"]), init=tidy(G @ g["init"]), G=G, unshifted=g)
    return shifted, {"step_tol": 3e-5}


def falsify(g, bad, seed):
    """makes the loop edges `bad` (indices among the loops) false in place: Z right-multiplied by exp((U(-3, 3)^3, N(0, 0.3)^3))"""
    r = _rng(seed, 6)
    x = np.concatenate([r.uniform(-3.0, 3.0, (len(bad), 3)), r.normal(0.0, 0.3, (len(bad), 3))], axis=1)
    first = len(g["init"]) - 1
    for q, b in enumerate(bad):
        g["Z"][first + b] = tidy(g["Z"][first + b] @ exp1(x[q]))
    g["bad"] = np.sort(np.asarray(bad, np.int64))
    return g


def robust_dense(seed=0):
    """all 741 pairs b >= a + 2 of 40 nodes, 60 of them false: two turns of k_graph_reweight's stride"""
    g = walk(40, pairs(40), seed)
    return falsify(g, _rng(seed, 7).choice(g["n_loops"], size=60, replace=False), seed), {}


def robust_one(seed=0):
    """a single loop edge, false"""
    return falsify(walk(80, [(5, 60)], seed), [0], seed), {}


PLAIN = {**{f"tiny-{k}": functools.partial(tiny, k) for k in TINY}, **{f"sizes-{n}": functools.partial(sizes, n) for n in SIZES},
         "hub": hub, "hub0": hub0, "dense": dense, "doubled": doubled, "doubled-merged": functools.partial(doubled, merged=True),
         "backwards": backwards, "perturbed": perturbed, "aniso": aniso, "zero_loop": zero_loop, "half_turns": half_turns,
         "reverts": reverts, "far": far}
ROBUST = {"robust_dense": robust_dense, "robust_one": robust_one}
# a case's seed: 0 unless a margin condition asked for another (the reason beside it)
SEEDS: dict = {}


@functools.lru_cache(maxsize=None)
def case(name):
    make = PLAIN[name] if name in PLAIN else ROBUST[name]
    g, cfg = make(seed=SEEDS.get(name, 0))
    for v in g.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)   # (shared among the tests: nobody changes it)
    return Case(name, g, cfg, name in ROBUST)


# ---- the contract's Gauss-Newton, replayed ----------------------------------------------------------------------------------
def trace(init, E, linear="pcg", **cfg):
    """graph_np.solve's loop with graph_np's own functions -> per iteration (max |d|, cost before, cost after the step)"""
    c = dict(GN.DEFAULTS)
    c.update(cfg)
    P = np.array(init, float).reshape(-1, 4, 4)
    n, m = len(P), len(E["i"])
    out = []
    if n < 2 or m <= n - 1:
        return out
    cur = GN.cost(P, E)
    for _ in range(c["max_iterations"]):
        e, A = GN.linearise(P, E)
        b = GN.rhs(n, E, e, A)
        d = GN.direct_solve(n, E, A, b) if linear == "direct" else \
            GN.pcg(n, E, A, b, GN.chain_preconditioner(P, E), c["cg_tol"], c["max_cg_iterations"])[0]
        Pn = P @ GN.se3_exp(d)
        Pn[0] = P[0]
        new = GN.cost(Pn, E)
        step = float(np.max(np.abs(d)))
        out.append((step, cur, new))
        small = step < c["step_tol"]
        if not np.isfinite(new) or (new > cur and not small) or small:
            break
        P, cur = Pn, new
    return out


def trace_margins(tr, step_tol):
    """conditions (c) and (d) on one trace -> the failures, as text"""
    bad = []
    for it, (step, cur, new) in enumerate(tr):
        if step_tol / 3.0 <= step <= 3.0 * step_tol:
            bad.append(f"(c) iteration {it}: max |d| {step:.3e} within a factor 3 of step_tol {step_tol:.1e}")
        if step >= step_tol and not abs(new - cur) >= COST_GAP * cur:
            bad.append(f"(d) iteration {it}: cost {cur:.12g} -> {new:.12g}, {abs(new - cur) / cur:.1e} relative, at max |d| {step:.3e}")
    return bad


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement on a plain case, computed once: per linear solve (poses, info, trace); node arrays read-only"""
    c = case(name)
    E = edges_of(c.graph)
    out = {}
    for lin in ("direct", "pcg"):
        P, info = GN.solve(c.graph["init"], E, linear=lin, **c.cfg)
        P.setflags(write=False)
        out[lin] = (P, info, trace(c.graph["init"], E, lin, **c.cfg))
    return out


@functools.lru_cache(maxsize=None)
def far_bar():
    """`far`'s pose bar, measured on the restatement: ten times the larger of what the shift itself moves the direct solve by
    (G P(unshifted) against P(shifted)) and what PCG and direct differ by on the shifted graph.  One rounding of a coordinate
    of 2e5 m is 3e-11, so 1e-9 would not be a fair bar; the ten is for the device's other operation order (quaternions, gathers
    in edge order).  -> (bar, the two terms)"""
    c = case("far")
    u = c.graph["unshifted"]
    ref = reference("far")
    Pu = GN.solve(u["init"], edges_of(u), linear="direct", **c.cfg)[0]
    shift = float(np.max(np.abs(c.graph["G"] @ Pu - ref["direct"][0])))
    lin = float(np.max(np.abs(ref["pcg"][0] - ref["direct"][0])))
    return 10.0 * max(shift, lin), shift, lin


def two_node_step(g):
    """N = 2 with both edges (0, 1) in closed form: node 1 is every edge's j, J_j = I, so one Gauss-Newton step solves the 6x6
    system (sum W_k) d = -sum W_k e_k -> the poses after it"""
    assert len(g["init"]) == 2 and np.all(g["i"] == 0) and np.all(g["j"] == 1)
    e, _ = GN.linearise(g["init"], edges_of(g))
    H = np.sum([np.diag(w) for w in g["w"]], axis=0)
    d = np.linalg.solve(H, -np.sum(g["w"] * e, axis=0))
    P = np.array(g["init"], copy=True)
    P[1] = P[1] @ exp1(d)
    return P


def kind(s):
    """a scale's decision: 0 rejected, 1 kept, 2 in between"""
    s = np.asarray(s)
    return np.where(s == 0.0, 0, np.where(s == 1.0, 1, 2))


def trace_robust(init, E, linear="pcg", noise_chi2=GR.DEFAULTS["noise_chi2"], mu_factor=GR.DEFAULTS["mu_factor"],
                 max_outer=GR.DEFAULTS["max_outer"], **cfg):
    """graph_robust_np.solve_robust's loop with its own functions -> (max r after the plain solve, per outer iteration
    (mu, lo, hi, the r the scales are set from, the scales))"""
    c2 = float(noise_chi2)
    P, info = GN.solve(init, E, linear=linear, **cfg)
    L = GR.loop_edges(info["n_nodes"], E)
    n = info["n_nodes"]
    if info["stop_reason"] == GN.STOP_NOT_RUN:
        return 0.0, []
    r = GR.edge_stat(P, L)
    first = float(np.max(r))
    out = []
    if first <= c2:
        return first, out
    mu = c2 / (2.0 * first - c2)
    for _ in range(int(max_outer)):
        s = GR.scales(r, mu, c2)
        out.append((mu, mu / (mu + 1.0) * c2, (mu + 1.0) / mu * c2, r, s))
        Es = dict(E)
        Es["w"] = np.concatenate([E["w"][: n - 1], s[:, None] * L["w"]])
        P, info = GN.solve(P, Es, linear=linear, **cfg)
        r = GR.edge_stat(P, L)
        if np.all((s == 0.0) | (s == 1.0)):
            break
        mu = mu * mu_factor
    return first, out


@functools.lru_cache(maxsize=None)
def reference_robust(name, max_outer=GR.DEFAULTS["max_outer"]):
    """the robust restatement on a robust case, computed once: per linear solve (poses, info, robust info)"""
    c = case(name)
    E = edges_of(c.graph)
    return {lin: GR.solve_robust(c.graph["init"], E, linear=lin, max_outer=max_outer, **c.cfg) for lin in ("direct", "pcg")}


class Margins(NamedTuple):
    failures: tuple   # text, one per missed condition
    figures: dict     # what was measured on the way


@functools.lru_cache(maxsize=None)
def margins(name):
    c = case(name)
    bad, fig = [], {}
    if c.robust:
        ref = reference_robust(name)
        (Pd, _, Rd), (Pp, _, Rp) = ref["direct"], ref["pcg"]
        if (Rd["outer_iterations"], Rd["stop_reason"]) != (Rp["outer_iterations"], Rp["stop_reason"]):
            bad.append(f"(e) outer iterations / stop differ: direct {Rd['outer_iterations']} / {Rd['stop_reason']}, PCG "
                       f"{Rp['outer_iterations']} / {Rp['stop_reason']}")
        if not np.array_equal(kind(Rd["scale"]), kind(Rp["scale"])):
            bad.append("(e) the kinds of the scales differ between direct and PCG")
        if Rd["gn_per_solve"] != Rp["gn_per_solve"]:
            bad.append(f"(e) gn_per_solve differs: direct {Rd['gn_per_solve']}, PCG {Rp['gn_per_solve']}")
        fig.update(outer=Rp["outer_iterations"], gap=float(np.max(np.abs(Pd - Pp))), nearest=np.inf)
        c2 = GR.DEFAULTS["noise_chi2"]
        for lin in ("direct", "pcg"):
            first, outer = trace_robust(c.graph["init"], edges_of(c.graph), lin, **c.cfg)
            if len(outer) != ref[lin][2]["outer_iterations"]:
                bad.append(f"(e) {lin}: the replay ran {len(outer)} outer iterations, solve_robust {ref[lin][2]['outer_iterations']}")
            maxes = [first] + [float(np.max(r)) for _, _, _, r, _ in outer]
            for t, mx in enumerate(maxes):
                fig["nearest"] = min(fig["nearest"], abs(mx / c2 - 1.0))
                if abs(mx - c2) <= STAT_GAP * c2:
                    bad.append(f"(e) {lin}: max r {mx!r} within {STAT_GAP} of noise_chi2 at outer iteration {t}")
            for t, (mu, lo, hi, r, s) in enumerate(outer, 1):
                for what, v in (("lo", lo), ("hi", hi)):
                    near = float(np.min(np.abs(r / v - 1.0)))
                    fig["nearest"] = min(fig["nearest"], near)
                    if near <= STAT_GAP:
                        bad.append(f"(e) {lin}: an r within {near:.1e} relative of {what} {v!r} at outer iteration {t}")
        return Margins(tuple(bad), fig)
    ref = reference(name)
    (Pd, Id, Td), (Pp, Ip, Tp) = ref["direct"], ref["pcg"]
    for k in ("iterations", "stop_reason", "reverted"):
        if Id[k] != Ip[k]:
            bad.append(f"(a) {k}: direct {Id[k]}, PCG {Ip[k]}")
    gap = float(np.max(np.abs(Pp - Pd)))
    bar = far_bar()[0] if name == "far" else POSE_GAP
    if not gap <= bar:
        bad.append(f"(b) max |P_pcg - P_direct| {gap:.2e} above {bar:.2e}")
    step_tol = {**GN.DEFAULTS, **c.cfg}["step_tol"]
    for lin, info, tr in (("direct", Id, Td), ("PCG", Ip, Tp)):
        if len(tr) != info["iterations"]:
            bad.append(f"{lin}: the replay ran {len(tr)} iterations, solve {info['iterations']}")
        bad += [f"{lin} {t}" for t in trace_margins(tr, step_tol)]
    fig.update(gap=gap, bar=bar, iterations=Id["iterations"], stop=Id["stop_reason"], reverted=Id["reverted"],
               steps=[t[0] for t in Td], cost_changes=[(t[2] - t[1]) / t[1] if t[1] > 0 else 0.0 for t in Td])
    return Margins(tuple(bad), fig)


def margins_ok(name):
    """every margin condition of the case holds, on the restatement alone"""
    return not margins(name).failures
