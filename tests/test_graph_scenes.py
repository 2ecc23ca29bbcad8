"""The hand-made pose graphs of tests/graph_scenes.py, on the CPU: every case meets its margin conditions on the restatement
(tests/graph_np.py, tests/graph_robust_np.py) with a direct solve and with conjugate gradients; the generators are deterministic
and rigid; every case has the shape it is named for; and the restatement does on them what the device is then held to
(tests/test_gpu_graph_edges.py)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import graph_np as GN  # noqa: E402
import graph_robust_np as GR  # noqa: E402
import graph_scenes as S  # noqa: E402

ALL = list(S.PLAIN) + list(S.ROBUST)


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def graph(name):
    return S.case(name).graph


# ---- 1: the margins --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_every_case_meets_its_margin_conditions(name):
    M = S.margins(name)
    print(name, S.case(name).cfg, {k: v for k, v in M.figures.items()})
    assert S.margins_ok(name), M.failures


def test_the_margin_checker_sees_a_thin_margin():
    """the conditions bite: lap-like traces that end on a cost change of rounding size, or a step beside step_tol, are refused"""
    assert S.trace_margins([(1e-1, 10.0, 1.0), (2.5e-7, 1.0, 1.0 + 6e-11)], 1e-7) != []       # (c) and (d): the hub at 1e-7
    assert S.trace_margins([(1e-1, 10.0, 1.0), (2.5e-6, 1.0, 1.0 - 6e-11), (1e-9, 1.0, 1.0)], 1e-7) != []   # (d) alone
    assert S.trace_margins([(1e-1, 10.0, 1.0), (3.2e-8, 1.0, 1.0)], 1e-7) == []
    assert S.trace_margins([(1e-1, 10.0, 1.0), (3.4e-8, 1.0, 1.0)], 1e-7) != []               # (c) from below
    assert S.trace_margins([(1e-1, 10.0, 1.0), (1e-3, 1.0, 1.0 + 2e-8)], 1e-7) == []          # a revert by a margin


# ---- 2: the generators -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_generators_are_deterministic_rigid_and_chained(name):
    c = S.case(name)
    g = c.graph
    make = S.PLAIN[name] if name in S.PLAIN else S.ROBUST[name]
    again, cfg = make(seed=S.SEEDS.get(name, 0))
    assert cfg == c.cfg
    for k in ("truth", "init", "Z", "w"):
        assert bits(again[k]) == bits(g[k]), k
    assert np.array_equal(again["i"], g["i"]) and np.array_equal(again["j"], g["j"])
    n, m = len(g["init"]), len(g["i"])
    assert len(g["truth"]) == n and g["Z"].shape == (m, 4, 4) and g["w"].shape == (m, 6) and g["n_loops"] == m - (n - 1) >= 1
    assert np.array_equal(g["i"][: n - 1], np.arange(n - 1)) and np.array_equal(g["j"][: n - 1], np.arange(1, n))
    assert np.all((g["i"] >= 0) & (g["i"] < n) & (g["j"] >= 0) & (g["j"] < n) & (g["i"] != g["j"]))
    assert np.all(g["w"][: n - 1] > 0.0) and np.all(g["w"] >= 0.0) and np.all(np.isfinite(g["w"]))
    for k in ("truth", "init", "Z"):
        assert S.rigid_error(g[k]) <= 1e-14, (k, S.rigid_error(g[k]))
    assert bits(g["init"][0]) == bits(g["truth"][0])


# ---- 3: the shapes ---------------------------------------------------------------------------------------------------------
def loops_of(g):
    n = len(g["init"])
    return list(zip(g["i"][n - 1:].tolist(), g["j"][n - 1:].tolist()))


def test_tiny_and_sizes_split_the_nodes_as_the_table_says():
    assert loops_of(graph("tiny-n2_forward")) == [(0, 1)] and len(graph("tiny-n2_forward")["init"]) == 2
    assert loops_of(graph("tiny-n2_backward")) == [(1, 0)] and len(graph("tiny-n2_backward")["init"]) == 2
    assert loops_of(graph("tiny-n3")) == [(0, 2), (2, 0), (1, 2)] and len(graph("tiny-n3")["init"]) == 3
    split = {}
    for n in S.SIZES:
        g = graph(f"sizes-{n}")
        assert len(g["init"]) == n
        assert loops_of(g) == [(k, k + n // 2) for k in range(0, n - n // 2, 9)] and g["n_loops"] >= 4
        chunk = S.chunk_of(n)
        owned = [max(0, min(1 + (t + 1) * chunk, n) - (1 + t * chunk)) for t in range(S.THREADS)]
        assert sum(owned) == n - 1
        split[n] = (chunk, sum(1 for o in owned if o == chunk), [o for o in owned if 0 < o < chunk], sum(1 for o in owned if o == 0))
    # (chunk, full threads, partial chunks, idle threads)
    assert split[65] == (1, 64, [], 448)          # exactly one wave
    assert split[66] == (1, 65, [], 447)          # one lane of the second
    assert split[513] == (1, 512, [], 0)          # every thread owns one node
    assert split[514] == (2, 256, [1], 255)       # thread 256 owns one node of its two, 255 threads own none
    assert split[1026] == (3, 341, [2], 170)      # thread 341 owns 2 of 3


def test_hubs_dense_doubled_and_backwards_have_their_edges():
    g = graph("hub")
    assert S.degree(g, 7) == 2 + 150 and int(np.sum(g["i"][199:] == 7)) == 75 and int(np.sum(g["j"][199:] == 7)) == 75
    assert sorted(a + b - 7 for a, b in loops_of(g)) == list(range(20, 170))
    g = graph("hub0")
    assert S.degree(g, 0) == 1 + 150 and int(np.sum(g["i"][199:] == 0)) == 75 and int(np.sum(g["j"][199:] == 0)) == 75
    assert sorted(a + b for a, b in loops_of(g)) == list(range(10, 160))
    g = graph("dense")
    assert len(g["init"]) == 30 and g["n_loops"] == 406 and len(g["i"]) == 435 and len(set(loops_of(g))) == 406
    assert min(S.degree(g, k) for k in range(30)) == 29 and all(b >= a + 2 for a, b in loops_of(g))
    g, gm = graph("doubled"), graph("doubled-merged")
    lo, first = loops_of(g), 119
    assert len(g["init"]) == 120 and len(lo) == 26 and len(loops_of(gm)) == 14
    for q in range(12):      # each pair twice, one after the other, the same bits
        assert lo[2 * q] == lo[2 * q + 1] == loops_of(gm)[q]
        for k in ("Z", "w"):
            assert bits(g[k][first + 2 * q]) == bits(g[k][first + 2 * q + 1])
        assert bits(gm["Z"][first + q]) == bits(g["Z"][first + 2 * q]) and bits(gm["w"][first + q]) == bits(2.0 * g["w"][first + 2 * q])
    k = S.DOUBLED_BESIDE
    assert lo[24:] == [(k, k + 1), (k + 1, k)] == loops_of(gm)[12:]
    assert bits(gm["init"]) == bits(g["init"]) and bits(gm["Z"][: first]) == bits(g["Z"][: first])
    g = graph("backwards")
    assert len(g["init"]) == 300 and loops_of(g) == [(k + 100, k) for k in range(0, 197, 7)]
    assert int(np.sum(g["i"] > g["j"])) == g["n_loops"] == 29 and S.degree(g, 0) == 2
    for name in ("perturbed", "aniso", "far"):
        assert loops_of(graph(name)) == [(k, k + 100) for k in range(0, 197, 7)] and len(graph(name)["init"]) == 300


def test_perturbed_aniso_zero_loop_reverts_far_and_robust_have_their_numbers():
    g = graph("perturbed")
    E = S.edges_of(g)
    e0 = GN.residuals(g["init"], E)[:299]
    assert 0.02 < float(np.max(np.abs(e0))) < 0.2                                  # the chain's residuals at the start
    assert float(np.max(np.abs(GN.residuals(graph("aniso")["init"], S.edges_of(graph("aniso")))[:299]))) < 1e-13
    w = graph("aniso")["w"][299:]
    assert w.min() >= 1e-2 and w.max() <= 1e6 and w.max() / w.min() > 1e7 and len(np.unique(w)) == w.size
    g = graph("zero_loop")
    assert len(g["init"]) == 60 and loops_of(g) == [(10, 50)] and np.all(g["w"][59] == 0.0)
    e = GN.residuals(g["init"], S.edges_of(g))
    assert np.all(e[:59] == 0.0) and float(np.max(np.abs(e[59]))) > 0.3            # an exact chain, a loop that disagrees
    g = graph("reverts")
    assert len(g["init"]) == 100 and loops_of(g) == [(k, k + 50) for k in range(0, 50, 5)]
    g = graph("far")
    u = g["unshifted"]
    assert bits(g["Z"]) == bits(u["Z"]) and np.max(np.abs(g["init"][:, :3, 3])) > 1.8e5 > 200.0 > np.max(np.abs(u["init"][:, :3, 3]))
    assert np.max(np.abs(g["G"] @ u["init"] - g["init"])) <= 1e-10
    g = graph("robust_dense")
    assert len(g["init"]) == 40 and g["n_loops"] == 741 > S.THREADS and len(g["bad"]) == len(set(g["bad"].tolist())) == 60
    g = graph("robust_one")
    assert len(g["init"]) == 80 and loops_of(g) == [(5, 60)] and g["bad"].tolist() == [0]


def test_half_turns_are_exact_and_every_quaternion_branch_occurs():
    g = graph("half_turns")
    R = g["truth"][:, :3, :3]
    exact = [k for k in range(90) if abs(np.trace(R[k]) + 1.0) < 1e-12]
    assert exact == list(range(0, 90, 5)) and g["n_loops"] == 8 and len(g["init"]) == 90
    for k in exact:
        assert bits(R[k]) == bits(S.HALF_TURNS[k % 3][:3, :3])
    assert {S.quat_branch(R[k]) for k in exact} == {1, 2, 3}
    # neighbours half a turn apart: qw ~ 0 in rigid_inverse(P_i) * P_j, about every axis
    rel = GN.inv(g["init"][:-1]) @ g["init"][1:]
    assert np.max(np.abs(np.trace(rel[:, :3, :3], axis1=1, axis2=2) + 1.0)) < 0.1
    assert {S.quat_branch(T[:3, :3]) for T in g["Z"]} >= {1, 2, 3}
    seen = set()
    for name in [f"sizes-{n}" for n in S.SIZES] + ["half_turns"]:
        gg = graph(name)
        for key in ("init", "Z"):
            seen |= {S.quat_branch(T[:3, :3]) for T in gg[key]}
    assert seen == {0, 1, 2, 3}
    for n in (513, 514, 1026):   # and the walk alone reaches them all at the larger sizes
        assert {S.quat_branch(T[:3, :3]) for T in graph(f"sizes-{n}")["init"]} == {0, 1, 2, 3}, n


# ---- 4: what the restatement does on them ------------------------------------------------------------------------------------
def test_reverts_ends_on_the_cost_with_a_lower_cost_than_it_started_with():
    for lin in ("direct", "pcg"):
        P, info, tr = S.reference("reverts")[lin]
        assert (info["stop_reason"], info["reverted"]) == (GN.STOP_COST, 1)
        assert info["final_cost"] < info["initial_cost"] and info["iterations"] >= 2
        step, cur, new = tr[-1]
        print(f"reverts ({lin}): iteration {len(tr)} dropped at max |d| {step:.2e} on a cost rise of {(new - cur) / cur:.2e} relative")
        assert step > 1e-4 and new - cur >= 1e-7 * cur       # by a margin, far above step_tol


def test_zero_loop_is_one_iteration_that_moves_nothing():
    g = graph("zero_loop")
    for lin in ("direct", "pcg"):
        P, info, tr = S.reference("zero_loop")[lin]
        assert (info["stop_reason"], info["iterations"], info["reverted"]) == (GN.STOP_STEP, 1, 0)
        assert info["final_cost"] == info["initial_cost"] == 0.0 and info["last_step"] == 0.0
        assert np.max(np.abs(P - g["init"])) <= 1e-15
    assert S.reference("zero_loop")["pcg"][1]["cg_iterations"] == 0 and S.reference("zero_loop")["pcg"][1]["last_cg_residual"] == 0.0


def test_a_doubled_edge_is_one_edge_of_twice_the_weight():
    a, b = S.reference("doubled"), S.reference("doubled-merged")
    for lin in ("direct", "pcg"):
        gap = float(np.max(np.abs(a[lin][0] - b[lin][0])))
        print(f"doubled against merged ({lin}): {gap:.2e}")
        assert gap <= 1e-10
        for k in ("iterations", "stop_reason", "reverted"):
            assert a[lin][1][k] == b[lin][1][k]


def test_two_nodes_are_the_closed_form():
    """N = 2 with both edges (0, 1): J_j = I for both, so one step is (W_0 + W_1) d = -(W_0 e_0 + W_1 e_1)"""
    g = graph("tiny-n2_forward")
    E = S.edges_of(g)
    want = S.two_node_step(g)
    for lin in ("direct", "pcg"):
        P, info = GN.solve(g["init"], E, linear=lin, max_iterations=1)
        assert info["stop_reason"] == GN.STOP_ITERATIONS and np.max(np.abs(P - want)) <= 1e-12


def test_far_bar_is_measured_and_far_from_the_plain_bar():
    bar, shift, lin = S.far_bar()
    print(f"far: the shift moves the direct solve by {shift:.2e}, PCG - direct {lin:.2e}, bar {bar:.2e}")
    assert bar == 10.0 * max(shift, lin) and 1e-11 < bar < 1e-7
    g = graph("far")
    ref, (Pu, iu) = S.reference("far")["direct"], GN.solve(g["unshifted"]["init"], S.edges_of(g["unshifted"]), linear="direct", **S.case("far").cfg)
    assert (ref[1]["iterations"], ref[1]["stop_reason"]) == (iu["iterations"], iu["stop_reason"])


def test_robust_cases_decide_as_the_table_says():
    g = graph("robust_dense")
    for lin in ("direct", "pcg"):
        P, info, R = S.reference_robust("robust_dense", max_outer=1)[lin]
        assert R["stop_reason"] == GR.STOP_OUTER_LIMIT and (R["rejected"], R["kept"], R["undecided"]) == (0, 0, 741)
        assert np.all((R["scale"] > 0.0) & (R["scale"] < 1.0))
        P, info, R = S.reference_robust("robust_dense")[lin]
        print(f"robust_dense ({lin}): outer {R['outer_iterations']} stop {R['stop_reason']} rejected {R['rejected']} kept {R['kept']} "
              f"GN {R['gn_per_solve']}")
        assert R["stop_reason"] == GR.STOP_BINARY and np.all(R["scale"][g["bad"]] == 0.0)
        assert (R["rejected"], R["kept"], R["undecided"]) == (60, 681, 0)
        P, info, R = S.reference_robust("robust_one")[lin]
        assert R["stop_reason"] == GR.STOP_BINARY and R["scale"].tolist() == [0.0]
        assert np.max(np.abs(P - graph("robust_one")["init"])) <= 1e-6
