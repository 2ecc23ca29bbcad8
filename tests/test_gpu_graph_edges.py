"""-m gpu: the keyframe pose-graph optimisation and its robust mode (DESIGN.md sections 18 and 20; k_graph_step, k_graph_reweight
in tl_graph.hip, the host side in tl_api_graph.hip) on the hand-made graphs of tests/graph_scenes.py, against the numpy
restatement (tests/graph_np.py with a direct solve; tests/graph_robust_np.py with conjugate gradients): every split of the nodes
over the 512 threads, hubs, backward, doubled and node-0 loop edges, far more edges than nodes, a chain that starts off its
measurements, weights over eight decades, a weightless loop, half turns, a run that ends on the cost, coordinates of 2e5 m, 741
loop edges under k_graph_reweight and one.  Every case's margin conditions are checked on the restatement before the device is
asked anything: a case whose stop hangs on rounding would hold the device to the restatement's accident."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import graph_scenes as S  # noqa: E402

pytestmark = pytest.mark.gpu

POSE_BAR = 1e-9
PARITY = [name for name in S.PLAIN if name != "far"]   # (far has a bar of its own: below)
SIZES_ORDER = ("sizes-1026", "tiny-n2_forward", "sizes-514", "sizes-65", "sizes-513", "sizes-1026")


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def same_info(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in b)


def close(a, b, rel):
    """|a - b| <= rel |b| (0 against 0 passes)"""
    return abs(a - b) <= rel * abs(b)


def device_cfg(reg, name, **over):
    return reg.default_graph_config(**{**S.case(name).cfg, **over})


@pytest.fixture(scope="module")
def ctx(hip_module):
    H = hip_module.HipRegistration()
    yield H
    H.close()


@pytest.fixture(scope="module")
def solved(hip_module, ctx):
    """per plain case: the device's poses and info, the restatement's with a direct solve (tests/graph_scenes.reference: computed
    once, read-only) -- after the case's margin conditions"""
    out = {}
    for name in S.PLAIN:
        assert S.margins_ok(name), S.margins(name).failures
        g = S.case(name).graph
        P, info = ctx.graph_solve(*S.args_of(g), device_cfg(hip_module, name))
        want, winfo, _ = S.reference(name)["direct"]
        out[name] = (g, P, info, want, winfo)
    return out


def check_counts_and_stops(name, g, info, winfo):
    assert (info["n_nodes"], info["n_edges"], info["n_loop_edges"]) == (len(g["init"]), len(g["i"]), g["n_loops"])
    assert (info["n_nodes"], info["n_edges"], info["n_loop_edges"]) == (winfo["n_nodes"], winfo["n_edges"], winfo["n_loop_edges"])
    assert info["iterations"] == winfo["iterations"] and info["stop_reason"] == winfo["stop_reason"]
    assert info["reverted"] == winfo["reverted"]


# ---- 1: parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PARITY)
def test_device_equals_the_restatement_with_a_direct_solve(solved, name):
    g, P, info, want, winfo = solved[name]
    diff = float(np.max(np.abs(P - want)))
    rel = abs(info["final_cost"] - winfo["final_cost"]) / winfo["final_cost"] if winfo["final_cost"] > 0.0 else 0.0
    print(f"{name}: N {info['n_nodes']} loops {info['n_loop_edges']} GN {info['iterations']} / {winfo['iterations']} stop "
          f"{info['stop']} / {winfo['stop_reason']} reverted {info['reverted']} PCG {info['cg_iterations']} residual "
          f"{info['last_cg_residual']:.1e} last step {info['last_step']:.2e} / {winfo['last_step']:.2e}; max |pose - restatement| "
          f"{diff:.2e}; cost {info['initial_cost']:.6g} -> {info['final_cost']:.12g} (relative difference {rel:.1e})")
    check_counts_and_stops(name, g, info, winfo)
    assert diff <= POSE_BAR
    assert close(info["final_cost"], winfo["final_cost"], 1e-9) and close(info["initial_cost"], winfo["initial_cost"], 1e-9)
    assert bits(P[0]) == bits(g["init"][0])
    assert np.all(np.isfinite(P)) and S.rigid_error(P) <= 1e-12


# ---- 2: what a case is for -------------------------------------------------------------------------------------------------
def test_reverts_keeps_the_poses_before_the_dropped_step(solved):
    g, P, info, want, winfo = solved["reverts"]
    assert info["reverted"] == 1 and info["stop"] == "cost" and info["final_cost"] < info["initial_cost"]
    assert winfo["reverted"] == 1 and np.max(np.abs(P - want)) <= POSE_BAR      # (solve returns the poses before the dropped step)
    step, cur, new = S.reference("reverts")["direct"][2][-1]
    assert close(info["last_step"], step, 1e-6) and info["iterations"] >= 2


def test_zero_loop_runs_no_conjugate_gradients_and_moves_nothing(solved):
    g, P, info, want, winfo = solved["zero_loop"]
    print("zero_loop:", info)
    assert info["cg_iterations"] == 0 and info["last_cg_residual"] == 0.0 and info["last_step"] == 0.0 and info["stop"] == "step"
    assert info["iterations"] == 1 and info["initial_cost"] == 0.0 and info["final_cost"] == 0.0
    assert np.max(np.abs(P - g["init"])) <= 1e-15                                # (through the quaternions: not bit for bit)


def test_two_nodes_are_the_closed_form(hip_module, ctx):
    g = S.case("tiny-n2_forward").graph
    want = S.two_node_step(g)
    P, info = ctx.graph_solve(*S.args_of(g), device_cfg(hip_module, "tiny-n2_forward", max_iterations=1))
    diff = float(np.max(np.abs(P - want)))
    print(f"N = 2, one step against the 6x6 normal equations: {diff:.2e}")
    assert info["stop"] == "iterations" and info["iterations"] == 1 and diff <= 1e-12
    assert bits(P[0]) == bits(g["init"][0])


def test_node_zero_with_150_loop_edges_stays_its_input(solved):
    g, P, info, want, winfo = solved["hub0"]
    assert S.degree(g, 0) == 151
    assert bits(P[0]) == bits(g["init"][0]) and np.max(np.abs(P - want)) <= POSE_BAR
    assert float(np.max(np.abs(P[1:] - g["init"][1:]))) > 1e-3                   # (its edges are read: the others move)


def test_a_doubled_edge_is_one_edge_of_twice_the_weight(solved):
    ref, refm = S.reference("doubled")["direct"][0], S.reference("doubled-merged")["direct"][0]
    assert np.max(np.abs(ref - refm)) <= 1e-10                                   # the contract's property, on the CPU first
    P, Pm = solved["doubled"][1], solved["doubled-merged"][1]
    diff = float(np.max(np.abs(P - Pm)))
    print(f"doubled against merged on the device: {diff:.2e}")
    assert diff <= POSE_BAR and solved["doubled"][2]["iterations"] == solved["doubled-merged"][2]["iterations"]


# ---- 3: the same bits across sizes -----------------------------------------------------------------------------------------
def test_grow_only_storage_gives_the_same_bits_across_sizes(hip_module, solved):
    """1026, 2, 514, 65, 513, 1026 on one context: a smaller graph in a larger one's storage and back"""
    H = hip_module.HipRegistration()
    got = []
    for name in SIZES_ORDER:
        got.append(H.graph_solve(*S.args_of(S.case(name).graph), device_cfg(hip_module, name)))
    H.close()
    assert bits(got[0][0]) == bits(got[5][0]) and same_info(got[0][1], got[5][1])
    fresh = {}
    for name in set(SIZES_ORDER):
        F = hip_module.HipRegistration()
        fresh[name] = F.graph_solve(*S.args_of(S.case(name).graph), device_cfg(hip_module, name))
        F.close()
    for name, (P, info) in zip(SIZES_ORDER, got):
        assert bits(P) == bits(fresh[name][0]) and same_info(info, fresh[name][1]), name
        assert bits(P) == bits(solved[name][1]) and same_info(info, solved[name][2]), name   # (and the module's context)


# ---- 4: far from the origin ------------------------------------------------------------------------------------------------
def test_far_from_the_origin(solved):
    """1e-9 is not a fair bar at 2e5 m (one rounding of such a coordinate is 3e-11): the bar is measured on the restatement
    (tests/graph_scenes.far_bar).  Rotations carry no large numbers: they keep 1e-9"""
    g, P, info, want, winfo = solved["far"]
    bar, shift, lin = S.far_bar()
    diff = float(np.max(np.abs(P - want)))
    rot = float(np.max(np.abs(P[:, :3, :3] - want[:, :3, :3])))
    print(f"far: bar {bar:.2e} (the shift moves the direct solve by {shift:.2e}, PCG - direct {lin:.2e}); device max |pose - "
          f"restatement| {diff:.2e}, orientations {rot:.2e}; GN {info['iterations']} stop {info['stop']}")
    check_counts_and_stops("far", g, info, winfo)
    assert diff <= bar
    assert rot <= POSE_BAR
    assert close(info["final_cost"], winfo["final_cost"], 1e-6) and bits(P[0]) == bits(g["init"][0])


# ---- 5: robust -------------------------------------------------------------------------------------------------------------
def test_robust_dense_one_outer_iteration_leaves_every_scale_undecided(hip_module, ctx):
    assert S.margins_ok("robust_dense"), S.margins("robust_dense").failures
    g = S.case("robust_dense").graph
    want, winfo, R = S.reference_robust("robust_dense", max_outer=1)["pcg"]
    assert np.all((R["scale"] > 0.0) & (R["scale"] < 1.0)) and len(R["scale"]) == 741
    rcfg = hip_module.default_graph_robust_config(enabled=1, max_outer=1)
    P, info, rinfo, scale, chi2 = ctx.graph_solve_robust(*S.args_of(g), cfg=device_cfg(hip_module, "robust_dense"), rcfg=rcfg)
    sdiff = float(np.max(np.abs(scale - R["scale"])))
    rdiff = float(np.max(np.abs(chi2 - R["chi2"]) / np.maximum(R["chi2"], 1.0)))
    print(f"robust_dense, one outer iteration: |scale - restatement| {sdiff:.2e} relative |chi2 - restatement| {rdiff:.2e} max |pose "
          f"- restatement| {float(np.max(np.abs(P - want))):.2e}")
    assert sdiff <= 1e-9 and rdiff <= 1e-6
    assert (rinfo["rejected"], rinfo["kept"], rinfo["undecided"]) == (0, 0, 741)
    assert rinfo["stop"] == "outer_limit" and rinfo["outer_iterations"] == 1


def test_robust_dense_rejects_the_sixty_false_edges(hip_module, ctx):
    assert S.margins_ok("robust_dense"), S.margins("robust_dense").failures
    g = S.case("robust_dense").graph
    want, winfo, R = S.reference_robust("robust_dense")["pcg"]
    rcfg = hip_module.default_graph_robust_config(enabled=1)
    P, info, rinfo, scale, chi2 = ctx.graph_solve_robust(*S.args_of(g), cfg=device_cfg(hip_module, "robust_dense"), rcfg=rcfg)
    diff = float(np.max(np.abs(P - want)))
    print(f"robust_dense: outer {rinfo['outer_iterations']} / {R['outer_iterations']} stop {rinfo['stop']} GN {rinfo['gn_iterations']} "
          f"/ {R['gn_iterations']} rejected {rinfo['rejected']} kept {rinfo['kept']}; max |pose - restatement| {diff:.2e}")
    assert (rinfo["outer_iterations"], rinfo["stop_reason"]) == (R["outer_iterations"], R["stop_reason"])
    assert np.array_equal(S.kind(scale), S.kind(R["scale"]))
    assert (rinfo["rejected"], rinfo["kept"], rinfo["undecided"]) == (R["rejected"], R["kept"], R["undecided"]) == (60, 681, 0)
    assert rinfo["gn_iterations"] == R["gn_iterations"] == sum(R["gn_per_solve"])
    assert diff <= POSE_BAR
    assert np.all(scale[g["bad"]] == 0.0) and rinfo["stop"] == "binary"


def test_robust_one_rejects_its_single_edge(hip_module, ctx):
    assert S.margins_ok("robust_one"), S.margins("robust_one").failures
    g = S.case("robust_one").graph
    want, winfo, R = S.reference_robust("robust_one")["pcg"]
    rcfg = hip_module.default_graph_robust_config(enabled=1)
    P, info, rinfo, scale, chi2 = ctx.graph_solve_robust(*S.args_of(g), cfg=device_cfg(hip_module, "robust_one"), rcfg=rcfg)
    diff = float(np.max(np.abs(P - g["init"])))
    print(f"robust_one: outer {rinfo['outer_iterations']} / {R['outer_iterations']} stop {rinfo['stop']} max |pose - chained guess| "
          f"{diff:.2e} max |pose - restatement| {float(np.max(np.abs(P - want))):.2e}")
    assert scale.tolist() == [0.0] and (rinfo["rejected"], rinfo["kept"], rinfo["undecided"]) == (1, 0, 0)
    assert (rinfo["outer_iterations"], rinfo["stop_reason"]) == (R["outer_iterations"], R["stop_reason"]) and rinfo["stop"] == "binary"
    assert diff <= 1e-6
