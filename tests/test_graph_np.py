"""The keyframe pose-graph optimisation without a GPU: the numpy restatement (tests/graph_np.py) against an
independent dense Gauss-Newton, its Jacobians against central differences, the chain preconditioner's prefix form against a direct
solve of M, the contract's stops, the generator (tloam_amd/synth_graph.py), and the new ABI types against their ctypes mirrors."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import graph_np as GN  # noqa: E402
from tloam_amd import registration as reg  # noqa: E402
from tloam_amd import synth_graph as SG  # noqa: E402

ROOT = os.path.dirname(HERE)
GRAPH_SYMBOLS = ("tloam_graph_default_config", "tloam_graph_configure", "tloam_graph_solve", "tloam_graph_optimize",
                 "tloam_graph_read_poses", "tloam_graph_correct_pose")


def graph(n, seed, **kw):
    g = SG.laps(n, seed=seed, **kw)
    return g, GN.as_edges(g["i"], g["j"], g["Z"], g["w"])


def dense_gauss_newton(P, E, iters=12):
    """the contract's iteration with J assembled entry by entry and numpy.linalg.solve; no stop but the count"""
    P = np.array(P, float)
    n, m = len(P), len(E["i"])
    W = np.diag(E["w"].reshape(-1))
    for _ in range(iters):
        J = np.zeros((6 * m, 6 * n))
        e = np.zeros(6 * m)
        for k in range(m):
            i, j = int(E["i"][k]), int(E["j"][k])
            Tji = np.linalg.inv(P[j]) @ P[i]
            R, t = Tji[:3, :3], Tji[:3, 3]
            tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
            Ad = np.block([[R, tx @ R], [np.zeros((3, 3)), R]])
            J[6 * k: 6 * k + 6, 6 * i: 6 * i + 6] = -Ad
            J[6 * k: 6 * k + 6, 6 * j: 6 * j + 6] = np.eye(6)
            e[6 * k: 6 * k + 6] = GN.se3_log(np.linalg.inv(E["Z"][k]) @ np.linalg.inv(P[i]) @ P[j])[0]
        Jr = J[:, 6:]
        d = np.linalg.solve(Jr.T @ W @ Jr, -Jr.T @ W @ e)
        P[1:] = P[1:] @ GN.se3_exp(d.reshape(n - 1, 6))
    return P, float(np.max(np.abs(d)))


def test_pcg_reaches_the_poses_of_a_dense_gauss_newton():
    g, E = graph(40, 3, loop_every=3)
    assert g["n_loops"] >= 5
    want, last = dense_gauss_newton(g["init"], E)
    assert last < 1e-12   # (the fixed point of the contract's iteration)
    got, info = GN.solve(g["init"], E, step_tol=1e-12, max_iterations=12)
    print(info)
    assert info["iterations"] >= 3 and info["cg_iterations"] > 0
    # the restatement stops where the cost no longer resolves a step (STEP) or where it rose (COST): within a step of the fixed point
    assert np.max(np.abs(got - want)) <= max(10 * info["last_step"], 1e-10)
    direct, _ = GN.solve(g["init"], E, linear="direct", step_tol=1e-12, max_iterations=12)
    assert np.max(np.abs(direct - got)) <= 1e-10
    assert SG.position_error(got, g["truth"]) < SG.position_error(g["init"], g["truth"])


def numeric_jacobians(P, E, k, h=1e-6):
    i, j = int(E["i"][k]), int(E["j"][k])
    one = {key: v[k: k + 1] for key, v in E.items()}
    out = []
    for node in (i, j):
        Jn = np.zeros((6, 6))
        for a in range(6):
            d = np.zeros(6)
            d[a] = h
            Pp, Pm = P.copy(), P.copy()
            Pp[node] = P[node] @ GN.se3_exp(d)[0]
            Pm[node] = P[node] @ GN.se3_exp(-d)[0]
            Jn[:, a] = (GN.residuals(Pp, one)[0] - GN.residuals(Pm, one)[0]) / (2 * h)
        out.append(Jn)
    return out


def test_jacobians_against_central_differences():
    g, E = graph(30, 5, loop_every=4)
    # exact where the residual is 0: measurements that agree with the poses
    P = g["truth"]
    exact = GN.as_edges(E["i"], E["j"], GN.inv(P[E["i"]]) @ P[E["j"]], E["w"])
    e, A = GN.linearise(P, exact)
    assert np.max(np.abs(e)) < 1e-12
    for k in (0, 7, len(E["i"]) - 1):
        Ji, Jj = numeric_jacobians(P, exact, k)
        assert np.max(np.abs(Ji + A[k])) < 1e-7 and np.max(np.abs(Jj - np.eye(6))) < 1e-7
    # elsewhere the contract takes the residual's inverse right Jacobian as I: the difference is of the residual's size
    P = g["init"]
    e, A = GN.linearise(P, E)
    for k in (len(E["i"]) - 1, len(E["i"]) - 2):
        Ji, Jj = numeric_jacobians(P, E, k)
        size = np.linalg.norm(e[k])
        assert 1e-3 < size < 1.0
        assert np.linalg.norm(Jj - np.eye(6), 2) <= 0.6 * size + 1e-6
        assert np.linalg.norm(Ji + A[k], 2) <= (0.6 * size + 1e-6) * np.linalg.norm(A[k], 2)


def test_chain_preconditioner_prefix_form_equals_a_direct_solve():
    g, E = graph(60, 2)
    P = g["init"]
    M = GN.chain_matrix(P, E)
    r = np.random.default_rng(0).normal(size=(60, 6))
    r[0] = 0.0
    z = GN.chain_preconditioner(P, E)(r)
    want = np.linalg.solve(M, r[1:].reshape(-1)).reshape(59, 6)
    diff = float(np.max(np.abs(z[1:] - want)))
    print("prefix form against a direct solve of M:", diff, "on entries up to", float(np.max(np.abs(want))))
    assert diff <= 1e-12 * max(1.0, float(np.max(np.abs(want)))) and np.all(z[0] == 0.0)
    # and it is the inverse of what the chain's edges alone assemble to
    Ec = {k: v[:59] for k, v in E.items()}
    back = GN.matvec(60, Ec, GN.linearise(P, Ec)[1], z)
    assert np.max(np.abs(back - r)) <= 1e-9 * np.max(np.abs(r))


def test_matrix_free_product_equals_the_assembled_matrix():
    g, E = graph(25, 1, loop_every=3)
    e, A = GN.linearise(g["init"], E)
    H = GN.normal_matrix(25, E, A)
    p = np.random.default_rng(1).normal(size=(25, 6))
    p[0] = 0.0
    y = GN.matvec(25, E, A, p)
    assert np.max(np.abs(y[1:].reshape(-1) - H @ p[1:].reshape(-1))) <= 1e-9 * np.max(np.abs(y))
    d = GN.direct_solve(25, E, A, GN.rhs(25, E, e, A))
    assert np.max(np.abs(H @ d[1:].reshape(-1) - GN.rhs(25, E, e, A)[1:].reshape(-1))) <= 1e-7 * np.max(np.abs(H)) * np.max(np.abs(d))


def test_contract_edges_of_the_restatement():
    g, E = graph(30, 4, loop_every=4)
    one, info = GN.solve(g["init"][:1], GN.as_edges([], [], np.zeros((0, 4, 4)), np.zeros((0, 6))))
    assert info["stop_reason"] == GN.STOP_NOT_RUN and one.tobytes() == g["init"][:1].tobytes()
    chain = {k: v[:29] for k, v in E.items()}
    same, info = GN.solve(g["init"], chain)
    assert info["stop_reason"] == GN.STOP_NOT_RUN and same.tobytes() == g["init"].tobytes()
    # a loop edge that agrees with the chain: nothing to correct
    agree = GN.as_edges(list(E["i"][:29]) + [3], list(E["j"][:29]) + [20], list(E["Z"][:29]) + [GN.inv(g["init"][3]) @ g["init"][20]],
                        list(E["w"][:29]) + [E["w"][-1]])
    P, info = GN.solve(g["init"], agree)
    assert info["final_cost"] < 1e-18 and np.max(np.abs(P - g["init"])) < 1e-12 and info["stop_reason"] == GN.STOP_STEP
    # one conjugate-gradient iteration per step: says so, stays finite
    P, info = GN.solve(g["init"], E, max_cg_iterations=1, max_iterations=3)
    assert info["stop_reason"] == GN.STOP_CG_LIMIT and np.all(np.isfinite(P)) and info["cg_iterations"] == 3
    # node 0 never moves
    P, info = GN.solve(g["init"], E)
    assert P[0].tobytes() == g["init"][0].tobytes() and info["stop_reason"] in (GN.STOP_STEP, GN.STOP_COST)
    assert info["final_cost"] < info["initial_cost"]


def test_generator():
    a, b = SG.laps(120, seed=2), SG.laps(120, seed=2)
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    n, m = 120, len(a["i"])
    assert list(a["i"][: n - 1]) == list(range(n - 1)) and list(a["j"][: n - 1]) == list(range(1, n))
    assert a["n_loops"] == m - (n - 1) == 12 and np.all(a["i"][n - 1:] + 60 == a["j"][n - 1:])
    assert SG.position_error(a["init"], a["truth"]) > 0.05 and a["init"][0].tobytes() == a["truth"][0].tobytes()
    assert np.max(np.abs(a["init"][5] - a["init"][4] @ a["Z"][4])) < 1e-12
    assert SG.open_chain(50)["n_loops"] == 0 and len(SG.open_chain(50)["i"]) == 49
    for T in a["truth"][::17]:
        assert np.max(np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3))) < 1e-14


def test_graph_struct_layout_matches_the_c_header():
    cfg = ["max_iterations", "max_cg_iterations", "step_tol", "cg_tol", "odom_sigma_t", "odom_sigma_r", "loop_sigma_t", "loop_sigma_r"]
    edge = ["i", "j", "rel_pose_colmajor", "weight"]
    info = ["n_nodes", "n_edges", "n_loop_edges", "iterations", "stop_reason", "reverted", "reserved0", "cg_iterations",
            "initial_cost", "final_cost", "last_step", "last_cg_residual"]
    items = ["sizeof(tloam_graph_config)"] + [f"offsetof(tloam_graph_config, {f})" for f in cfg] + \
            ["sizeof(tloam_graph_edge)"] + [f"offsetof(tloam_graph_edge, {f})" for f in edge] + \
            ["sizeof(tloam_graph_info)"] + [f"offsetof(tloam_graph_info, {f})" for f in info] + \
            ["(size_t)TLOAM_GRAPH_STOP_NOT_RUN", "(size_t)TLOAM_GRAPH_STOP_STEP", "(size_t)TLOAM_GRAPH_STOP_ITERATIONS",
             "(size_t)TLOAM_GRAPH_STOP_COST", "(size_t)TLOAM_GRAPH_STOP_CG_LIMIT"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "tloam_hip.h"\nint main(void) {\n' + \
          "".join(f'  printf("%zu ", {x});\n' for x in items) + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c"); exe = os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = list(map(int, subprocess.check_output([exe]).split()))
    want = []
    for S, fields in ((reg.GraphConfig, cfg), (reg.GraphEdge, edge), (reg.GraphInfo, info)):
        want += [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
        assert [f for f, _ in S._fields_] == fields
    want += [GN.STOP_NOT_RUN, GN.STOP_STEP, GN.STOP_ITERATIONS, GN.STOP_COST, GN.STOP_CG_LIMIT]
    assert vals == want
    assert (C.sizeof(reg.GraphConfig), C.sizeof(reg.GraphEdge), C.sizeof(reg.GraphInfo)) == (56, 192, 80)
    assert sorted(reg.GRAPH_STOP) == [0, 1, 2, 3, 4]


def test_graph_symbols_defaults_and_host_side_refusals():
    L = reg.load_library()
    for s in GRAPH_SYMBOLS:
        assert hasattr(L, s) and s in reg.EXPORTED_SYMBOLS
    cfg = reg.default_graph_config()
    for k, v in GN.DEFAULTS.items():   # the restatement runs with the library's defaults
        assert getattr(cfg, k) == v, k
    assert (cfg.odom_sigma_t, cfg.odom_sigma_r, cfg.loop_sigma_t, cfg.loop_sigma_r) == (0.05, 0.005, 0.05, 0.01)
    assert reg.default_graph_config(cg_tol=1e-6, max_iterations=3).max_iterations == 3
    with pytest.raises(KeyError):
        reg.default_graph_config(no_such_field=1)
    info = reg.GraphInfo()
    out = np.zeros(16)
    assert L.tloam_graph_configure(None, None) == -1 and L.tloam_graph_optimize(None, C.byref(info)) == -1
    assert L.tloam_graph_read_poses(None, 0, 0, None) == -1
    assert L.tloam_graph_correct_pose(None, 0, out.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double))) == -1
    assert L.tloam_graph_solve(None, None, 1, out.ctypes.data_as(C.POINTER(C.c_double)), 0, None,
                               out.ctypes.data_as(C.POINTER(C.c_double)), None) == -1
