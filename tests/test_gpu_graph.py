"""-m gpu: the keyframe pose-graph optimisation (tl_graph.hip, tl_api_graph.hip) against its numpy
restatement (tests/graph_np.py) run with a direct solve, on the graphs of tloam_amd/synth_graph.py; that it closes the loop; that
runs give the same bits; the context's graph against the public calls on section 17's out-and-back pass (the recipe of
tests/test_gpu_loop.py's `ob_run`, rebuilt here); that the odometry frame is undisturbed; and the edges of the contract."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import graph_np as GN  # noqa: E402
import loop_np as LN  # noqa: E402
from tloam_amd import synth_graph as SG  # noqa: E402
from tloam_amd import synth_hdl64 as G  # noqa: E402
from tloam_amd import synth_revisit as RV  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(200, 0), (200, 1), (200, 2), (1000, 0), (1000, 1), (1000, 2)]
FEATURE = dict(radius=0.5, cvr_submap=0.05)
ODOM_PLACE = dict(kf_dist=2.0, exclude_recent=2)
THIN = dict(n_az=600, rings=np.arange(0, 64, 2))
N_OUT, EX, SEED = 16, 8, 1


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def same_info(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in b)


def invalid(reg):
    return pytest.raises(reg.TloamHipError, match="TLOAM_E_INVALID")


def not_ready(reg):
    return pytest.raises(reg.TloamHipError, match="TLOAM_E_NOT_READY")


@pytest.fixture(scope="module")
def ctx(hip_module):
    H = hip_module.HipRegistration()
    yield H
    H.close()


@pytest.fixture(scope="module")
def solved(ctx):
    """per case: the graph, the device's poses and info, the restatement's with a direct solve"""
    out = {}
    for n, seed in CASES:
        g = SG.laps(n, seed=seed)
        P, info = ctx.graph_solve(g["init"], g["i"], g["j"], g["Z"], g["w"])
        want, winfo = GN.solve(g["init"], GN.as_edges(g["i"], g["j"], g["Z"], g["w"]), linear="direct")
        out[(n, seed)] = (g, P, info, want, winfo)
    return out


# ---- 1: parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_device_equals_the_restatement_with_a_direct_solve(solved, case):
    g, P, info, want, winfo = solved[case]
    diff = float(np.max(np.abs(P - want)))
    rel = abs(info["final_cost"] - winfo["final_cost"]) / winfo["final_cost"]
    print(f"N {case[0]} seed {case[1]}: loops {info['n_loop_edges']} GN {info['iterations']} / {winfo['iterations']} stop "
          f"{info['stop']} / {winfo['stop_reason']} PCG {info['cg_iterations']} residual {info['last_cg_residual']:.1e} last step "
          f"{info['last_step']:.2e}; max |pose - restatement| {diff:.2e}; cost {info['initial_cost']:.6g} -> "
          f"{info['final_cost']:.12g} (relative difference {rel:.1e}); largest correction "
          f"{float(np.max(np.abs(P[:, :3, 3] - g['init'][:, :3, 3]))):.2f} m")
    assert (info["n_nodes"], info["n_edges"], info["n_loop_edges"]) == (case[0], len(g["i"]), g["n_loops"])
    assert diff <= 1e-9
    assert rel <= 1e-9
    assert info["stop_reason"] == winfo["stop_reason"] and info["iterations"] == winfo["iterations"]
    assert info["reverted"] == winfo["reverted"] and abs(info["initial_cost"] / winfo["initial_cost"] - 1) <= 1e-9


# ---- 2: it closes the loop -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_it_closes_the_loop(solved, case):
    g, P, info, want, _ = solved[case]
    before = SG.position_error(g["init"], g["truth"])
    after, after_np = SG.position_error(P, g["truth"]), SG.position_error(want, g["truth"])
    print(f"N {case[0]} seed {case[1]}: largest position error {before:.3f} m -> {after:.3f} m (restatement {after_np:.3f} m)")
    assert after < before
    assert abs(after - after_np) <= 1e-6
    assert info["final_cost"] < info["initial_cost"]


# ---- 3: the same bits ------------------------------------------------------------------------------------------------------
def test_two_contexts_and_two_calls_give_the_same_bits(hip_module, ctx, solved):
    g, P, info, _, _ = solved[(1000, 0)]
    again, info2 = ctx.graph_solve(g["init"], g["i"], g["j"], g["Z"], g["w"])
    assert bits(again) == bits(P) and same_info(info2, info)
    small = solved[(200, 1)]   # (the storage of a larger graph, reused)
    a3, i3 = ctx.graph_solve(small[0]["init"], small[0]["i"], small[0]["j"], small[0]["Z"], small[0]["w"])
    assert bits(a3) == bits(small[1]) and same_info(i3, small[2])
    H = hip_module.HipRegistration()
    other, info4 = H.graph_solve(g["init"], g["i"], g["j"], g["Z"], g["w"])
    H.close()
    assert bits(other) == bits(P) and same_info(info4, info)


# ---- 4: the context's graph equals the public calls ------------------------------------------------------------------------------
def odom_cfg(reg):
    return reg.default_odom_config(**{f"feature__{k}": v for k, v in FEATURE.items()})


def kf_lists(H, reg, xyz):
    """a scan's keyframe clouds through the public stage calls (later-frame lists: selections, down-sampled edge / ground)"""
    cfg = odom_cfg(reg)
    S = H.segment(xyz, cfg.seg)
    assert S["status"] == 0
    ground, edge, general = xyz[S["ground"]], xyz[S["edge"]], xyz[S["general"]]
    ps, pm, ss, sm = H.extract_planar_sphere(general, cfg.feature)
    e_ds = H.voxel_down_sample(edge, cfg.edge_down_sample)
    g_ds = H.voxel_down_sample(ground, cfg.submap.ground_down_sample)
    sel = lambda idx: np.ascontiguousarray(general[idx])  # noqa: E731
    return [sel(ps), g_ds, e_ds, sel(ss)], [sel(pm), g_ds, e_ds, sel(sm)]


@pytest.fixture(scope="module")
def ob(hip_module):
    reg = hip_module
    thin, poses, leg = RV.out_and_back(N_OUT, seed=SEED, **THIN)
    full, _, _ = RV.out_and_back(N_OUT, seed=SEED)
    H = reg.HipRegistration()
    lists = [kf_lists(H, reg, xyz) for xyz in full]
    H.close()
    return thin, poses, leg, lists


def ob_context(reg, ob, keep=None):
    thin, poses, _, lists = ob
    H = reg.HipRegistration()
    H.place_configure(enabled=1, exclude_recent=EX)
    H.loop_configure(enabled=1)
    ks = range(len(poses)) if keep is None else keep
    for f, k in enumerate(ks):
        assert H.place_add_scan(thin[k], poses[k], 100 + k) == f
        H.place_set_keyframe_clouds(f, *lists[k])
    return H


@pytest.fixture(scope="module")
def ob_run(hip_module, ob):
    H = ob_context(hip_module, ob)
    assert H.loop_verify_pending() > 0
    yield H
    H.close()


def context_graph(reg, H, cfg):
    """the graph tloam_graph_optimize states, from the public reads: (poses, i, j, Z, w)"""
    P = H.place_read_keyframes()["poses"]
    cons = [c for c in H.loop_constraints() if c["accepted"]]
    n = len(P)
    wo = [1.0 / (cfg.odom_sigma_t * cfg.odom_sigma_t)] * 3 + [1.0 / (cfg.odom_sigma_r * cfg.odom_sigma_r)] * 3
    wl = [1.0 / (cfg.loop_sigma_t * cfg.loop_sigma_t)] * 3 + [1.0 / (cfg.loop_sigma_r * cfg.loop_sigma_r)] * 3
    i = list(range(n - 1)) + [c["match"] for c in cons]
    j = list(range(1, n)) + [c["query"] for c in cons]
    Z = [LN.t_rel(P[k], P[k + 1]) for k in range(n - 1)] + [c["rel_pose"] for c in cons]
    return P, i, j, np.array(Z), np.array([wo] * (n - 1) + [wl] * len(cons))


def test_context_graph_equals_the_public_calls(hip_module, ob_run):
    reg = hip_module
    H = ob_run
    for cfg in (reg.default_graph_config(), reg.default_graph_config(odom_sigma_t=0.02, loop_sigma_r=0.003)):
        H.graph_configure(cfg)
        with not_ready(reg):
            H.graph_poses(0, 1)
        info = H.graph_optimize()
        got = H.graph_poses()
        P, i, j, Z, w = context_graph(reg, H, cfg)
        want, winfo = H.graph_solve(P, i, j, Z, w)
        print(f"context graph: {info['n_nodes']} keyframes, {info['n_loop_edges']} loop edges, GN {info['iterations']} PCG "
              f"{info['cg_iterations']} stop {info['stop']}, cost {info['initial_cost']:.4g} -> {info['final_cost']:.4g}, largest "
              f"correction {float(np.max(np.abs(got[:, :3, 3] - P[:, :3, 3]))):.4f} m")
        assert info["n_nodes"] == 2 * N_OUT and info["n_loop_edges"] == H.loop_info()["n_accepted"] > 0
        assert info["iterations"] >= 1 and info["final_cost"] < info["initial_cost"]
        assert bits(got) == bits(want) and same_info(info, winfo)
        assert bits(got[0]) == bits(P[0]) and np.max(np.abs(got - P)) > 1e-6
        assert bits(H.place_read_keyframes()["poses"]) == bits(P)   # (the stored poses are not changed)
        for k in (0, 5, 2 * N_OUT - 1):
            assert np.max(np.abs(H.graph_correct_pose(k, P[k]) - got[k])) <= 1e-12
        assert bits(H.graph_correct_pose(-1, P[-1])) == bits(H.graph_correct_pose(2 * N_OUT - 1, P[-1]))
        near = P[7] @ GN.se3_exp([0.3, -0.1, 0.02, 0.0, 0.01, 0.05])[0]
        assert np.max(np.abs(H.graph_correct_pose(7, near) - got[7] @ np.linalg.inv(P[7]) @ near)) <= 1e-12
        assert bits(H.graph_poses(3, 2)) == bits(got[3:5])
        with invalid(reg):
            H.graph_poses(2 * N_OUT, 1)
        with invalid(reg):
            H.graph_correct_pose(2 * N_OUT, P[0])


# ---- 5: undisturbed --------------------------------------------------------------------------------------------------------
def odom_run(reg, scans, hook=None):
    H = reg.HipRegistration()
    H.map_configure(reg.default_map_config(enabled=1))
    H.voxel_map_configure(reg.default_voxel_map_config(enabled=1))
    H.place_configure(enabled=1, **ODOM_PLACE)
    H.loop_configure(enabled=1)
    H.odometry_reset(None, odom_cfg(reg))
    res = []
    for f, xyz in enumerate(scans):
        rc, T, st = H.odometry_frame(xyz)
        assert rc in (0, -7), (f, rc)
        res.append({"pose": T, "stats": st, "reg": H.registered_scan(), "map_info": H.map_info(), "map": H.map_read(),
                    "vinfo": H.voxel_map_info(), "vmap": H.voxel_map_read()})
        if hook:
            hook(f, H)
    H.loop_verify_pending()
    return H, res


def test_odometry_is_undisturbed_by_the_graph_calls(hip_module):
    reg = hip_module
    seq = G.sequence(7, seed=3)[0]
    g = SG.laps(200, seed=0)
    seen = []

    def graph_between_frames(f, H):
        if f in (2, 4):
            seen.append(H.graph_optimize())
            H.graph_poses()
            P, info = H.graph_solve(g["init"], g["i"], g["j"], g["Z"], g["w"])
            assert info["iterations"] >= 2
            seen.append(info)

    Hoff, off = odom_run(reg, seq)
    Hon, on = odom_run(reg, seq, hook=graph_between_frames)
    assert len(seen) == 4 and seen[0]["n_nodes"] >= 1
    for f, (a, b) in enumerate(zip(on, off)):
        assert bits(a["pose"]) == bits(b["pose"]), f
        assert bits(a["reg"]) == bits(b["reg"]), f
        sa, sb = a["stats"], b["stats"]
        for key in sb:
            if key != "match":
                assert sa[key] == sb[key], (f, key)
        for key, v in sb["match"].items():
            if key != "host_wait_us":
                assert np.asarray(sa["match"][key]).tobytes() == np.asarray(v).tobytes(), (f, key)
        assert a["map_info"] == b["map_info"] and bits(a["map"]) == bits(b["map"]), f
        assert a["vinfo"] == b["vinfo"], f
        for x, y in zip(a["vmap"], b["vmap"]):
            assert x.tobytes() == y.tobytes(), f
    ka, kb = Hon.place_read_keyframes(), Hoff.place_read_keyframes()
    for k in ka:
        assert np.asarray(ka[k]).tobytes() == np.asarray(kb[k]).tobytes(), k
    assert Hon.place_loops() == Hoff.place_loops()
    ca, cb = Hon.loop_constraints(), Hoff.loop_constraints()
    assert len(ca) == len(cb)
    for a, b in zip(ca, cb):
        for k in b:
            if k in ("coarse", "fine"):
                assert all(np.asarray(a[k][s]).tobytes() == np.asarray(b[k][s]).tobytes() for s in b[k] if s != "host_wait_us"), k
            else:
                assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    Hon.close(); Hoff.close()


# ---- 6: the edges of the contract ------------------------------------------------------------------------------------------
def test_shortcuts_and_a_loop_that_agrees(ctx):
    g = SG.laps(60, seed=4)
    one, info = ctx.graph_solve(g["init"][:1], [], [], np.zeros((0, 4, 4)), np.zeros((0, 6)))
    assert bits(one) == bits(g["init"][:1]) and info["stop"] == "not_run" and info["iterations"] == 0
    n = 60
    chain, info = ctx.graph_solve(g["init"], g["i"][: n - 1], g["j"][: n - 1], g["Z"][: n - 1], g["w"][: n - 1])
    assert bits(chain) == bits(g["init"]) and info["stop"] == "not_run" and info["n_loop_edges"] == 0
    # a loop edge that agrees with the chain exactly: nothing to correct
    i, j = list(g["i"][: n - 1]) + [3], list(g["j"][: n - 1]) + [41]
    Z = list(g["Z"][: n - 1]) + [GN.inv(g["init"][3]) @ g["init"][41]]
    P, info = ctx.graph_solve(g["init"], i, j, np.array(Z), g["w"][:n])
    print("agreeing loop:", info)
    assert info["final_cost"] < 1e-18 and np.max(np.abs(P - g["init"])) <= 1e-12 and info["stop"] == "step"
    # a loop edge may carry weight 0 in a component (a chain edge may not: below)
    w = g["w"].copy()
    w[n - 1:, 2] = 0.0
    P, info = ctx.graph_solve(g["init"], g["i"], g["j"], g["Z"], w)
    assert np.all(np.isfinite(P)) and info["final_cost"] < info["initial_cost"]


def test_node_zero_never_moves_and_one_cg_iteration_says_so(hip_module, ctx, solved):
    reg = hip_module
    for g, P, *_ in solved.values():
        assert bits(P[0]) == bits(g["init"][0])
    g = solved[(200, 0)][0]
    P, info = ctx.graph_solve(g["init"], g["i"], g["j"], g["Z"], g["w"], reg.default_graph_config(max_cg_iterations=1, max_iterations=3))
    print("max_cg_iterations 1:", info)
    assert info["stop"] == "cg_limit" and info["stop_reason"] == GN.STOP_CG_LIMIT
    assert np.all(np.isfinite(P)) and info["cg_iterations"] <= 3 and 1 <= info["iterations"] <= 3
    P, info = ctx.graph_solve(g["init"], g["i"], g["j"], g["Z"], g["w"], reg.default_graph_config(max_iterations=1))
    assert info["stop"] == "iterations" and info["iterations"] == 1


def test_invalid_graphs_are_refused_and_leave_earlier_results(hip_module, ob_run):
    reg = hip_module
    H = ob_run
    H.graph_configure()
    H.graph_optimize()
    before = H.graph_poses()
    g = SG.laps(40, seed=6)
    n, m = 40, len(g["i"])

    def bad(**change):
        a = {k: np.array(g[k], copy=True) for k in ("init", "i", "j", "Z", "w")}
        for k, (at, v) in change.items():
            a[k][at] = v
        with invalid(reg):
            H.graph_solve(a["init"], a["i"], a["j"], a["Z"], a["w"])

    bad(i=(m - 1, n))                  # an index out of range
    bad(j=(m - 1, -1))
    bad(j=(m - 1, g["i"][m - 1]))      # i == j
    bad(i=(5, 6))                      # a broken chain
    bad(j=(5, 7))
    bad(init=((3, 0, 3), np.nan))      # a non-finite pose
    bad(init=((3, 0, 0), 1.5))         # a non-rigid pose
    bad(Z=((m - 1, 1, 1), 2.0))        # a non-rigid measurement
    bad(Z=((2, 2, 3), np.inf))
    bad(w=((m - 1, 4), -1.0))          # a negative weight
    bad(w=((m - 1, 4), np.nan))
    bad(w=((7, 0), 0.0))               # a chain weight of 0
    with invalid(reg):                 # fewer edges than the chain
        H.graph_solve(g["init"], g["i"][: n - 2], g["j"][: n - 2], g["Z"][: n - 2], g["w"][: n - 2])
    with invalid(reg):                 # no node
        H.graph_solve(np.zeros((0, 4, 4)), [], [], np.zeros((0, 4, 4)), np.zeros((0, 6)))
    for over in (dict(max_iterations=0), dict(max_cg_iterations=0), dict(step_tol=-1.0), dict(cg_tol=np.nan),
                 dict(odom_sigma_t=0.0), dict(loop_sigma_r=np.inf)):
        with invalid(reg):
            H.graph_solve(g["init"], g["i"], g["j"], g["Z"], g["w"], reg.default_graph_config(**over))
        with invalid(reg):
            H.graph_configure(**over)
    assert bits(H.graph_poses()) == bits(before)
    P, info = H.graph_solve(g["init"], g["i"], g["j"], g["Z"], g["w"])   # and the context still solves
    assert info["final_cost"] < info["initial_cost"] and bits(H.graph_poses()) == bits(before)


def test_one_way_optimises_nothing_and_reset_and_configure_drop_the_poses(hip_module, ob):
    reg = hip_module
    _, poses, leg, _ = ob
    out = [k for k in range(len(poses)) if leg[k] == 0]
    H = ob_context(reg, ob, keep=out)
    with not_ready(reg):
        H.graph_poses(0, 0)
    with not_ready(reg):
        H.graph_correct_pose(0, poses[0])
    assert H.loop_verify_pending() == 0
    info = H.graph_optimize()
    assert info["stop"] == "not_run" and info["n_nodes"] == len(out) and info["n_loop_edges"] == 0
    assert bits(H.graph_poses()) == bits(H.place_read_keyframes()["poses"])
    for drop in (lambda: H.graph_configure(), lambda: H.place_configure(enabled=1, exclude_recent=EX),
                 lambda: H.loop_configure(enabled=1), lambda: H.odometry_reset(None, odom_cfg(reg))):
        info = H.graph_optimize()   # (no keyframes after the first drop: still TLOAM_OK)
        assert info["stop"] == "not_run"
        H.graph_poses()
        drop()
        with not_ready(reg):
            H.graph_poses(0, 0)
    H.place_configure(enabled=0)
    with invalid(reg):              # place recognition off
        H.graph_optimize()
    H.close()
