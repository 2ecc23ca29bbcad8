"""-m gpu: the robust mode of the pose graph (k_graph_reweight in tl_graph.hip, the outer loop in
tl_api_graph.hip) against its numpy restatement (tests/graph_robust_np.py, conjugate gradients as the device runs them) on lap
graphs with false loop edges; that runs give the same bits; that the mode off is the plain solve bit for bit; the context's graph
on section 17's out-and-back pass (the recipe of tests/test_gpu_graph.py, rebuilt here) through tloam_graph_optimize, the loop
scales, the closed map; and the refusals."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import graph_np as GN  # noqa: E402
import graph_robust_np as GR  # noqa: E402
import loop_np as LN  # noqa: E402
from tloam_amd import synth_graph as SG  # noqa: E402
from tloam_amd import synth_revisit as RV  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(200, seed, k) for k in (1, 4, 8) for seed in (0, 1, 2)] + [(1000, 1, 10)]   # tests/test_graph_robust_np.py's
POSE_BAR = 1e-9   # the single solve's; section 20 has the robust run's measured difference
FEATURE = dict(radius=0.5, cvr_submap=0.05)
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


def kind(s):
    """a scale's decision: 0 rejected, 1 kept, 2 in between"""
    return np.where(s == 0.0, 0, np.where(s == 1.0, 1, 2))


def graph_args(g):
    return g["init"], g["i"], g["j"], g["Z"], g["w"]


def corrupted(n, seed, n_bad):
    g = SG.laps(n, seed=seed)
    bad = SG.false_loops(g, n_bad, seed)
    return g, bad


@pytest.fixture(scope="module")
def ctx(hip_module):
    H = hip_module.HipRegistration()
    yield H
    H.close()


@pytest.fixture(scope="module")
def on(hip_module):
    return hip_module.default_graph_robust_config(enabled=1)


@pytest.fixture(scope="module")
def solved(ctx, on):
    """per case: the graph, its false edges, the device's robust result"""
    out = {}
    for n, seed, k in CASES:
        g, bad = corrupted(n, seed, k)
        out[(n, seed, k)] = (g, bad, ctx.graph_solve_robust(*graph_args(g), rcfg=on))
    return out


# ---- 1: parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_device_equals_the_restatement(hip_module, ctx, solved, case):
    n, seed, k = case
    g, bad, (P, info, rinfo, scale, chi2) = solved[case]
    want, winfo, R = GR.solve_robust(g["init"], GN.as_edges(g["i"], g["j"], g["Z"], g["w"]), linear="pcg")
    diff = float(np.max(np.abs(P - want)))
    sdiff = float(np.max(np.abs(scale - R["scale"])))
    rdiff = float(np.max(np.abs(chi2 - R["chi2"]) / np.maximum(R["chi2"], 1.0)))
    # an inner solve's Gauss-Newton count: the totals of the runs that stop after t and after t - 1 outer iterations
    totals = [ctx.graph_solve_robust(*graph_args(g), rcfg=hip_module.default_graph_robust_config(enabled=1, max_outer=t))[2]
              for t in range(1, rinfo["outer_iterations"] + 1)]
    first = ctx.graph_solve(*graph_args(g))[1]["iterations"]
    gn = [first] + list(np.diff([first] + [t["gn_iterations"] for t in totals]))
    print(f"N {n} seed {seed} false {k}: outer {rinfo['outer_iterations']} / {R['outer_iterations']} stop {rinfo['stop']} GN "
          f"{rinfo['gn_iterations']} / {R['gn_iterations']} PCG {rinfo['cg_iterations']} / {R['cg_iterations']} mu "
          f"{rinfo['mu_first']:.4g} -> {rinfo['mu_last']:.4g} max chi2 {rinfo['max_chi2_first']:.4g}; rejected {rinfo['rejected']} "
          f"kept {rinfo['kept']}; max |pose - restatement| {diff:.2e} |scale - restatement| {sdiff:.2e} relative |chi2 - "
          f"restatement| {rdiff:.2e}; position error {SG.position_error(P, g['truth']):.3f} m; per-solve GN {gn}")
    assert np.array_equal(kind(scale), kind(R["scale"]))
    assert sdiff <= POSE_BAR
    assert (rinfo["outer_iterations"], rinfo["stop_reason"]) == (R["outer_iterations"], R["stop_reason"])
    assert [int(v) for v in gn] == R["gn_per_solve"]
    assert totals[-1] == rinfo                                   # (the run that is allowed exactly as many is the run itself)
    assert rinfo["gn_iterations"] == R["gn_iterations"] and info["iterations"] == winfo["iterations"]
    assert info["stop_reason"] == winfo["stop_reason"] and info["reverted"] == winfo["reverted"]
    assert diff <= POSE_BAR
    assert rdiff <= 1e-6                                         # (r moves with the poses: 2 w e de, w up to 1e6)
    assert (rinfo["rejected"], rinfo["kept"], rinfo["undecided"]) == (R["rejected"], R["kept"], R["undecided"])
    assert abs(rinfo["mu_first"] / R["mu_first"] - 1) <= 1e-9 and abs(rinfo["mu_last"] / R["mu_last"] - 1) <= 1e-9
    assert abs(info["initial_cost"] / winfo["initial_cost"] - 1) <= 1e-9 and abs(info["final_cost"] / winfo["final_cost"] - 1) <= 1e-6
    # and what the mode is for
    assert np.all(scale[bad - (n - 1)] == 0.0) and rinfo["rejected"] <= k + 1
    assert SG.position_error(P, g["truth"]) < 2.0 < 5.0 < SG.position_error(ctx.graph_solve(*graph_args(g))[0], g["truth"])


# ---- 2: the same bits ------------------------------------------------------------------------------------------------------
def test_two_runs_and_two_contexts_give_the_same_bits(hip_module, ctx, solved, on):
    for case in ((1000, 1, 10), (200, 1, 4)):   # (the second in the storage of a larger graph, reused)
        g, _, (P, info, rinfo, scale, chi2) = solved[case]
        P2, info2, rinfo2, scale2, chi22 = ctx.graph_solve_robust(*graph_args(g), rcfg=on)
        assert bits(P2) == bits(P) and bits(scale2) == bits(scale) and bits(chi22) == bits(chi2)
        assert same_info(info2, info) and same_info(rinfo2, rinfo)
    H = hip_module.HipRegistration()
    H.graph_robust_configure(enabled=1)          # (rcfg None: the context's)
    P3, info3, rinfo3, scale3, chi23 = H.graph_solve_robust(*graph_args(g))
    H.close()
    assert bits(P3) == bits(P) and bits(scale3) == bits(scale) and bits(chi23) == bits(chi2)
    assert same_info(info3, info) and same_info(rinfo3, rinfo)


# ---- 3: the mode off -------------------------------------------------------------------------------------------------------
def test_mode_off_is_the_plain_solve(hip_module, ctx, solved):
    reg = hip_module
    for case in ((200, 0, 4), (1000, 1, 10)):
        g = solved[case][0]
        want, winfo = ctx.graph_solve(*graph_args(g))
        for rcfg in (None, reg.default_graph_robust_config(), reg.default_graph_robust_config(enabled=0, noise_chi2=1.0)):
            P, info, rinfo, scale, chi2 = ctx.graph_solve_robust(*graph_args(g), rcfg=rcfg)
            assert bits(P) == bits(want) and same_info(info, winfo)
            assert rinfo["stop"] == "off" and rinfo["outer_iterations"] == 0 and rinfo["gn_iterations"] == 0
            assert np.all(scale == 1.0) and len(scale) == g["n_loops"] and np.all(np.isnan(chi2))


# ---- 4: all inliers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(200, 0), (200, 2), (1000, 0)])
def test_all_inliers_is_the_plain_solve(ctx, on, n, seed):
    g = SG.laps(n, seed=seed)
    want, winfo = ctx.graph_solve(*graph_args(g))
    P, info, rinfo, scale, chi2 = ctx.graph_solve_robust(*graph_args(g), rcfg=on)
    r = GR.edge_stat(want, GR.loop_edges(n, GN.as_edges(g["i"], g["j"], g["Z"], g["w"])))
    print(f"N {n} seed {seed}: max chi2 {rinfo['max_chi2_first']:.4g} (numpy at the device's poses {float(np.max(r)):.4g})")
    assert rinfo["max_chi2_first"] <= 36.0
    assert bits(P) == bits(want) and same_info(info, winfo)
    assert rinfo["stop"] == "all_inliers" and rinfo["outer_iterations"] == 0 and rinfo["gn_iterations"] == winfo["iterations"]
    assert rinfo["cg_iterations"] == winfo["cg_iterations"] and (rinfo["rejected"], rinfo["kept"], rinfo["undecided"]) == (0, g["n_loops"], 0)
    assert np.all(scale == 1.0) and np.max(np.abs(chi2 - r) / np.maximum(r, 1.0)) <= 1e-9
    assert rinfo["max_chi2_first"] == float(np.max(chi2)) and rinfo["mu_first"] == 0.0


def test_all_loop_edges_false_and_one_outer_iteration(hip_module, ctx, on):
    g = SG.laps(200, seed=0)
    SG.false_loops(g, g["n_loops"], 0)
    P, info, rinfo, scale, chi2 = ctx.graph_solve_robust(*graph_args(g), rcfg=on)
    diff = float(np.max(np.abs(P - g["init"])))
    print(f"all false: outer {rinfo['outer_iterations']} rejected {rinfo['rejected']} max |pose - chained guess| {diff:.2e}")
    assert rinfo["stop"] == "binary" and rinfo["rejected"] == g["n_loops"] and np.all(scale == 0.0) and diff <= 1e-6
    g, _ = corrupted(200, 0, 4)
    P, info, rinfo, scale, chi2 = ctx.graph_solve_robust(*graph_args(g), rcfg=hip_module.default_graph_robust_config(enabled=1, max_outer=1))
    assert rinfo["stop"] == "outer_limit" and rinfo["outer_iterations"] == 1 and rinfo["undecided"] > 0
    assert rinfo["mu_last"] == rinfo["mu_first"] and np.all((scale >= 0.0) & (scale <= 1.0))
    assert rinfo["rejected"] + rinfo["kept"] + rinfo["undecided"] == g["n_loops"]


# ---- 5: through the context ------------------------------------------------------------------------------------------------
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


def ob_context(reg, ob):
    thin, poses, _, lists = ob
    H = reg.HipRegistration()
    H.place_configure(enabled=1, exclude_recent=EX)
    H.loop_configure(enabled=1)
    for k in range(len(poses)):
        assert H.place_add_scan(thin[k], poses[k], 100 + k) == k
        H.place_set_keyframe_clouds(k, *lists[k])
    assert H.loop_verify_pending() > 0
    return H


def context_graph(reg, H, cfg):
    """the graph tloam_graph_optimize states, from the public reads: (poses, i, j, Z, w), the loop edges' constraint indices"""
    P = H.place_read_keyframes()["poses"]
    allc = H.loop_constraints()
    idx = [k for k, c in enumerate(allc) if c["accepted"]]
    cons = [allc[k] for k in idx]
    n = len(P)
    wo = [1.0 / (cfg.odom_sigma_t * cfg.odom_sigma_t)] * 3 + [1.0 / (cfg.odom_sigma_r * cfg.odom_sigma_r)] * 3
    wl = [1.0 / (cfg.loop_sigma_t * cfg.loop_sigma_t)] * 3 + [1.0 / (cfg.loop_sigma_r * cfg.loop_sigma_r)] * 3
    i = list(range(n - 1)) + [c["match"] for c in cons]
    j = list(range(1, n)) + [c["query"] for c in cons]
    Z = [LN.t_rel(P[k], P[k + 1]) for k in range(n - 1)] + [c["rel_pose"] for c in cons]
    return (P, i, j, np.array(Z), np.array([wo] * (n - 1) + [wl] * len(cons))), idx


def test_through_the_context(hip_module, ob):
    reg = hip_module
    H = ob_context(reg, ob)
    fresh = ob_context(reg, ob)
    cfg = reg.default_graph_config()
    plain_info = fresh.graph_optimize()
    plain = fresh.graph_poses()
    args, idx = context_graph(reg, H, cfg)
    assert len(idx) == plain_info["n_loop_edges"] > 0
    with not_ready(reg):
        H.graph_read_loop_scales(0, 0)
    with not_ready(reg):
        H.graph_robust_info()
    # a non-robust optimise: every scale is 1
    H.graph_optimize()
    ci, scale, chi2 = H.graph_read_loop_scales()
    assert ci.tolist() == idx and np.all(scale == 1.0) and np.all(np.isnan(chi2)) and H.graph_robust_info()["stop"] == "off"
    # the pass's own constraints are true: at the default bound the robust run may well keep them all.  A tight bound makes
    # the outer loop run, whatever it decides: the context must do what the public solve does
    for over in (dict(), dict(noise_chi2=1e-3, max_outer=12)):
        rcfg = reg.default_graph_robust_config(enabled=1, **over)
        H.graph_robust_configure(rcfg)
        with not_ready(reg):                       # configuring drops the corrected poses
            H.graph_poses(0, 1)
        with not_ready(reg):
            H.graph_read_loop_scales(0, 0)
        info = H.graph_optimize()
        got, rinfo = H.graph_poses(), H.graph_robust_info()
        want, winfo, wrinfo, wscale, wchi2 = H.graph_solve_robust(*args, rcfg=rcfg)
        ci, scale, chi2 = H.graph_read_loop_scales()
        print(f"context graph, {over}: {info['n_loop_edges']} loop edges, outer {rinfo['outer_iterations']} stop {rinfo['stop']} "
              f"max chi2 {rinfo['max_chi2_first']:.4g} rejected {rinfo['rejected']} kept {rinfo['kept']} undecided "
              f"{rinfo['undecided']} GN {rinfo['gn_iterations']}")
        assert bits(got) == bits(want) and same_info(info, winfo) and same_info(rinfo, wrinfo)
        assert ci.tolist() == idx and bits(scale) == bits(wscale) and bits(chi2) == bits(wchi2)
        c1, s1, r1 = H.graph_read_loop_scales(1, 1)
        assert c1.tolist() == idx[1:2] and bits(s1) == bits(scale[1:2]) and bits(r1) == bits(chi2[1:2])
        with invalid(reg):
            H.graph_read_loop_scales(len(idx), 1)
        assert rinfo["stop"] != "off" and rinfo["rejected"] + rinfo["kept"] + rinfo["undecided"] == len(idx)
        if over:
            assert rinfo["outer_iterations"] >= 1
        # the corrected poses' readers use them with no change of their own
        assert np.max(np.abs(H.graph_correct_pose(5, args[0][5]) - got[5])) <= 1e-12
        cm = H.closed_map_build(pose_source=1)
        assert cm["pose_source"] == 1 and bits(H.closed_map_poses()) == bits(got)
    # configured and then disabled: a fresh context's bits
    H.graph_robust_configure(enabled=0)
    with not_ready(reg):
        H.graph_poses(0, 1)
    off_info = H.graph_optimize()
    assert bits(H.graph_poses()) == bits(plain) and same_info(off_info, plain_info)
    assert H.graph_robust_info()["stop"] == "off" and np.all(H.graph_read_loop_scales()[1] == 1.0)
    # the robust configuration persists across a reset; the corrected poses do not
    H.graph_robust_configure(enabled=1, max_outer=3)
    H.graph_optimize()
    H.odometry_reset(None, odom_cfg(reg))
    with not_ready(reg):
        H.graph_read_loop_scales(0, 0)
    g, _ = corrupted(200, 0, 4)
    assert H.graph_solve_robust(*graph_args(g))[2]["outer_iterations"] == 3
    H.close(); fresh.close()


# ---- 6: refusals -----------------------------------------------------------------------------------------------------------
def test_bad_configurations_and_a_sharded_context_are_refused(hip_module, ctx, on):
    reg = hip_module
    g = SG.laps(40, seed=6)
    for over in (dict(noise_chi2=0.0), dict(noise_chi2=-1.0), dict(noise_chi2=np.inf), dict(noise_chi2=np.nan), dict(mu_factor=1.0),
                 dict(mu_factor=0.5), dict(mu_factor=np.inf), dict(mu_factor=np.nan), dict(max_outer=0), dict(max_outer=10001)):
        for enabled in (0, 1):
            with invalid(reg):
                ctx.graph_solve_robust(*graph_args(g), rcfg=reg.default_graph_robust_config(enabled=enabled, **over))
            with invalid(reg):
                ctx.graph_robust_configure(enabled=enabled, **over)
    with invalid(reg):   # the graph's validation is tloam_graph_solve's
        ctx.graph_solve_robust(g["init"], g["i"][:38], g["j"][:38], g["Z"][:38], g["w"][:38], rcfg=on)   # fewer edges than the chain
    w = g["w"].copy()
    w[-1, 2] = -1.0
    with invalid(reg):
        ctx.graph_solve_robust(g["init"], g["i"], g["j"], g["Z"], w, rcfg=on)
    with invalid(reg):
        ctx.graph_solve_robust(*graph_args(g), cfg=reg.default_graph_config(max_iterations=0), rcfg=on)
    # one node, or the chain alone: the solver is not run
    n = 40
    P, info, rinfo, scale, chi2 = ctx.graph_solve_robust(g["init"], g["i"][: n - 1], g["j"][: n - 1], g["Z"][: n - 1], g["w"][: n - 1], rcfg=on)
    assert bits(P) == bits(g["init"]) and info["stop"] == "not_run" and rinfo["stop"] == "all_inliers" and len(scale) == 0
    with not_ready(reg):
        ctx.graph_read_loop_scales(0, 0)
    with not_ready(reg):
        ctx.graph_robust_info()
    H = reg.HipRegistration()
    H.comm_init_callback(0, 2, lambda dev, count, stream: 0)
    with invalid(reg):
        H.graph_robust_configure(enabled=1)
    with invalid(reg):
        H.graph_solve_robust(*graph_args(g), rcfg=on)
    with invalid(reg):
        H.graph_read_loop_scales(0, 0)
    with invalid(reg):
        H.graph_robust_info()
    H.close()
