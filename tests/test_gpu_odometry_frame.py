"""-m gpu: tloam_odometry_frame -- one raw scan in, one pose out, every cloud in between in HBM --
against the same frame driven stage by stage through the public entry points (bit for bit), against the CPU statements
(tests/segmentation_np.py and the oracle), and against the generator's trajectory.

The ray-cast street of tloam_amd/synth_hdl64.py has boxes, walls and ground but nothing round: with feature.yaml's radius
(0.2 m) and cvr_submap (0.15) extractPlanarSphere finds no sphere candidate in it, and a frame without ten sphere points is
skipped.  The tests therefore widen the PCA radius to 0.5 m and lower cvr_submap to 0.05, which gives 13-42 sphere points
per frame on both sequences used here."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import segmentation_np as SNP  # noqa: E402
from conftest import pose_delta  # noqa: E402
from oracle import binding as ob  # noqa: E402
from tloam_amd import replay, synth_hdl64 as G  # noqa: E402
from tloam_amd.synth import Frame  # noqa: E402

pytestmark = pytest.mark.gpu

FEATURE = dict(radius=0.5, cvr_submap=0.05)
# host waits of the stage chain's public calls for a later frame, counted from their code: tloam_segment 2 (control block,
# lists), tloam_voxel_down_sample 2 x 2 (sizes, cloud), tloam_extract_planar_sphere 4 (bounds, sizes, lists, drain),
# tloam_set_source_frame 0, tloam_submap_update 1
CHAIN_SYNCS = 11


def odom_cfg(reg):
    return reg.default_odom_config(**{f"feature__{k}": v for k, v in FEATURE.items()})


def _mul(A, B):   # tl_api_odom.hip mat_mul: sums over k in ascending order
    return [[((A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j]) + A[i][3] * B[3][j] for j in range(4)] for i in range(4)]


def _rigid_inv(T):   # tl_api_odom.hip rigid_inverse
    r = [[0.0] * 4 for _ in range(4)]
    for i in range(3):
        for j in range(3):
            r[i][j] = T[j][i]
        r[i][3] = -((T[0][i] * T[0][3] + T[1][i] * T[1][3]) + T[2][i] * T[2][3])
    r[3][3] = 1.0
    return r


class Predictor:
    """FrontEnd's last_pose / predicate_pose (front_end.cpp:329-332), in the device's operation order"""
    def __init__(self, init=None):
        T = np.eye(4) if init is None else np.asarray(init, float)
        self.last = [[float(v) for v in row] for row in T]
        self.pred = [row[:] for row in self.last]

    def predict(self):
        return np.array(self.pred)

    def accept(self, T):
        T = [[float(v) for v in row] for row in np.asarray(T)]
        step = _mul(_rigid_inv(self.last), T)
        self.pred = _mul(T, step)
        self.last = T


def snapshot(H):
    """what the getters say after a frame"""
    out = {"targets": [H.get_target(k) for k in range(4)], "fitness": H.fitness()}
    out["corr"] = [H.get_correspondences(k) for k in range(4)]
    return out


def chain(reg, scans, cfg):
    """context B: the stage chain through the public calls, host glue in numpy"""
    H = reg.HipRegistration()
    P = Predictor()
    res = []
    for f, xyz in enumerate(scans):
        S = H.segment(xyz, cfg.seg)
        assert S["status"] == 0, f
        ground, edge, general = xyz[S["ground"]], xyz[S["edge"]], xyz[S["general"]]
        ps, pm, ss, sm = H.extract_planar_sphere(general, cfg.feature)
        sel = lambda idx: np.ascontiguousarray(general[idx])  # noqa: E731
        if f == 0:
            H.submap_init(sel(pm), sel(sm), edge, ground, cfg.submap)
            res.append({"pose": np.eye(4), "snap": {"targets": [H.get_target(k) for k in range(4)]}})
            continue
        e_ds = H.voxel_down_sample(edge, cfg.edge_down_sample)
        g_ds = H.voxel_down_sample(ground, cfg.submap.ground_down_sample)
        H.set_input_source(Frame(sel(ps), g_ds, e_ds, sel(ss)))
        rc, T, st = H.scan_match(P.predict())
        assert rc in (0, -7), (f, rc)
        H.submap_update(T, sel(pm), sel(sm), e_ds, g_ds)
        P.accept(T)
        res.append({"pose": T, "stats": st, "snap": snapshot(H),
                    "sizes": dict(n_ground=len(ground), n_edge=len(edge), n_general=len(general), n_edge_ds=len(e_ds),
                                  n_ground_ds=len(g_ds), n_planar_scan=len(ps), n_sphere_scan=len(ss),
                                  n_planar_submap=len(pm), n_sphere_submap=len(sm))})
    H.close()
    return res


def fused(reg, scans, cfg, H=None):
    H = H or reg.HipRegistration()
    H.odometry_reset(None, cfg)
    res = []
    for f, xyz in enumerate(scans):
        rc, T, st = H.odometry_frame(xyz)
        assert rc in (0, -7), (f, rc)
        assert st["frame"] == f
        snap = snapshot(H) if f else {"targets": [H.get_target(k) for k in range(4)]}
        res.append({"pose": T, "stats": st, "snap": snap})
    return H, res


def same_stats(a, b):
    for k in ("outer_iterations", "gn_evaluations", "gn_iterations", "accepted_steps", "n_corr", "converged_early",
              "bad_weights", "gn_sweeps"):
        assert a[k] == b[k], k
    for k in ("kind_cost", "mu", "solver_cost"):
        assert np.asarray(a[k], float).tobytes() == np.asarray(b[k], float).tobytes(), k
    assert a["se3"].tobytes() == b["se3"].tobytes()


@pytest.fixture(scope="module")
def seq3():
    return G.sequence(8, seed=3)


@pytest.fixture(scope="module")
def run3(hip_module, seq3):
    H, res = fused(hip_module, seq3[0], odom_cfg(hip_module))
    H.close()
    return res


@pytest.mark.parametrize("seed", (3, 5))
def test_frame_equals_the_stage_chain(hip_module, seq3, run3, seed):
    scans = seq3[0] if seed == 3 else G.sequence(8, seed=seed)[0]
    cfg = odom_cfg(hip_module)
    if seed == 3:
        A = run3
    else:
        H, A = fused(hip_module, scans, cfg)
        H.close()
    B = chain(hip_module, scans, cfg)
    for f, (a, b) in enumerate(zip(A, B)):
        assert a["pose"].tobytes() == b["pose"].tobytes(), f
        for k in range(4):
            assert a["snap"]["targets"][k].tobytes() == b["snap"]["targets"][k].tobytes(), (f, k)
        if f == 0:
            continue
        same_stats(a["stats"]["match"], b["stats"])
        for key, v in b["sizes"].items():
            assert a["stats"][key] == v, (f, key)
        assert a["snap"]["fitness"] == b["snap"]["fitness"], f
        for k in range(4):
            for key in ("idx", "a", "b", "d", "w", "cost"):
                assert a["snap"]["corr"][k][key].tobytes() == b["snap"]["corr"][k][key].tobytes(), (f, k, key)


def test_frame_against_the_cpu_statements(hip_module, seq3, run3):
    scans = seq3[0][:4]
    fc = ob.make_feature_config(**FEATURE)
    O = ob.Oracle()
    M = ob.OracleSubmap()
    P = Predictor()
    cfg = odom_cfg(hip_module)
    H = hip_module.HipRegistration()
    H.odometry_reset(None, cfg)
    for f, xyz in enumerate(scans):
        rc, T, st = H.odometry_frame(xyz)
        assert rc == 0 and st["frame"] == f
        S = SNP.segment(xyz, first_frame=f == 0)
        assert S["status"] == 0
        ground, edge, general = xyz[S["ground"]], xyz[S["edge"]], xyz[S["general"]]
        ps, pm, ss, sm = ob.extract_planar_sphere(general, fc)
        assert (st["n_ground"], st["n_edge"], st["n_general"]) == (len(ground), len(edge), len(general)), f
        assert (st["n_planar_scan"], st["n_planar_submap"], st["n_sphere_scan"], st["n_sphere_submap"]) == \
            (len(ps), len(pm), len(ss), len(sm)), f
        if f == 0:
            M.init(general[pm], general[sm], edge, ground)
            assert np.array_equal(T, np.eye(4))
        else:
            e_ds = ob.pc_voxel_down_sample(edge, cfg.edge_down_sample)
            g_ds = ob.pc_voxel_down_sample(ground, cfg.submap.ground_down_sample)
            # the device's down-sampled clouds, bit for bit, through the public voxel call on the device's own inputs
            assert H.voxel_down_sample(edge, cfg.edge_down_sample).tobytes() == e_ds.tobytes()
            assert (st["n_edge_ds"], st["n_ground_ds"]) == (len(e_ds), len(g_ds)), f
            for k, cl in enumerate((general[ps], g_ds, e_ds, general[ss])):
                O.set_source(k, cl)
                O.set_target(k, M.get(k))
            ro, To, so = O.scan_match(P.predict())
            assert ro == 0
            assert st["match"]["n_corr"] == so["n_corr"], f
            assert st["match"]["outer_iterations"] == so["outer_iterations"], f
            dt, dr = pose_delta(T, To)
            assert dt < 1e-8 and dr < 1e-8, (f, dt, dr)
            assert T.tobytes() == run3[f]["pose"].tobytes(), f
            M.update(To, general[pm], general[sm], e_ds, g_ds)
            P.accept(T)
        for k in range(4):
            a, b = H.get_target(k), M.get(k)
            assert a.shape == b.shape, (f, k)
            assert np.abs(a - b).max() < 1e-8, (f, k)
    H.close()


def test_frame_tracks_the_generator(hip_module):
    """eight frames at 0.8 m per frame.  The first later frame is predicted with zero motion (last_pose = predicate_pose =
    init, :281-282): at 1.2 m per frame (G.sequence's step, the sequences above) the boxes' faces across the street are
    beyond the 0.5 m planar / 1.0 m edge search radii from that prediction, and the first two frames stop about 1 m short
    (measured on the MI355X: 2.1 m behind after frame 2, then the steps are followed); at 0.5-0.8 m per frame the worst
    error of both seeds is 0.067 m."""
    W = G.make_street(3)
    Ts = G.trajectory(8, step=0.8, seed=3)
    scans = [G.scan(W, T, seed=3000 + f)[0] for f, T in enumerate(Ts)]
    H, res = fused(hip_module, scans, odom_cfg(hip_module))
    H.close()
    T0inv = np.linalg.inv(Ts[0])
    worst = max(float(np.linalg.norm(r["pose"][:3, 3] - (T0inv @ Ts[f])[:3, 3])) for f, r in enumerate(res))
    print("odometry_frame: worst translation error", worst, "m over", len(res), "frames")
    assert worst < 0.15


def test_voxel_down_sample_is_the_oracle_bit_for_bit(hip_module):
    H = hip_module.HipRegistration()
    rng = np.random.default_rng(11)
    clouds = [rng.uniform(-20, 20, (5000, 3)), rng.normal(0, 3, (20000, 3))]
    dup = rng.uniform(-2, 2, (300, 3))
    clouds.append(np.concatenate([dup, dup, dup[::-1]]))                 # duplicate points
    clouds.append(np.concatenate([rng.uniform(0, 0.05, (100, 3)), rng.uniform(-5, 5, (500, 3))]))   # a voxel of 100 members
    for i, c in enumerate(clouds):
        for v in (0.1, 0.3, 1.0):
            a = H.voxel_down_sample(c, v)
            b = ob.pc_voxel_down_sample(c, v)
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (i, v)
    assert len(H.voxel_down_sample(np.zeros((0, 3)), 0.1)) == 0
    for v in (0.0, -1.0, 1e-9):
        with pytest.raises(hip_module.TloamHipError, match="TLOAM_E_INVALID"):
            H.voxel_down_sample(clouds[0], v)
    H.close()


def test_residency_contract(seq3, run3):
    scans = seq3[0]
    for f, r in enumerate(run3):
        st = r["stats"]
        assert st["h2d_bytes"] == 24 * len(scans[f]), f   # the raw scan, and nothing else
        assert st["d2h_bytes"] < 4096, f
        if f:
            assert st["host_syncs"] == 4 < CHAIN_SYNCS, f


def test_status_paths(hip_module, seq3, run3):
    scans = seq3[0]
    cfg = odom_cfg(hip_module)
    H = hip_module.HipRegistration()
    T = np.zeros(16)
    assert H.L.tloam_odometry_frame(H.h, hip_module._dp(np.ascontiguousarray(scans[0])), len(scans[0]), hip_module._dp(T),
                                    None) == -6   # before the reset: TLOAM_E_NOT_READY
    with pytest.raises(hip_module.TloamHipError, match="TLOAM_E_INVALID"):
        H.odometry_reset(None, hip_module.default_odom_config(edge_down_sample=0.0))
    with pytest.raises(hip_module.TloamHipError, match="TLOAM_E_INVALID"):
        H.odometry_reset(None, hip_module.default_odom_config(seg__sensor_model=16))
    H.odometry_reset(None, cfg)
    for f in range(2):
        rc, T, st = H.odometry_frame(scans[f])
        assert rc == 0 and np.array_equal(T, run3[f]["pose"]), f
    targets = [H.get_target(k) for k in range(4)]
    rng = np.random.default_rng(3)
    bad = [np.zeros((0, 3)), rng.uniform(-5, 5, (5000, 3)).astype(np.float32).astype(np.float64)]   # empty; no object point
    for b in bad:
        rc, T, st = H.odometry_frame(b)
        assert rc == -2 and st["frame"] == 2
        for k in range(4):
            assert H.get_target(k).tobytes() == targets[k].tobytes()
    for f in range(2, 4):   # the bad frames changed nothing: the run goes on as if they had never come
        rc, T, st = H.odometry_frame(scans[f])
        assert rc == 0 and st["frame"] == f and T.tobytes() == run3[f]["pose"].tobytes(), f
    # a reset mid-sequence: the next frame is a first frame again
    init = np.eye(4)
    init[:3, 3] = (1.0, 2.0, 0.5)
    H.odometry_reset(init, cfg)
    rc, T, st = H.odometry_frame(scans[4])
    assert rc == 0 and st["frame"] == 0 and np.array_equal(T, init)
    rc, T, st = H.odometry_frame(scans[5])
    assert rc == 0 and st["frame"] == 1
    assert np.isfinite(T).all() and not np.array_equal(T, init)
    H.close()


def test_replay_device_pipeline(hip_module, seq3, run3):
    H = hip_module.HipRegistration()
    poses, stats = replay.replay(H, seq3[0], pipeline="device", odom_cfg=odom_cfg(hip_module))
    H.close()
    assert stats["frames"] == len(run3) and stats["skipped"] == []
    for f, (a, r) in enumerate(zip(poses, run3)):
        assert a.tobytes() == r["pose"].tobytes(), f
