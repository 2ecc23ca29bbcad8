"""-m gpu: the deskew of the odometry frame -- tloam_deskew_scan against the numpy restatement
(tests/deskew_np.py) and against the generator's world hits, the fused frame with deskew on against the stage chain fed with
the correction's output (bit for bit), deskew off / no motion against a context without it (bit for bit), tracking on swept
sequences with deskew on and off, the status paths, and the maps.

Sequences: tloam_amd/synth_sweep.py, the street of synth_hdl64 swept while the sensor moves 0.8 m and turns 0.03 rad per
frame.  Feature settings as tests/test_gpu_odometry_frame.py (no round objects in the street: a wider PCA radius)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import deskew_np as D  # noqa: E402
from conftest import pose_delta  # noqa: E402
from tloam_amd import synth_hdl64 as G  # noqa: E402
from tloam_amd import synth_sweep as SW  # noqa: E402
from tloam_amd.synth import Frame, se3_exp_np  # noqa: E402

pytestmark = pytest.mark.gpu

FEATURE = dict(radius=0.5, cvr_submap=0.05)
TWIST = np.array([0.8, 0.0, 0.0, 0.0, 0.0, 0.03])
PERIOD = 0.1
INVALID = -1
# tracking (test 5; DESIGN.md 15 has the measured numbers): deskew on stays below these bars -- mean translation error, max
# translation error from frame 3 on, max rotation error -- and below deskew off by these factors
BAR_MEAN_T, BAR_MAX_T, BAR_MAX_R = 0.20, 0.30, 0.015
MARGIN_MEAN, MARGIN_MAX = 0.8, 0.85


def odom_cfg(reg):
    return reg.default_odom_config(**{f"feature__{k}": v for k, v in FEATURE.items()})


def dcfg(reg, timed=False, **over):
    return reg.default_deskew_config(enabled=1, time_source=1 if timed else 0, **over)


@pytest.fixture(scope="module")
def seq3():
    return SW.sequence(12, TWIST, seed=3)


@pytest.fixture(scope="module")
def seq5():
    return SW.sequence(12, TWIST, seed=5)


# ---- 1, 2: the correction alone -----------------------------------------------------------------------------------------
def test_deskew_scan_against_the_restatement(hip_module):
    reg = hip_module
    W = G.make_street(2)
    pose = SW.trajectory(3, TWIST)[2]
    p, _, t, _ = SW.sweep_scan(W, pose, TWIST, seed=21, nan_inf=40)
    assert len(p) > 100_000
    rng = np.random.default_rng(0)
    on_axis = rng.choice(len(p), 50, replace=False)   # azimuth 0: s == 0 in azimuth mode
    p[on_axis, 1] = 0.0
    p[on_axis, 0] = np.abs(p[on_axis, 0]) + 1.0
    zero_t = rng.choice(len(p), 300, replace=False)   # s == 0 in timed mode
    t = t.copy()
    t[zero_t] = 0.0
    M = se3_exp_np(TWIST * 1.1)
    H = reg.HipRegistration()
    try:
        for timed in (False, True):
            for direction, start, ref in ((1, 0.0, 0.0), (-1, 0.7, 0.3)) if not timed else ((1, 0.0, 0.0),):
                cfg = dcfg(reg, timed, direction=direction, start_azimuth=start, ref_fraction=ref)
                dev = H.deskew_scan(p, M, cfg, PERIOD, t if timed else None)
                ref_np = D.deskew(p, M, direction, start, ref, t if timed else None, PERIOD)
                s = D.sweep_s(p, direction, start, ref, t if timed else None, PERIOD)
                copy = ~np.isfinite(p).all(axis=1) | (s == 0.0)
                assert copy.sum() >= (300 if timed else 40)
                assert dev[copy].tobytes() == p[copy].tobytes(), (timed, direction)
                err = np.abs(dev[~copy] - ref_np[~copy]).max(axis=1) / (1.0 + np.abs(p[~copy]).max(axis=1))
                assert err.max() < 1e-12, (timed, direction, err.max())
                assert np.abs(dev[~copy] - p[~copy]).max() > 0.1
        # identity motion: the input bits, in both modes
        assert H.deskew_scan(p, np.eye(4), dcfg(reg)).tobytes() == p.tobytes()
        assert H.deskew_scan(p, np.eye(4), dcfg(reg, True), PERIOD, t).tobytes() == p.tobytes()
    finally:
        H.close()


@pytest.mark.parametrize("ref", (0.0, 0.5))
def test_deskew_scan_puts_a_swept_scan_on_the_world(hip_module, ref):
    reg = hip_module
    W = G.make_street(4)
    pose = SW.trajectory(4, TWIST)[3]
    p, _, t, hits = SW.sweep_scan(W, pose, TWIST, ref=ref, seed=5, noise=0.0)
    to_world = lambda q: q @ pose[:3, :3].T + pose[:3, 3]  # noqa: E731
    H = reg.HipRegistration()
    try:
        M = se3_exp_np(TWIST)
        for out in (H.deskew_scan(p, M, dcfg(reg, ref_fraction=ref)), H.deskew_scan(p, M, dcfg(reg, True), PERIOD, t)):
            assert np.abs(to_world(out) - hits).max() < 1e-4
        assert np.abs(to_world(p) - hits).max() > 0.1
    finally:
        H.close()


# ---- 3: the fused frame against the stage chain ---------------------------------------------------------------------------
def _mul(A, B):   # tl_api_odom.hip mat_mul
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
    """last_pose / predicate_pose / step_pose in the device's operation order"""
    def __init__(self):
        self.last = [[float(i == j) for j in range(4)] for i in range(4)]
        self.pred = [row[:] for row in self.last]
        self.step = [row[:] for row in self.last]

    def accept(self, T):
        T = [[float(v) for v in row] for row in np.asarray(T)]
        self.step = _mul(_rigid_inv(self.last), T)
        self.pred = _mul(T, self.step)
        self.last = T


def snapshot(H):
    return {"targets": [H.get_target(k) for k in range(4)], "fitness": H.fitness(),
            "corr": [H.get_correspondences(k) for k in range(4)]}


def fused(reg, scans, times=None, deskew=None, mapping=False, vmap=False):
    H = reg.HipRegistration()
    if deskew is not None:
        H.deskew_configure(deskew)
    if mapping:
        H.map_configure(reg.default_map_config(enabled=1))
    if vmap:
        H.voxel_map_configure(reg.default_voxel_map_config(enabled=1))
    H.odometry_reset(None, odom_cfg(reg))
    res = []
    for f, xyz in enumerate(scans):
        motion = H.deskew_info()["next_motion"]
        rc, T, st = H.odometry_frame(xyz, None if times is None else times[f])
        assert rc in (0, -7), (f, rc)
        res.append({"pose": T, "stats": st, "motion": motion, "info": H.deskew_info(), "reg": H.registered_scan(),
                    "snap": snapshot(H) if f else {"targets": [H.get_target(k) for k in range(4)]}})
    H.close()
    return res


def chain(reg, scans, dc, times=None):
    """the stage chain through the public calls: segmentation on the raw scan, its lists taken from tloam_deskew_scan's
    output under the frame's own step"""
    cfg = odom_cfg(reg)
    H = reg.HipRegistration()
    P = Predictor()
    res = []
    for f, raw in enumerate(scans):
        S = H.segment(raw, cfg.seg)
        assert S["status"] == 0, f
        xyz = H.deskew_scan(raw, np.array(P.step), dc, cfg.seg.scan_period, None if times is None else times[f])
        ground, edge, general = xyz[S["ground"]], xyz[S["edge"]], xyz[S["general"]]
        ps, pm, ss, sm = H.extract_planar_sphere(general, cfg.feature)
        sel = lambda idx: np.ascontiguousarray(general[idx])  # noqa: E731
        if f == 0:
            H.submap_init(sel(pm), sel(sm), edge, ground, cfg.submap)
            res.append({"pose": np.eye(4), "step": np.array(P.step), "snap": {"targets": [H.get_target(k) for k in range(4)]}})
            continue
        e_ds = H.voxel_down_sample(edge, cfg.edge_down_sample)
        g_ds = H.voxel_down_sample(ground, cfg.submap.ground_down_sample)
        H.set_input_source(Frame(sel(ps), g_ds, e_ds, sel(ss)))
        step = np.array(P.step)
        rc, T, st = H.scan_match(np.array(P.pred))
        assert rc in (0, -7), (f, rc)
        H.submap_update(T, sel(pm), sel(sm), e_ds, g_ds)
        P.accept(T)
        res.append({"pose": T, "stats": st, "step": step, "snap": snapshot(H),
                    "sizes": dict(n_ground=len(ground), n_edge=len(edge), n_general=len(general), n_edge_ds=len(e_ds),
                                  n_ground_ds=len(g_ds), n_planar_scan=len(ps), n_sphere_scan=len(ss),
                                  n_planar_submap=len(pm), n_sphere_submap=len(sm))})
    H.close()
    return res


def same_stats(a, b):
    for k in ("outer_iterations", "gn_evaluations", "gn_iterations", "accepted_steps", "n_corr", "converged_early",
              "bad_weights", "gn_sweeps"):
        assert a[k] == b[k], k
    for k in ("kind_cost", "mu", "solver_cost"):
        assert np.asarray(a[k], float).tobytes() == np.asarray(b[k], float).tobytes(), k
    assert a["se3"].tobytes() == b["se3"].tobytes()


@pytest.mark.parametrize("timed", (False, True))
def test_frame_equals_the_deskewed_stage_chain(hip_module, seq3, timed):
    reg = hip_module
    scans, times = seq3[0][:6], (seq3[1][:6] if timed else None)
    A = fused(reg, scans, times, dcfg(reg, timed))
    B = chain(reg, scans, dcfg(reg, timed), times)
    for f, (a, b) in enumerate(zip(A, B)):
        assert a["motion"].tobytes() == b["step"].tobytes(), f
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
    # frames 2.. were corrected; frames 0 and 1 had no motion
    assert [r["info"]["frames_deskewed"] for r in A] == [0, 0, 1, 2, 3, 4]
    last = A[-1]["info"]
    assert last["last_frame"] == 5 and 0.1 < last["last_max_shift"] < 5.0
    assert np.abs(last["last_twist"] - TWIST).max() < 0.05


# ---- 4: off, or no motion: bit for bit ------------------------------------------------------------------------------------
def _same_frame(a, b, f, bytes_too=True):
    assert a["pose"].tobytes() == b["pose"].tobytes(), f
    for k in range(4):
        assert a["snap"]["targets"][k].tobytes() == b["snap"]["targets"][k].tobytes(), (f, k)
    if f:
        same_stats(a["stats"]["match"], b["stats"]["match"])
        assert a["snap"]["fitness"] == b["snap"]["fitness"], f
    skip = () if bytes_too else ("h2d_bytes", "d2h_bytes")
    for key, v in a["stats"].items():
        if key != "match" and key not in skip:
            assert np.asarray(v).tobytes() == np.asarray(b["stats"][key]).tobytes(), (f, key)
    assert a["reg"].tobytes() == b["reg"].tobytes(), f


def test_deskew_off_or_without_motion_changes_nothing(hip_module, seq3):
    reg = hip_module
    scans, times = seq3[0][:4], seq3[1][:4]
    off = fused(reg, scans)
    # configured but disabled (every other field set): the frames of a context that never heard of deskew, bit for bit
    dis = fused(reg, scans, deskew=reg.default_deskew_config(enabled=0, time_source=0, direction=-1, start_azimuth=1.0,
                                                              ref_fraction=0.5))
    for f in range(4):
        _same_frame(off[f], dis[f], f)
    # on: frames 0 and 1 have no motion yet -- no correction, the same frames (timed: the times' bytes on top)
    az = fused(reg, scans[:2], deskew=dcfg(reg))
    tm = fused(reg, scans[:2], times[:2], dcfg(reg, True))
    for f in range(2):
        _same_frame(off[f], az[f], f)
        _same_frame(off[f], tm[f], f, bytes_too=False)
        assert az[f]["info"]["frames_deskewed"] == 0 and tm[f]["info"]["frames_deskewed"] == 0


def test_zero_twist_sequence_barely_moves(hip_module):
    """a sensor at rest: the frames' estimated step is not bitwise the identity, so the correction runs, but it is tiny"""
    reg = hip_module
    scans, times, poses, _ = SW.sequence(5, np.zeros(6), seed=4)
    off = fused(reg, scans)
    on = fused(reg, scans, times, dcfg(reg, True))
    for f in range(5):
        dt, dr = pose_delta(off[f]["pose"], on[f]["pose"])
        assert dt < 5e-3 and dr < 1e-3, (f, dt, dr)
    assert on[-1]["info"]["last_max_shift"] < 0.2   # (a step of ~1 mrad of noise moves a 90 m return by 0.1 m)


# ---- 5: tracking ----------------------------------------------------------------------------------------------------------
def _errors(res, poses, first=0):
    d = [pose_delta(r["pose"], T) for r, T in zip(res[first:], poses[first:])]
    dt = np.array([x[0] for x in d])
    dr = np.array([x[1] for x in d])
    return float(dt.mean()), float(dt.max()), float(dr.max())


@pytest.mark.parametrize("seed", (3, 5))
def test_deskew_tracks_a_swept_sequence(hip_module, seed):
    """the sensor stands for two frames, then moves 0.8 m and turns 0.03 rad per frame (12 frames).  Frame 2 is corrected with
    the standing frames' motion (none) in every run; from frame 3 on deskew has the motion.  (A sequence that moves from its
    first frame seeds the submap with two uncorrected scans: there deskew on tracks worse than off -- DESIGN.md 15.)"""
    reg = hip_module
    scans, times, poses, _ = SW.sequence(12, TWIST, seed=seed, rest_frames=2)
    off_res = fused(reg, scans)
    off, off3 = _errors(off_res, poses), _errors(off_res, poses, 3)
    for name, res in (("azimuth", fused(reg, scans, deskew=dcfg(reg))), ("timed", fused(reg, scans, times, dcfg(reg, True)))):
        on, on3 = _errors(res, poses), _errors(res, poses, 3)
        print(f"tracking seed {seed} {name}: mean t {on[0]:.4f} (off {off[0]:.4f}) m, max t from frame 3 {on3[1]:.4f} "
              f"(off {off3[1]:.4f}) m, max r {on[2]:.5f} (off {off[2]:.5f}) rad")
        assert on[0] < BAR_MEAN_T and on3[1] < BAR_MAX_T and on[2] < BAR_MAX_R, (seed, name, on, on3)
        assert on[0] < MARGIN_MEAN * off[0] and on3[1] < MARGIN_MAX * off3[1], (seed, name, on, off, on3, off3)


# ---- 6: status paths ------------------------------------------------------------------------------------------------------
def _raw_timed(reg, H, xyz, t):
    """the status of tloam_odometry_frame_timed (t None: a NULL pointer)"""
    a = np.ascontiguousarray(xyz, dtype=np.float64)
    T = np.zeros(16)
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    return H.L.tloam_odometry_frame_timed(H.h, dp(a), None if t is None else dp(np.ascontiguousarray(t, dtype=np.float64)),
                                          len(a), dp(T), C.byref(reg.OdomStats()))


def test_status_paths(hip_module, seq3):
    reg = hip_module
    scans, times = seq3[0][:5], seq3[1][:5]
    n = len(scans[0])
    H = reg.HipRegistration()
    try:
        L, h = H.L, H.h
        # bad configurations
        for over in (dict(direction=0), dict(direction=2), dict(time_source=2), dict(time_source=-1),
                     dict(start_azimuth=float("nan")), dict(ref_fraction=float("inf")), dict(enabled=2)):
            assert L.tloam_deskew_configure(h, C.byref(reg.default_deskew_config(**over))) == INVALID, over
        M = np.eye(4).T.copy()
        assert L.tloam_deskew_scan(h, C.byref(dcfg(reg, True)), PERIOD, M.ctypes.data_as(C.POINTER(C.c_double)),
                                   scans[0].ctypes.data_as(C.POINTER(C.c_double)), None, n,
                                   np.zeros((n, 3)).ctypes.data_as(C.POINTER(C.c_double))) == INVALID   # timed, no times
        bad_motion = se3_exp_np(TWIST)
        bad_motion[0, 0] += 1e-3
        with pytest.raises(reg.TloamHipError):
            H.deskew_scan(scans[0], bad_motion)
        t_nan = times[0].copy(); t_nan[100] = np.nan
        with pytest.raises(reg.TloamHipError):
            H.deskew_scan(scans[0], se3_exp_np(TWIST), dcfg(reg, True), PERIOD, t_nan)
        H.odometry_reset(None, odom_cfg(reg))
        # timed mode: the untimed call and the timed call without times are refused; so is the timed call in azimuth mode
        H.deskew_configure(dcfg(reg))
        assert _raw_timed(reg, H, scans[0], times[0]) == INVALID
        H.deskew_configure(dcfg(reg, True))
        with pytest.raises(reg.TloamHipError):
            H.odometry_frame(scans[0])
        assert _raw_timed(reg, H, scans[0], None) == INVALID
        for f in range(3):
            rc, _, st = H.odometry_frame(scans[f], times[f])
            assert rc in (0, -7)
            assert st["h2d_bytes"] == 32 * len(scans[f]), f
            if f:
                assert st["host_syncs"] == 4, f
        # a refused frame: a NaN time, a time beyond two sweeps (frame 3 is corrected: the check runs beside the correction)
        for bad in (np.nan, 0.25):
            t = times[3].copy(); t[1234] = bad
            assert _raw_timed(reg, H, scans[3], t) == INVALID
        assert H.deskew_info()["frames_deskewed"] == 1
        rest = [H.odometry_frame(scans[f], times[f]) for f in (3, 4)]
        assert H.deskew_info()["frames_deskewed"] == 3
    finally:
        H.close()
    # the refused frames left nothing behind: a run that never saw them
    ref = fused(reg, scans, times, dcfg(reg, True))
    for (rc, T, st), r in zip(rest, ref[3:]):
        assert T.tobytes() == r["pose"].tobytes()
        same_stats(st["match"], r["stats"]["match"])
    # azimuth mode: 24 n bytes up, 4 waits
    for f, r in enumerate(fused(reg, scans[:3], deskew=dcfg(reg))):
        assert r["stats"]["h2d_bytes"] == 24 * len(scans[f])
        assert f == 0 or r["stats"]["host_syncs"] == 4


# ---- 7: the maps ----------------------------------------------------------------------------------------------------------
def test_registered_scan_and_maps_take_the_deskewed_scan(hip_module, seq5):
    reg = hip_module
    scans, times = seq5[0][:5], seq5[1][:5]
    plain = fused(reg, scans, times, dcfg(reg, True))
    mapped = fused(reg, scans, times, dcfg(reg, True), mapping=True, vmap=True)
    H = reg.HipRegistration()
    try:
        for f, (a, b) in enumerate(zip(plain, mapped)):
            assert a["pose"].tobytes() == b["pose"].tobytes(), f
            same = H.deskew_scan(scans[f], a["motion"], dcfg(reg, True), PERIOD, times[f])
            T = a["pose"] if f else np.eye(4)
            want = same @ T[:3, :3].T + T[:3, 3]
            fin = np.isfinite(want).all(axis=1)
            for r in (a["reg"], b["reg"]):
                assert np.abs(r[fin] - want[fin]).max() < 1e-9, f
            if f >= 2:
                assert np.abs(same - scans[f]).max() > 0.1, f
    finally:
        H.close()
