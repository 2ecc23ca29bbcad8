"""-m gpu: loop verification -- the keyframe clouds the odometry frame stores against the stage chain's
lists bit for bit (and through the arena's growth); the odometry with verification on against off (everything bit-identical,
deskew off and on; the parent's getters and later frames undisturbed by a verification); a constraint against the same two
matches run through the public calls on the restated clouds; right answers on an out-and-back pass with true poses; determinism,
reset, configure, a query without clouds and refused configurations.

Sequences: synth_hdl64's full scans with the feature settings of tests/test_gpu_odometry_frame.py (odometry), and
tloam_amd/synth_revisit.py (keyframes with true poses: descriptors from the thinned scans of tests/test_gpu_place.py, clouds
from the full-density scans through the public stage calls)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import loop_np as LN  # noqa: E402
from tloam_amd import synth_hdl64 as G  # noqa: E402
from tloam_amd import synth_revisit as RV  # noqa: E402
from tloam_amd.synth import Frame  # noqa: E402

pytestmark = pytest.mark.gpu

FEATURE = dict(radius=0.5, cvr_submap=0.05)
ODOM_PLACE = dict(kf_dist=2.0, exclude_recent=2)
THIN = dict(n_az=600, rings=np.arange(0, 64, 2))
N_OUT = 16
EX = 8
SEED = 1            # (street 1: every keyframe's clouds hold >= 10 points of every kind under FEATURE)


def odom_cfg(reg):
    return reg.default_odom_config(**{f"feature__{k}": v for k, v in FEATURE.items()})


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def stage_lists(reg, scans, cfg):
    """per frame: the four source and four target clouds the stage chain hands to the match and the submap (the lists of
    tests/test_gpu_odometry_frame.py chain(); a segmentation context of its own, called frame after frame)"""
    H = reg.HipRegistration()
    out = []
    for f, xyz in enumerate(scans):
        S = H.segment(xyz, cfg.seg)
        assert S["status"] == 0, f
        ground, edge, general = xyz[S["ground"]], xyz[S["edge"]], xyz[S["general"]]
        ps, pm, ss, sm = H.extract_planar_sphere(general, cfg.feature)
        sel = lambda idx: np.ascontiguousarray(general[idx])  # noqa: E731
        if f == 0:
            z = np.zeros((0, 3))
            out.append(([z, z, z, z], [sel(pm), ground, edge, sel(sm)]))
            continue
        e_ds = H.voxel_down_sample(edge, cfg.edge_down_sample)
        g_ds = H.voxel_down_sample(ground, cfg.submap.ground_down_sample)
        out.append(([sel(ps), g_ds, e_ds, sel(ss)], [sel(pm), g_ds, e_ds, sel(sm)]))
    H.close()
    return out


def snapshot(H):
    """what the parent's getters say"""
    return {"targets": [H.get_target(k) for k in range(4)], "fitness": H.fitness(),
            "corr": [H.get_correspondences(k) for k in range(4)], "weights": [H.get_weights(k) for k in range(4)]}


def same_snapshot(a, b):
    for x, y in zip(a["targets"], b["targets"]):
        assert bits(x) == bits(y)
    assert a["fitness"][0] == b["fitness"][0] and bits(a["fitness"][1:]) == bits(b["fitness"][1:])
    for x, y in zip(a["corr"], b["corr"]):
        for k in x:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k
    for x, y in zip(a["weights"], b["weights"]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


@pytest.fixture(scope="module")
def seq():
    return G.sequence(7, seed=3)[0]


def odom_run(reg, scans, loop, deskew=False, reserve=0, hook=None):
    H = reg.HipRegistration()
    H.map_configure(reg.default_map_config(enabled=1))
    H.voxel_map_configure(reg.default_voxel_map_config(enabled=1))
    if deskew:
        H.deskew_configure(reg.default_deskew_config(enabled=1))
    H.place_configure(enabled=1, **ODOM_PLACE)
    if loop:
        H.loop_configure(enabled=1, reserve_points=reserve)
    H.odometry_reset(None, odom_cfg(reg))
    res = []
    for f, xyz in enumerate(scans):
        rc, T, st = H.odometry_frame(xyz)
        assert rc in (0, -7), (f, rc)
        res.append({"pose": T, "stats": st, "reg": H.registered_scan(), "map_info": H.map_info(), "map": H.map_read(),
                    "vinfo": H.voxel_map_info(), "vmap": H.voxel_map_read()})
        if hook:
            hook(f, H)
    return H, res


# ---- 1: the stored clouds ----------------------------------------------------------------------------------------------
def test_keyframe_clouds_are_the_stage_lists(hip_module, seq):
    reg = hip_module
    lists = stage_lists(reg, seq, odom_cfg(reg))
    stored = []
    for reserve in (0, 1000):   # the default arena, and growth from a tiny one
        H, _ = odom_run(reg, seq, True, reserve=reserve)
        frames = list(H.place_read_keyframes()["frames"])
        assert 2 < len(frames) < len(seq)
        clouds = [H.place_read_keyframe_clouds(q) for q in range(len(frames))]
        for q, f in enumerate(frames):
            src, tgt = lists[f]
            for k in range(4):
                assert bits(clouds[q][0][k]) == bits(src[k]), (reserve, q, f, "source", k)
                assert bits(clouds[q][1][k]) == bits(tgt[k]), (reserve, q, f, "target", k)
        info = H.loop_info()
        assert info["arena_points"] == sum(len(c) for q in clouds for side in q for c in side)
        if reserve:
            assert info["arena_capacity_points"] >= info["arena_points"] > reserve
        stored.append(clouds)
        H.close()


# ---- 2: undisturbed --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deskew", (False, True))
def test_odometry_with_verification_is_undisturbed(hip_module, seq, deskew):
    reg = hip_module
    seen = {}

    def verify_midway(f, H):
        if f != 4:
            return
        before = snapshot(H)
        n_kf = H.place_info()["n_keyframes"]
        assert n_kf >= 2
        H.loop_verify_pending()
        seen["pair"] = H.loop_verify_pair(n_kf - 1, 0)
        same_snapshot(snapshot(H), before)

    Hoff, off = odom_run(reg, seq, False, deskew)
    Hon, on = odom_run(reg, seq, True, deskew, hook=verify_midway)
    assert seen["pair"]["points"] > 0 or seen["pair"]["status"] != 0
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
        if f:
            assert sa["host_syncs"] == 4, f
        assert a["map_info"] == b["map_info"] and bits(a["map"]) == bits(b["map"]), f
        assert a["vinfo"] == b["vinfo"], f
        for x, y in zip(a["vmap"], b["vmap"]):
            assert x.tobytes() == y.tobytes(), f
    ka, kb = Hon.place_read_keyframes(), Hoff.place_read_keyframes()
    for k in ka:
        assert np.asarray(ka[k]).tobytes() == np.asarray(kb[k]).tobytes(), k
    assert Hon.place_loops() == Hoff.place_loops() or \
        [(L["query"], L["match"], L["shift"]) for L in Hon.place_loops()] == \
        [(L["query"], L["match"], L["shift"]) for L in Hoff.place_loops()]
    Hon.close(); Hoff.close()


# ---- 4 (and 3, 5): an out-and-back pass with true poses -----------------------------------------------------------------
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
    src, tgt = [sel(ps), g_ds, e_ds, sel(ss)], [sel(pm), g_ds, e_ds, sel(sm)]
    for c in src + tgt:
        assert len(c) >= 10
    return src, tgt


@pytest.fixture(scope="module")
def ob(hip_module):
    reg = hip_module
    thin, poses, leg = RV.out_and_back(N_OUT, seed=SEED, **THIN)
    full, poses_f, _ = RV.out_and_back(N_OUT, seed=SEED)
    assert all(bits(a) == bits(b) for a, b in zip(poses, poses_f))
    H = reg.HipRegistration()
    lists = [kf_lists(H, reg, xyz) for xyz in full]
    H.close()
    return thin, poses, leg, lists


def ob_context(reg, ob, **loop):
    thin, poses, _, lists = ob
    H = reg.HipRegistration()
    H.place_configure(enabled=1, exclude_recent=EX)
    H.loop_configure(enabled=1, **loop)
    for f, (s, T) in enumerate(zip(thin, poses)):
        assert H.place_add_scan(s, T, 100 + f) == f
        H.place_set_keyframe_clouds(f, *lists[f])
    return H


@pytest.fixture(scope="module")
def ob_run(hip_module, ob):
    H = ob_context(hip_module, ob)
    n = H.loop_verify_pending()
    loops, cons = H.place_loops(), H.loop_constraints()
    assert n == len(loops) == len(cons) > 0
    yield H, loops, cons
    H.close()


def test_true_revisits_are_accepted_and_right(ob, ob_run):
    _, poses, leg, _ = ob
    H, loops, cons = ob_run
    for L, c in zip(loops, cons):
        q, m = L["query"], L["match"]
        assert (c["query"], c["match"], c["query_frame"], c["match_frame"]) == (q, m, 100 + q, 100 + m)
        assert c["d"] == L["d"] and c["yaw"] == L["yaw"]
        truth = np.linalg.inv(poses[m]) @ poses[q]
        assert np.linalg.norm(truth[:3, 3] - c["init"][:3, 3]) > 0.5   # (the SC start: no translation)
        err = np.linalg.inv(truth) @ c["rel_pose"]
        dt = np.linalg.norm(err[:3, 3])
        da = np.arccos(np.clip((np.trace(err[:3, :3]) - 1) / 2, -1, 1))
        print(f"loop {q}->{m}: status {c['status']} accepted {c['accepted']} overlap {c['overlap']:.3f} rmse {c['rmse']:.4f} "
              f"init off {np.linalg.norm(truth[:3, 3]):.2f} m -> {dt:.4f} m {da:.5f} rad")
        assert np.linalg.norm(poses[q][:3, 3] - poses[m][:3, 3]) < 3.0   # (every record is a true revisit: test_gpu_place)
        assert c["status"] == 0 and c["accepted"], c
        assert dt <= 0.05 and da <= 0.01, (q, m, dt, da)
    assert H.loop_info()["n_accepted"] == len(cons)


def test_far_pairs_are_rejected(hip_module, ob, ob_run):
    _, poses, leg, _ = ob
    H, _, _ = ob_run
    n = 0
    for q in range(len(poses)):
        if leg[q] != 1:
            continue
        for m in range(0, q, 3):
            if np.linalg.norm(poses[q][:3, 3] - poses[m][:3, 3]) < 15.0:
                continue
            yaw = RV.relative_yaw(poses[q], poses[m])
            init = np.eye(4)
            init[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
            c = H.loop_verify_pair(q, m, init)
            assert not c["accepted"], (q, m, c["overlap"], c["rmse"])
            n += 1
    assert n >= 10
    assert H.loop_info()["n_constraints"] == len(H.place_loops())   # (pairs are not appended)


def test_one_way_verifies_nothing(hip_module, ob):
    thin, poses, leg, lists = ob
    out = [k for k in range(len(poses)) if leg[k] == 0]
    H = hip_module.HipRegistration()
    H.place_configure(enabled=1, exclude_recent=EX)
    H.loop_configure(enabled=1)
    for i, k in enumerate(out):
        H.place_add_scan(thin[k], poses[k], k)
        H.place_set_keyframe_clouds(i, *lists[k])
    assert H.loop_verify_pending() == 0 and H.loop_info()["n_constraints"] == 0
    H.close()


def test_device_equals_the_public_calls(hip_module, ob_run):
    reg = hip_module
    H, loops, cons = ob_run
    c = cons[0]
    q, m = c["query"], c["match"]
    w = reg.default_loop_config().window
    kf = H.place_read_keyframes()
    clouds = {k: H.place_read_keyframe_clouds(k) for k in set(LN.window(q, m, w)) | {q}}
    tgt = LN.assemble(q, m, w, kf["poses"], {k: v[1] for k, v in clouds.items()})
    src = clouds[q][0]
    A = reg.HipRegistration(reg.default_loop_config().coarse)
    A.set_input_source(Frame(*src))
    A.set_input_target(Frame(*tgt))
    rc1, T1, st1 = A.scan_match(c["init"])
    B = reg.HipRegistration()
    B.set_input_source(Frame(*src))
    B.set_input_target(Frame(*tgt))
    rc2, T2, st2 = B.scan_match(T1)
    A.close(); B.close()
    assert (rc1, rc2) == (0, 0) and c["status"] == 0
    assert bits(T2) == bits(c["rel_pose"])
    for got, want in ((st1, c["coarse"]), (st2, c["fine"])):
        for k in want:
            if k != "host_wait_us":
                assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    ov, rmse, inl, pts = LN.score_device_order(src, tgt, T2, reg.default_loop_config().inlier_dist)
    assert (inl, pts) == (c["inliers"], c["points"])
    assert ov == c["overlap"] and bits(rmse) == bits(c["rmse"])


# ---- 5: bookkeeping --------------------------------------------------------------------------------------------------------
def test_two_contexts_give_the_same_bits(hip_module, ob, ob_run):
    _, _, cons = ob_run
    H = ob_context(hip_module, ob)
    H.loop_verify_pending()
    again = H.loop_constraints()
    assert len(again) == len(cons)
    for a, b in zip(again, cons):
        for k in b:
            if k in ("coarse", "fine"):
                for s in b[k]:
                    if s != "host_wait_us":
                        assert np.asarray(a[k][s]).tobytes() == np.asarray(b[k][s]).tobytes(), (k, s)
            else:
                assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    H.close()


def test_reset_configure_and_missing_clouds(hip_module, ob, seq):
    reg = hip_module
    thin, poses, _, lists = ob
    H = ob_context(reg, ob)
    assert H.loop_verify_pending() > 0 and H.loop_info()["arena_points"] > 0
    H.loop_configure(enabled=1)
    info = H.loop_info()
    assert (info["n_constraints"], info["arena_points"]) == (0, 0) and H.place_info()["n_keyframes"] == 0
    # keyframes without clouds
    for f in range(2):
        H.place_add_scan(thin[f], poses[f], f)
    c = H.loop_verify_pair(1, 0)
    assert c["status"] == -6 and not c["accepted"]
    H.place_set_keyframe_clouds(1, src=lists[1][0])   # (a source, still no target on keyframe 0)
    assert H.loop_verify_pair(1, 0)["status"] == -6
    H.place_set_keyframe_clouds(0, tgt=lists[0][1])
    c = H.loop_verify_pair(1, 0)
    assert c["status"] == 0 and c["points"] == sum(len(x) for x in lists[1][0])
    # the odometry reset empties them too
    H.odometry_reset(None, odom_cfg(reg))
    H.odometry_frame(seq[0])
    H.odometry_frame(seq[1])
    H.odometry_reset(None, odom_cfg(reg))
    info = H.loop_info()
    assert (info["n_constraints"], info["arena_points"]) == (0, 0) and H.place_info()["n_keyframes"] == 0
    H.close()


def test_invalid_configurations_are_refused(hip_module):
    reg = hip_module
    H = reg.HipRegistration()
    bad = [dict(enabled=2), dict(window=-1), dict(init_mode=2), dict(inlier_dist=0.0), dict(inlier_dist=float("nan")),
           dict(min_overlap=1.5), dict(min_overlap=0.0), dict(max_rmse=-1.0), dict(max_rmse=float("inf")),
           dict(reserve_points=-1), dict(coarse__planar_dist_thres=0.0), dict(coarse__factor_num=5),
           dict(coarse__max_iterations=0)]
    for over in bad:
        with pytest.raises(reg.TloamHipError):
            H.loop_configure(reg.default_loop_config(**{"enabled": 1, **over}))
    H.loop_configure(enabled=0)
    with pytest.raises(reg.TloamHipError):   # off: no clouds, nothing to verify
        H.loop_verify_pending()
    H.close()
