"""-m gpu: place recognition -- tloam_place_describe against the numpy restatement (tests/place_np.py) bit
for bit; tloam_place_add_scan over an out-and-back pass with true poses (keyframes, loop records and read-backs against the
restatement's search, recall and correctness against the generator's truth, nothing on a one-way pass); the odometry frame with
place recognition on against off (everything else bit-identical, deskew off and on; keyframes by the policy; the database
against the restatement); reset, configure, skipped frames, determinism, growth and refused configurations.

Sequences: tloam_amd/synth_revisit.py (32 of the 64 rings, 600 azimuth steps: the descriptor has 60 sectors) and, for the
odometry, synth_hdl64's full scans with the feature settings of tests/test_gpu_odometry_frame.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "golden")]

import place_np as P  # noqa: E402
import make_seg_golden as MG  # noqa: E402
from tloam_amd import synth_hdl64 as G  # noqa: E402
from tloam_amd import synth_revisit as RV  # noqa: E402

pytestmark = pytest.mark.gpu

THIN = dict(n_az=600, rings=np.arange(0, 64, 2))
N_OUT = 16
EX = 8              # exclude_recent of the true-pose tests (a 16-keyframe leg)
FEATURE = dict(radius=0.5, cvr_submap=0.05)
ODOM_PLACE = dict(kf_dist=2.0, exclude_recent=2)   # the odometry tests: every other frame of a 1.2 m step, searched from kf 2
SECTOR = 2 * np.pi / 60


def odom_cfg(reg):
    return reg.default_odom_config(**{f"feature__{k}": v for k, v in FEATURE.items()})


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


@pytest.fixture(scope="module")
def ob():
    scans, poses, leg = RV.out_and_back(N_OUT, seed=0, **THIN)
    for s in scans:
        assert len(P.margins(s)) == 0
    return scans, poses, leg


def add_all(reg, scans, poses, **over):
    H = reg.HipRegistration()
    H.place_configure(enabled=1, **over)
    ids = [H.place_add_scan(s, T, 100 + f) for f, (s, T) in enumerate(zip(scans, poses))]
    assert ids == list(range(len(scans)))
    return H


def restated(scans, poses, **over):
    db = P.PlaceDB(**over)
    for f, (s, T) in enumerate(zip(scans, poses)):
        db.add(s, T, 100 + f)
    return db


def same_database(H, db):
    kf = H.place_read_keyframes()
    n = len(db.desc)
    assert H.place_info()["n_keyframes"] == n
    assert list(kf["frames"]) == db.frames
    assert bits(kf["poses"]) == bits(np.array(db.poses))
    assert bits(kf["descriptors"]) == bits(np.array(db.desc))
    assert bits(kf["ring_keys"]) == bits(np.array(db.rkey))
    assert bits(kf["sector_keys"]) == bits(np.array(db.skey))
    loops = H.place_loops()
    assert H.place_info()["n_loops"] == len(db.loops)
    assert len(loops) == len(db.loops)
    for a, b in zip(loops, db.loops):
        assert {k: a[k] for k in ("query", "query_frame", "match", "match_frame", "shift")} == \
            {k: b[k] for k in ("query", "query_frame", "match", "match_frame", "shift")}
        assert bits(a["d"]) == bits(b["d"]) and bits(a["yaw"]) == bits(b["yaw"])
    return kf, loops


# ---- 1: the descriptor ---------------------------------------------------------------------------------------------------
def test_describe_equals_the_restatement(hip_module):
    reg = hip_module
    H = reg.HipRegistration()
    scans = [MG.golden_scan(seed) for seed in MG.SEEDS]
    dirty = scans[0].copy()
    rng = np.random.default_rng(5)
    idx = rng.choice(len(dirty), 60, replace=False)
    dirty[idx[:20], 0] = np.nan
    dirty[idx[20:40], 1] = np.inf
    dirty[idx[40:], 2] = -np.inf
    far = scans[1].copy()
    far[:, :2] *= 1000.0   # every return beyond max_radius
    cases = scans + [dirty, np.zeros((0, 3)), far]
    for k, xyz in enumerate(cases):
        assert len(P.margins(xyz)) == 0, k
        d, rk, sk = H.place_describe(xyz, reg.default_place_config())
        wd, wrk, wsk = P.describe(xyz)
        assert bits(d) == bits(wd) and bits(rk) == bits(wrk) and bits(sk) == bits(wsk), k
    assert not np.any(H.place_describe(far, reg.default_place_config())[0])
    # another grid and a negative offset (negative maxima stay negative): the context's default path, then cfg=None
    over = dict(n_rings=7, n_sectors=37, max_radius=50.0, height_offset=-1.5)
    cfg = reg.default_place_config(enabled=1, **over)
    d, rk, sk = H.place_describe(scans[2], cfg)
    assert len(P.margins(scans[2], **over)) == 0
    wd, wrk, wsk = P.describe(scans[2], **over)
    assert (wd < 0).any() and bits(d) == bits(wd) and bits(rk) == bits(wrk) and bits(sk) == bits(wsk)
    H.place_configure(cfg)
    d2, _, _ = H.place_describe(scans[2])
    assert bits(d2) == bits(wd)
    assert H.place_info()["n_keyframes"] == 0   # describe touches no database
    H.close()


# ---- 2: add_scan over an out-and-back pass with true poses ---------------------------------------------------------------
@pytest.fixture(scope="module")
def ob_run(hip_module, ob):
    scans, poses, _ = ob
    H = add_all(hip_module, scans, poses, exclude_recent=EX)
    db = restated(scans, poses, exclude_recent=EX)
    kf, loops = same_database(H, db)
    H.close()
    return db, kf, loops


def test_add_scan_equals_the_restatement(ob_run):
    db, _, loops = ob_run
    assert len(loops) > 0
    print("loops:", [(L["query"], L["match"], L["shift"], round(L["d"], 4)) for L in loops])


def test_revisits_are_found_and_right(ob, ob_run):
    scans, poses, leg = ob
    db, _, loops = ob_run
    by_query = {L["query"]: L for L in loops}
    revisits = [q for q in range(len(poses)) if leg[q] == 1 and
                any(np.linalg.norm(poses[q][:3, 3] - poses[k][:3, 3]) < 3.0 for k in range(q - EX + 1))]
    assert len(revisits) >= 10
    found = [q for q in revisits if q in by_query]
    recall = len(found) / len(revisits)
    print(f"recall {len(found)}/{len(revisits)} = {recall:.3f}; best d of the revisits:",
          [round(by_query[q]["d"], 3) for q in found])
    assert recall >= 0.9
    for L in loops:   # every loop is right: place and heading
        q, m = L["query"], L["match"]
        assert np.linalg.norm(poses[q][:3, 3] - poses[m][:3, 3]) < 3.0, L
        assert abs(wrap(L["yaw"] - RV.relative_yaw(poses[q], poses[m]))) <= SECTOR, L
        assert abs(abs(L["yaw"]) - np.pi) < 0.2   # (a U-turn)


def test_one_way_reports_no_loop(hip_module, ob):
    scans, poses, leg = ob
    out = [k for k in range(len(poses)) if leg[k] == 0]   # the outbound leg alone is a one-way pass
    ow_poses = RV.one_way_poses(len(out), seed=0)
    assert all(bits(ow_poses[k]) == bits(poses[k]) for k in out)
    H = add_all(hip_module, [scans[k] for k in out], ow_poses, exclude_recent=EX)
    info = H.place_info()
    assert info["n_keyframes"] == len(out) and info["n_loops"] == 0
    H.close()


# ---- 3: the odometry frame with place recognition on against off ---------------------------------------------------------
@pytest.fixture(scope="module")
def seq():
    return G.sequence(7, seed=3)[0]


def odom_run(reg, scans, place, deskew):
    H = reg.HipRegistration()
    H.map_configure(reg.default_map_config(enabled=1))
    H.voxel_map_configure(reg.default_voxel_map_config(enabled=1))
    if deskew:
        H.deskew_configure(reg.default_deskew_config(enabled=1))
    if place:
        H.place_configure(enabled=1, **ODOM_PLACE)
    H.odometry_reset(None, odom_cfg(reg))
    res = []
    for f, xyz in enumerate(scans):
        motion = H.deskew_info()["next_motion"]
        rc, T, st = H.odometry_frame(xyz)
        assert rc in (0, -7), (f, rc)
        info = H.map_info()
        res.append({"pose": T, "stats": st, "reg": H.registered_scan(), "motion": motion, "map_info": info,
                    "map": H.map_read(), "vinfo": H.voxel_map_info(), "vmap": H.voxel_map_read()})
    return H, res


@pytest.mark.parametrize("deskew", (False, True))
def test_odometry_with_place_recognition_is_undisturbed(hip_module, seq, deskew):
    reg = hip_module
    Hoff, off = odom_run(reg, seq, False, deskew)
    Hon, on = odom_run(reg, seq, True, deskew)
    for f, (a, b) in enumerate(zip(on, off)):
        assert bits(a["pose"]) == bits(b["pose"]), f
        assert bits(a["reg"]) == bits(b["reg"]), f
        sa, sb = a["stats"], b["stats"]
        for key in sb:
            if key != "match":
                assert sa[key] == sb[key], (f, key)
        for key, v in sb["match"].items():
            if key != "host_wait_us":   # (a time)
                assert np.asarray(sa["match"][key]).tobytes() == np.asarray(v).tobytes(), (f, key)
        if f:
            assert sa["host_syncs"] == 4, f
        assert a["map_info"] == b["map_info"] and bits(a["map"]) == bits(b["map"]), f
        assert a["vinfo"] == b["vinfo"], f
        for x, y in zip(a["vmap"], b["vmap"]):
            assert x.tobytes() == y.tobytes(), f
    # the keyframes: the policy on the returned poses, described from the scan each frame used
    used = seq
    if deskew:
        Hd = reg.HipRegistration()
        used = [Hd.deskew_scan(xyz, r["motion"]) for xyz, r in zip(seq, on)]
        Hd.close()
        assert any(bits(u) != bits(x) for u, x in zip(used, seq))
    db = P.PlaceDB(**ODOM_PLACE)
    chosen = [f for f, (xyz, r) in enumerate(zip(used, on)) if db.frame(xyz, r["pose"], r["stats"]["frame"])]
    assert 2 < len(chosen) < len(seq)   # (the policy skips some)
    assert list(Hon.place_read_keyframes()["frames"]) == chosen
    same_database(Hon, db)
    print("keyframes", chosen, "loops", Hon.place_loops())
    assert Hoff.place_info()["n_keyframes"] == 0
    Hon.close(); Hoff.close()


# ---- 4: reset, configure, skipped frames, determinism, growth, refused configurations ------------------------------------
def test_reset_configure_and_skipped_frames(hip_module, seq):
    reg = hip_module
    H = reg.HipRegistration()
    H.place_configure(enabled=1, **ODOM_PLACE)
    H.odometry_reset(None, odom_cfg(reg))
    assert H.odometry_frame(np.zeros((0, 3)))[0] == -2   # skipped: nothing added, not even the first keyframe
    assert H.odometry_frame(seq[0][:5])[0] == -2
    assert H.place_info()["n_keyframes"] == 0
    assert H.odometry_frame(seq[0])[0] == 0
    info = H.place_info()
    assert info["n_keyframes"] == 1 and info["last_keyframe_frame"] == 0
    assert H.odometry_frame(np.zeros((0, 3)))[0] == -2
    assert H.place_info() == info
    H.odometry_reset(None, odom_cfg(reg))   # empties the database; the configuration stays
    assert H.place_info()["n_keyframes"] == 0 and H.place_info()["last_keyframe_frame"] == -1
    assert H.odometry_frame(seq[0])[0] == 0
    assert H.place_info()["n_keyframes"] == 1
    H.place_configure(enabled=1, **ODOM_PLACE)   # so does configure
    assert H.place_info()["n_keyframes"] == 0 and H.place_info()["n_loops"] == 0
    H.place_configure(enabled=0)
    assert H.odometry_frame(seq[1])[0] in (0, -7)
    assert H.place_info()["n_keyframes"] == 0
    with pytest.raises(reg.TloamHipError):
        H.place_add_scan(seq[1], np.eye(4))   # off: refused
    H.close()


def test_runs_contexts_and_growth_give_the_same_bits(hip_module, ob, ob_run):
    reg = hip_module
    scans, poses, _ = ob
    db, kf, loops = ob_run
    m = 20
    want_loops = [L for L in loops if L["query"] < m]
    H = add_all(reg, scans[:m], poses[:m], exclude_recent=EX, reserve_keyframes=3)   # grows 3 -> 6 -> 12 -> 24
    for run in range(2):
        info = H.place_info()
        assert info["n_keyframes"] == m and info["capacity_keyframes"] >= m
        got = H.place_read_keyframes()
        for k in ("frames", "poses", "descriptors", "ring_keys", "sector_keys"):
            assert got[k].tobytes() == kf[k][:m].tobytes(), (run, k)
        got_loops = H.place_loops()
        assert [(a["query"], a["match"], a["shift"], bits(a["d"])) for a in got_loops] == \
            [(a["query"], a["match"], a["shift"], bits(a["d"])) for a in want_loops], run
        part = H.place_read_keyframes(5, 3)
        assert part["descriptors"].tobytes() == kf["descriptors"][5:8].tobytes()
        if run == 0:   # the same context again, from an emptied database
            H.place_configure(enabled=1, exclude_recent=EX, reserve_keyframes=3)
            for f in range(m):
                H.place_add_scan(scans[f], poses[f], 100 + f)
    H.close()


INVALID = [dict(enabled=2), dict(n_rings=0), dict(n_rings=65), dict(n_sectors=1), dict(n_sectors=361), dict(num_candidates=0),
           dict(num_candidates=33), dict(exclude_recent=0), dict(max_radius=0.0), dict(max_radius=-1.0),
           dict(max_radius=float("inf")), dict(max_radius=float("nan")), dict(height_offset=float("nan")),
           dict(height_offset=float("inf")), dict(kf_dist=0.0), dict(kf_dist=float("nan")), dict(kf_angle=-0.1),
           dict(kf_angle=float("inf")), dict(dist_thres=0.0), dict(dist_thres=float("nan")), dict(reserve_keyframes=-1)]


def test_invalid_configurations_are_refused(hip_module, ob):
    reg = hip_module
    H = reg.HipRegistration()
    L = H.L
    H.place_configure(enabled=1)
    H.place_add_scan(ob[0][0], ob[1][0], 7)
    before = H.place_info()
    for over in INVALID:
        cfg = reg.default_place_config(**over)
        assert L.tloam_place_configure(H.h, C.byref(cfg)) == -1, over
    assert H.place_info() == before   # a refused configuration changes nothing
    bad = np.eye(4); bad[0, 3] = np.nan
    with pytest.raises(reg.TloamHipError):
        H.place_add_scan(ob[0][0], bad)
    with pytest.raises(reg.TloamHipError):
        H.place_read_keyframes(0, 2)   # one keyframe
    with pytest.raises(reg.TloamHipError):
        H.place_loops(0, 1)            # no loop
    H.close()
