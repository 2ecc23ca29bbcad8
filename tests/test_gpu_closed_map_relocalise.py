"""-m gpu: relocalisation of a scan in the closed map without a prior (tloam_closed_map_relocalise) against
its numpy restatement (tests/closed_map_relocalise_np.py) on the static pass of tests/relocalise_scenes.py, against
closed_map_localise_batch from the priors it reports, and its lifecycle.

The pick between two hypotheses that end at the same optimum -- the keyframes on either side of the scan do, with the same
`used` -- falls to the costs, which differ in their last bits and depend on the order the sums are formed in.  The restatement
does not restate that order, so where its winner ties in `used` the device's pick is held to the rule applied to the device's own
figures and to the set of the tied hypotheses; everything else is held to the restatement's."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_localise_np as LN  # noqa: E402
import closed_map_relocalise_np as RN  # noqa: E402
import localise_scenes as LS  # noqa: E402
import relocalise_scenes as RS  # noqa: E402
import test_gpu_closed_map_localise as TL  # noqa: E402

pytestmark = pytest.mark.gpu

bits, invalid, not_ready, log_bytes = TL.bits, TL.invalid, TL.not_ready, TL.log_bytes
BAR_T, BAR_R = 6.67e-3, 5.07e-4
NCAND = 3   # of the restated runs: a restated hypothesis costs a second


def context(reg, poses, clouds, scans, place=True):
    """the static pass's keyframes with their real descriptors, the closed map not yet built"""
    H = reg.HipRegistration()
    H.place_configure(enabled=1, **RS.PLACE)
    H.loop_configure(enabled=1)
    for k in range(len(poses)):
        assert H.place_add_scan(scans[k], poses[k], k) == k
        H.place_set_keyframe_clouds(k, *clouds[k])
    H.closed_map_configure(voxel=CS.STATIC["voxel"], cloud_mask=CS.MASK)
    return H


@pytest.fixture(scope="module")
def scene(hip_module):
    poses, clouds, scans, queries = RS.static()
    H = context(hip_module, poses, clouds, scans)
    H.closed_map_build(2, poses)
    H.closed_map_surfels()
    T = LS.target(poses, clouds, CS.MASK, CS.STATIC["voxel"])[4]
    rk, ds = RS.database(scans)
    yield H, T, rk, ds, poses, queries, (clouds, scans)
    H.close()


def database_bytes(H):
    info = H.place_info()
    kf = H.place_read_keyframes()
    loops = H.place_loops()
    return repr(info).encode() + b"".join(np.asarray(kf[k]).tobytes() for k in sorted(kf)) + repr(loops).encode()


# ---- 4: against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RS.TURNS))
def test_against_the_restatement(scene, hip_module, name):
    H, T, rk, ds, poses, queries, _ = scene
    scan, truth = queries[name]
    H.closed_map_relocalise_configure(num_candidates=NCAND)
    pose, info = H.closed_map_relocalise(scan)
    hyps = H.closed_map_relocalise_hypotheses()
    logs = [H.closed_map_localise_batch_log(h) for h in range(len(hyps))]
    H.closed_map_relocalise_configure()
    wpose, winfo, whyps = RN.relocalise(T, rk, ds, poses, scan, RS.PLACE, dict(num_candidates=NCAND))
    print(name, info, [(h["keyframe"], h["shift"], h["dist"], h["localise"]["used"]) for h in hyps])
    assert [(h["keyframe"], h["shift"], h["skipped"]) for h in hyps] == [(h["keyframe"], h["shift"], h["skipped"]) for h in whyps]
    assert bits([h["dist"] for h in hyps]) == bits([h["dist"] for h in whyps])
    assert bits([h["yaw"] for h in hyps]) == bits([h["yaw"] for h in whyps])
    for h, w, log in zip(hyps, whyps, logs):
        assert np.abs(h["prior"] - w["prior"]).max() <= 1e-12
        L, W = h["localise"], w["localise"]
        assert (L["status"], L["iterations"], L["matched"], L["used"]) == (W["status"], W["iterations"], W["matched"], W["used"])
        assert [(r["matched"], r["used"]) for r in log] == [(r["matched"], r["used"]) for r in w["log"]]
        assert max(LN.pose_error(h["pose"], w["pose"])) < 1e-9 and abs(L["rms"] - W["rms"]) <= 1e-9
        assert L["launches"] == 40
    best = RN.pick([h["localise"] for h in hyps], [log[-1]["cost"] if log else 0.0 for log in logs], [h["skipped"] for h in hyps])
    assert info["best"] == best and info["status"] == winfo["status"] == hip_module.RELOCALISE_FOUND
    top = max(w["localise"]["used"] for w in whyps)
    tied = [i for i, w in enumerate(whyps) if w["localise"]["used"] == top]
    assert winfo["best"] in tied and info["best"] in tied and (len(tied) > 1 or info["best"] == winfo["best"])
    assert info["keyframe"] == hyps[best]["keyframe"] and info["shift"] == hyps[best]["shift"] == winfo["shift"]
    assert info["shift"] in RS.TURNS[name][1] and info["n_hypotheses"] == NCAND and info["launches"] == 45
    assert info["localise"] == hyps[best]["localise"] and bits(pose) == bits(hyps[best]["pose"])
    err = LN.pose_error(pose, truth)
    print(name, "error", err)
    assert err[0] < BAR_T and err[1] < BAR_R


# ---- 5: relocalise against localise_batch ------------------------------------------------------------------------------------
def test_hypotheses_are_the_batch_from_the_reported_priors(scene):
    H, T, rk, ds, poses, queries, _ = scene
    scan, _ = queries["off_grid"]
    pose, info = H.closed_map_relocalise(scan)
    hyps = H.closed_map_relocalise_hypotheses()
    logs = [log_bytes(H.closed_map_localise_batch_log(h)) for h in range(len(hyps))]
    assert info["n_hypotheses"] == len(hyps) == 8 and info["launches"] == 45
    bposes, binfos, bbest = H.closed_map_localise_batch(scan, np.array([h["prior"] for h in hyps]))
    assert bbest == info["best"]
    for h, hyp in enumerate(hyps):
        assert bits(bposes[h]) == bits(hyp["pose"]) and binfos[h] == hyp["localise"], h
        assert log_bytes(H.closed_map_localise_batch_log(h)) == logs[h], h
    # and a second call gives the same bytes
    pose2, info2 = H.closed_map_relocalise(scan)
    assert bits(pose2) == bits(pose) and info2 == info
    assert [repr(h) for h in H.closed_map_relocalise_hypotheses()] == [repr(h) for h in hyps]


# ---- 6: the database is untouched --------------------------------------------------------------------------------------------
def test_nothing_else_changes(scene):
    H, T, rk, ds, poses, queries, _ = scene
    scan, truth = queries["as_it_is"]
    prior = LS.offset(truth, *LS.STARTS[0])
    before = database_bytes(H), TL.TS.surfel_bytes(H), H.closed_map_localise(scan, prior), log_bytes(H.closed_map_localise_log())
    H.closed_map_relocalise(queries["quarter"][0])
    H.closed_map_relocalise(RS.foreign())
    assert log_bytes(H.closed_map_localise_log()) == before[3]          # the single call's log stays
    after = database_bytes(H), TL.TS.surfel_bytes(H), H.closed_map_localise(scan, prior), log_bytes(H.closed_map_localise_log())
    assert after[0] == before[0] and after[1] == before[1] and after[3] == before[3]
    assert bits(after[2][0]) == bits(before[2][0]) and after[2][1] == before[2][1]


# ---- 7: the remaining behaviours ---------------------------------------------------------------------------------------------
def test_not_found_skips_and_clamps(scene, hip_module):
    H, T, rk, ds, poses, queries, _ = scene
    reg = hip_module
    foreign = RS.foreign()
    pose, info = H.closed_map_relocalise(foreign)
    hyps = H.closed_map_relocalise_hypotheses()
    whyps = RN.hypotheses(rk, ds, poses, foreign, RS.PLACE)
    assert pose is None and (info["status"], info["best"], info["keyframe"]) == (reg.RELOCALISE_NOT_FOUND, -1, -1)
    assert [(h["keyframe"], h["shift"]) for h in hyps] == [(h["keyframe"], h["shift"]) for h in whyps]
    assert max(h["localise"]["used"] for h in hyps) < 0.5 * len(foreign)
    # the acceptance: the same scan under a ratio it passes
    H.closed_map_relocalise_configure(min_used_ratio=0.1)
    assert H.closed_map_relocalise(foreign)[1]["status"] == reg.RELOCALISE_FOUND
    H.closed_map_relocalise_configure(min_used_ratio=0.1, max_rms=1e-6)
    assert H.closed_map_relocalise(foreign)[1]["status"] == reg.RELOCALISE_NOT_FOUND
    # points that are not finite are not counted
    scan = queries["as_it_is"][0]
    holes = np.concatenate([scan, np.full((len(scan), 3), np.nan)])
    H.closed_map_relocalise_configure(min_used_ratio=0.9)
    assert H.closed_map_relocalise(holes)[1]["status"] == reg.RELOCALISE_FOUND
    # max_dist: the two keyframes beside the scan stay, the others are skipped
    H.closed_map_relocalise_configure(max_dist=0.2)
    pose, info = H.closed_map_relocalise(scan)
    hyps = H.closed_map_relocalise_hypotheses()
    assert info["status"] == reg.RELOCALISE_FOUND and [h["skipped"] for h in hyps] == [int(not h["dist"] < 0.2) for h in hyps]
    assert sorted(h["keyframe"] for h in hyps if not h["skipped"]) == [3, 4] and info["launches"] == 45
    for h, hyp in enumerate(hyps):
        if hyp["skipped"]:
            assert bits(hyp["pose"]) == bits(hyp["prior"]) and H.closed_map_localise_batch_log(h) == []
            assert hyp["localise"] == dict(status=reg.LOCALISE_DEGENERATE, iterations=0, matched=0, used=0, rms=0.0, launches=40, prepared=0)
    H.closed_map_relocalise_configure(max_dist=1e-6)
    pose, info = H.closed_map_relocalise(scan)
    assert pose is None and info["status"] == reg.RELOCALISE_NOT_FOUND and all(h["skipped"] for h in H.closed_map_relocalise_hypotheses())
    # num_candidates above K clamps
    H.closed_map_relocalise_configure(num_candidates=32)
    pose, info = H.closed_map_relocalise(scan)
    assert info["n_hypotheses"] == 8 and sorted(h["keyframe"] for h in H.closed_map_relocalise_hypotheses()) == list(range(8))
    # refused configurations leave the old one
    for bad in (dict(num_candidates=0), dict(num_candidates=33), dict(max_dist=0.0), dict(max_dist=float("nan")),
                dict(min_used_ratio=-0.1), dict(min_used_ratio=1.5), dict(min_used_ratio=float("nan")), dict(max_rms=0.0),
                dict(max_rms=float("nan"))):
        with invalid(reg):
            H.closed_map_relocalise_configure(**bad)
    assert H.closed_map_relocalise(scan)[1]["n_hypotheses"] == 8
    with invalid(reg):
        H.closed_map_relocalise(np.zeros((0, 3)))
    H.closed_map_relocalise_configure()


def test_lifecycle(scene, hip_module):
    reg = hip_module
    _, _, _, _, poses, queries, (clouds, scans) = scene
    scan = queries["as_it_is"][0]
    H = context(reg, poses[:3], clouds, scans)
    assert H.closed_map_relocalise_hypotheses() == []
    with not_ready(reg):
        H.closed_map_relocalise(scan)                      # no map
    H.closed_map_build(2, poses[:3])
    with not_ready(reg):
        H.closed_map_relocalise(scan)                      # no surfels
    H.closed_map_surfels()
    H.closed_map_relocalise_configure(num_candidates=2)
    pose, info = H.closed_map_relocalise(scan)
    assert info["n_hypotheses"] == 2 and info["launches"] == 45 and len(H.closed_map_relocalise_hypotheses()) == 2
    H.odometry_reset(None, TL.TS.TC.odom_cfg(reg))         # the keyframes and the map go, the configuration stays
    with not_ready(reg):
        H.closed_map_relocalise(scan)
    assert H.closed_map_relocalise_hypotheses() == []
    for k in range(3):
        assert H.place_add_scan(scans[k], poses[k], k) == k
        H.place_set_keyframe_clouds(k, *clouds[k])
    H.closed_map_build(2, poses[:3])
    H.closed_map_surfels()
    assert H.closed_map_relocalise(scan)[1]["n_hypotheses"] == 2
    H.place_configure(enabled=0)                           # place recognition off
    with not_ready(reg):
        H.closed_map_relocalise(scan)
    H.close()
    H = reg.HipRegistration()
    H.comm_init_callback(0, 2, lambda dev, count, stream: 0)
    for call in (H.closed_map_relocalise_configure, lambda: H.closed_map_relocalise(scan), H.closed_map_relocalise_hypotheses):
        with invalid(reg):
            call()
    H.close()
