"""The relocalisation's restatement (tests/closed_map_relocalise_np.py) on the static pass, without a GPU:
every query of tests/relocalise_scenes.py is found within section 23's bars of the generator's pose, the turned queries pick the
shift the turn predicts, a scan of another world and a tiny max_dist are NOT_FOUND, and the pick's ties."""
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
import place_np as PN  # noqa: E402
import relocalise_scenes as RS  # noqa: E402

BAR_T, BAR_R = 6.67e-3, 5.07e-4   # ten times the localiser's own error on this pass


@pytest.fixture(scope="module")
def scene():
    poses, clouds, scans, queries = RS.static()
    T = LS.target(poses, clouds, CS.MASK, CS.STATIC["voxel"])[4]
    rk, ds = RS.database(scans)
    return T, rk, ds, poses, queries


@pytest.mark.parametrize("name,ncand", [("as_it_is", 8), ("quarter", 3), ("half", 3), ("off_grid", 3)])
def test_every_query_is_found(scene, name, ncand):
    T, rk, ds, poses, queries = scene
    scan, truth = queries[name]
    pose, info, hyps = RN.relocalise(T, rk, ds, poses, scan, RS.PLACE, dict(num_candidates=ncand))
    err = LN.pose_error(pose, truth)
    print(name, info, err, [(H["keyframe"], H["shift"], H["localise"]["used"]) for H in hyps])
    assert info["status"] == RN.FOUND and info["n_hypotheses"] == ncand and info["keyframe"] in (3, 4)
    assert err[0] < BAR_T and err[1] < BAR_R
    assert all(H["shift"] in RS.TURNS[name][1] for H in hyps[:2]) and info["shift"] in RS.TURNS[name][1]
    assert sorted(H["keyframe"] for H in hyps[:2]) == [3, 4]          # the scan was taken midway between them
    for H in hyps:
        assert H["yaw"] == PN.yaw_of(H["shift"], 60) and not H["skipped"]
        assert np.allclose(H["prior"][:3, :3] @ H["prior"][:3, :3].T, np.eye(3), atol=1e-15)
        assert np.array_equal(H["prior"][:, 3], poses[H["keyframe"]][:, 3])


def test_the_prior_turns_with_the_sensor():
    """the sign: a keyframe at P, a sensor turned by +a about its own z stands at P Rz(a); yaw_of(shift) is +a for shift = a / w"""
    P = LS.offset(np.eye(4), 2.0, 0.3)
    for shift, a in ((15, 0.5 * np.pi), (45, -0.5 * np.pi), (4, 4 * 2.0 * np.pi / 60)):
        Q = RN.prior_of(P, PN.yaw_of(shift, 60))
        want = P.copy()
        want[:3, :3] = P[:3, :3] @ LS.rotation([0.0, 0.0, 1.0], a)
        assert np.abs(Q - want).max() < 1e-15
    # and the descriptor of a turned scan is the descriptor shifted the same way
    scan = np.random.default_rng(3).uniform(-30.0, 30.0, (4000, 3))
    quarter = np.stack([scan[:, 1], -scan[:, 0], scan[:, 2]], axis=1)
    d0, dq = PN.describe(scan)[0], PN.describe(quarter)[0]
    assert int(np.argmin(PN.shift_distances(dq, d0))) == 15


def test_another_world_is_not_found(scene):
    T, rk, ds, poses, _ = scene
    scan = RS.foreign()
    pose, info, hyps = RN.relocalise(T, rk, ds, poses, scan, RS.PLACE)
    print(info, [(H["keyframe"], H["localise"]["used"], H["localise"]["status"]) for H in hyps])
    assert pose is None and info["status"] == RN.NOT_FOUND and info["best"] == -1 and info["n_hypotheses"] == 8
    assert max(H["localise"]["used"] for H in hyps) < 0.5 * len(scan)


def test_a_tiny_max_dist_skips_every_hypothesis(scene):
    T, rk, ds, poses, queries = scene
    pose, info, hyps = RN.relocalise(T, rk, ds, poses, queries["as_it_is"][0], RS.PLACE, dict(max_dist=1e-6))
    assert pose is None and info["status"] == RN.NOT_FOUND and len(hyps) == 8
    assert all(H["skipped"] and np.array_equal(H["pose"], H["prior"]) and H["log"] == [] for H in hyps)


def test_num_candidates_clamps(scene):
    T, rk, ds, poses, queries = scene
    hyps = RN.hypotheses(rk, ds, poses, queries["as_it_is"][0], RS.PLACE, dict(num_candidates=32))
    assert sorted(H["keyframe"] for H in hyps) == list(range(8))


def test_the_pick():
    ok, deg = LN.CONVERGED, LN.DEGENERATE
    info = lambda status, used: dict(status=status, used=used, rms=0.01)   # noqa: E731
    assert RN.pick([info(ok, 10), info(ok, 12), info(ok, 11)], [1.0, 5.0, 0.1]) == 1              # the largest used
    assert RN.pick([info(ok, 12), info(ok, 12), info(ok, 12)], [2.0, 1.0, 1.0]) == 1              # then the smaller cost, then the lower index
    assert RN.pick([info(deg, 99), info(LN.MAX_ITERATIONS, 3)], [0.0, 9.0]) == 1                  # never a degenerate one
    assert RN.pick([info(deg, 99), info(deg, 3)], [0.0, 9.0]) == -1
    assert RN.pick([info(ok, 99), info(ok, 3)], [0.0, 9.0], skipped=[1, 0]) == 1                  # nor a skipped one
    assert RN.pick([], []) == -1
    assert RN.accepted(dict(used=50, rms=0.1), 100, 0.5, 0.1) and not RN.accepted(dict(used=49, rms=0.1), 100, 0.5, 0.1)
    assert not RN.accepted(dict(used=50, rms=0.2), 100, 0.5, 0.1) and RN.accepted(dict(used=0, rms=0.0), 0, 0.5, float("inf"))
