"""The restatement of the localisation in the closed map (tests/closed_map_localise_np.py) without a GPU:
the corner, the single wall, the static pass from four starts, another summation order, and the association's edge cases
against a brute-force loop."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_localise_np as LN  # noqa: E402
import localise_scenes as LS  # noqa: E402
import voxel_map_np as VN  # noqa: E402

# The restatement's own error against the generator on the static pass (start 0, scan seed 77, orc_eig3_sym): 0.667 mm and
# 5.07e-5 rad.  The bars are ten times that; the margin is for other seeds of the scan's noise, not for the device.
OWN_ERROR = (6.67e-4, 5.07e-5)
BARS = (10.0 * OWN_ERROR[0], 10.0 * OWN_ERROR[1])


def test_the_corner():
    poses, clouds, scan, truth = LS.corner()
    V, S, normals, evals, T = LS.target(poses, clouds, CS.MASK, LS.CORNER["voxel"])
    assert int(T.eligible.sum()) == 192 and np.all(evals[T.eligible, 0] == 0.0)
    assert {tuple(n) for n in normals[T.eligible].tolist()} == {(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)}
    pose, info, log = LN.localise(T, scan, LS.offset(truth, *LS.CORNER_START))
    dt, dr = LN.pose_error(pose, truth)
    print(info, dt, dr)
    assert info["status"] == LN.CONVERGED and info["iterations"] < 10 and info["used"] == info["matched"] == len(scan)
    assert dt < 1e-9 and dr < 1e-9
    at = LN.linearise(T, scan, truth, 0.1)
    # The planes lie on grid planes and ev0 == 0, so every voxel's plane is the grid plane exactly.  The scan is taken from a
    # turned pose, so E = M p comes back with the rounding of a rotation (a few ulp of coordinates below 5 m) and the residuals
    # are that rounding, not an exact zero: the bound is 16 ulp of 5 m.  From a pose of identity rotation and dyadic
    # translation, as the keyframes', they are exactly zero.
    assert at["used"] == len(scan) and np.abs(at["residuals"]).max() < 16 * 5.0 * 2.0 ** -52
    for k, P in enumerate(poses):
        own = LN.linearise(T, np.concatenate([np.asarray(c, np.float64).reshape(-1, 3) for side in clouds[k] for c in side]), P, 0.1)
        assert own["used"] == own["matched"] > 0 and not own["residuals"].any() and own["sums"][27] == 0.0


def test_a_single_wall_is_degenerate():
    poses, clouds, scan, truth = LS.wall()
    V, S, normals, evals, T = LS.target(poses, clouds, CS.MASK, CS.GHOST["voxel"])
    assert int(T.eligible.sum()) == 144 and np.all(normals[T.eligible] == np.array([0.0, -1.0, 0.0]))
    prior = LS.offset(truth, 0.2, 0.03)
    at = LN.linearise(T, scan, prior, 1.0)
    J = np.zeros((6, 6))
    for t, (a, b) in enumerate(LN.UPPER):
        J[a, b] = J[b, a] = at["sums"][t]
    assert at["used"] > 500 and not J[[0, 2, 4]].any() and J[1, 1] == at["used"]   # columns 0, 2 and 4 of every J are zero
    pose, info, log = LN.localise(T, scan, prior)
    assert info["status"] == LN.DEGENERATE and info["iterations"] == 1 and pose.tobytes() == prior.tobytes()
    assert np.isfinite(info["rms"]) and np.isfinite(log[0]["cost"]) and not log[0]["d"].any() and np.isfinite(pose).all()
    # too few matches is the same status: a scan far from the map
    pose, info, log = LN.localise(T, scan + [0.0, 40.0, 0.0], prior)
    assert info["status"] == LN.DEGENERATE and info["matched"] == 0 and info["rms"] == 0.0 and pose.tobytes() == prior.tobytes()


@pytest.fixture(scope="module")
def static():
    poses, clouds = CS.static_pass()
    scan, truth = LS.static_scan(poses)
    V, S, normals, evals, T = LS.target(poses, clouds, CS.MASK, CS.STATIC["voxel"])
    runs = [LN.localise(T, scan, LS.offset(truth, *start)) for start in LS.STARTS]
    return T, scan, truth, runs


def test_the_static_pass_from_four_starts(static):
    T, scan, truth, runs = static
    assert len(scan) == 18988 and len(T.eligible) == 11557 and int(T.eligible.sum()) == 4069
    for start, (pose, info, log) in zip(LS.STARTS, runs):
        dt, dr = LN.pose_error(pose, truth)
        print(start, info, f"{dt:.3e} m {dr:.3e} rad")
        assert info["status"] in (LN.CONVERGED, LN.MAX_ITERATIONS) and info["used"] > 17000
        assert dt < BARS[0] and dr < BARS[1], start
    dt, dr = LN.pose_error(runs[0][0], truth)
    assert abs(dt - OWN_ERROR[0]) < 0.05 * OWN_ERROR[0] and abs(dr - OWN_ERROR[1]) < 0.05 * OWN_ERROR[1]   # the literal is the measurement


def test_another_summation_order_gives_the_same_iterations(static):
    """the scan's points permuted: the same matched and used in every iteration and the same pose within 1e-9 -- the project's bar
    for another summation order, which is what the device's block partials are"""
    T, scan, truth, runs = static
    perm = np.random.default_rng(1).permutation(len(scan))
    for start, (pose, info, log) in zip(LS.STARTS, runs):
        pose2, info2, log2 = LN.localise(T, scan[perm], LS.offset(truth, *start))
        assert (info2["status"], info2["iterations"]) == (info["status"], info["iterations"])
        assert [(r["matched"], r["used"]) for r in log2] == [(r["matched"], r["used"]) for r in log]
        dt, dr = LN.pose_error(pose, pose2)
        assert dt < 1e-9 and dr < 1e-9
    # and the exactly rounded sums (math.fsum) in place of numpy's order
    import math
    pose3, info3, log3 = LN.localise(T, scan, LS.offset(truth, *LS.STARTS[0]), sums_of=lambda t: [math.fsum(c) for c in t.T])
    assert [(r["matched"], r["used"]) for r in log3] == [(r["matched"], r["used"]) for r in runs[0][2]]
    assert max(LN.pose_error(runs[0][0], pose3)) < 1e-9


# ---- the association's edge cases ------------------------------------------------------------------------------------------
def brute(T, E):
    """the contract read literally, one point: every voxel, kept when it lies in the 27 cells; visited in (dz, dy, dx) order"""
    if not np.isfinite(E).all():
        return -1
    f = np.floor((E - T.origin) / T.voxel)
    if not (np.abs(f) < VN.LIMIT).all():
        return -1
    best, bid = np.inf, -1
    keys = {int(k): j for j, k in enumerate(T.keys)}
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                cell = f.astype(np.int64) + [dx, dy, dz]
                if not (np.abs(cell) < VN.LIMIT).all():
                    continue
                j = keys.get(int(VN.pack(cell[None])[0]), -1)
                if j < 0 or not T.eligible[j]:
                    continue
                d = E - T.c[j]
                D = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                if D < best:
                    best, bid = D, j
    return bid


def hand_map(points, ineligible=()):
    """a voxel per given point (v = 0.5), each its own centroid, every voxel eligible but those listed"""
    V = VN.VoxelMapNP(0.5)
    V.add_frame(np.asarray(points, np.float64))
    n = len(V.keys)
    S = np.zeros((n, 13), np.int64)
    S[:, 0] = 5
    evals = np.tile([0.0, 1.0, 1.0], (n, 1))
    evals[list(ineligible), 2] = 0.0
    T = LN.Target(V, S, np.tile([0.0, 0.0, 1.0], (n, 1)), evals)
    T.keys = V.keys
    return T


def test_association_edge_cases():
    edge = (VN.LIMIT - 1) * 0.5 + 0.25
    pts = [[0.25, 0.25, 0.25], [0.75, 0.25, 0.25],      # 0, 1: a tie
           [5.25, 5.25, 5.25],                            # 2: a neighbour of an empty cell
           [10.25, 10.25, 10.25], [10.75, 10.75, 10.25],  # 3 (ineligible, nearest), 4 (eligible, farther)
           [edge, 0.25, 0.25]]                            # 5: the grid's last cell
    T = hand_map(pts, ineligible=(3,))
    assert T.eligible.tolist() == [True, True, True, False, True, True]
    E = np.array([[0.5, 0.25, 0.25],                      # the same distance to 0 and 1; its own cell is 1's, 0's is visited first
                  [5.75, 5.25, 5.25],                     # its own cell is empty
                  [10.3, 10.3, 10.25],                    # nearest is 3
                  [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf],
                  [VN.LIMIT * 0.5, 0.25, 0.25],           # |i| = 2^20
                  [-VN.LIMIT * 0.5 - 0.25, 0.25, 0.25],   # beyond on the other side
                  [edge + 0.1, 0.3, 0.3],                 # the last cell: its +x neighbours are beyond the grid
                  [20.0, 20.0, 20.0]])                    # nothing near
    ids, d = LN.associate(T, E)
    assert ids.tolist() == [0, 2, 4, -1, -1, -1, -1, -1, 5, -1]
    assert ids.tolist() == [brute(T, e) for e in E]
    assert d[0].tolist() == [0.25, 0.0, 0.0] and not d[ids < 0].any()
    rng = np.random.default_rng(4)
    cloud = rng.uniform(-3.0, 3.0, (400, 3))
    T = hand_map(cloud, ineligible=range(0, 300, 3))
    E = rng.uniform(-3.5, 3.5, (300, 3))
    ids, _ = LN.associate(T, E)
    assert ids.tolist() == [brute(T, e) for e in E] and (ids >= 0).sum() > 100 and (ids < 0).sum() > 0
    L = LN.linearise(T, E, np.eye(4), 0.2)
    assert L["matched"] == int((ids >= 0).sum()) and 0 < L["used"] < L["matched"] and L["terms"].shape == (L["used"], 28)
    assert not L["residuals"][ids < 0].any()


def test_the_step_and_the_pose_arithmetic():
    rng = np.random.default_rng(2)
    A = rng.normal(size=(40, 6))
    H, g = A.T @ A, rng.normal(size=6)
    sums = np.concatenate([[H[a, b] for a, b in LN.UPPER], g, [0.0]])
    assert np.allclose(LN.solve6(sums, 1e-9), np.linalg.solve(H, -g), rtol=1e-10, atol=1e-12)
    H[:, 2] = H[2, :] = 0.0
    assert LN.solve6(np.concatenate([[H[a, b] for a, b in LN.UPPER], g, [0.0]]), 1e-9) is None
    P = LS.offset(np.eye(4), 0.7, 2.9)   # trace < 0: the other branch of the quaternion
    T = LN.pose_from_matrix(P)
    assert np.allclose(LN.pose_to_matrix(T), P, atol=1e-14)
    assert LN.pose_from_matrix(np.diag([1.0, 1.0, -1.0, 1.0])) is None and LN.pose_from_matrix(2.0 * np.eye(4)) is None
    d = [0.1, -0.2, 0.3, 0.02, 0.05, -0.04]
    from tloam_amd import registration as reg
    assert np.allclose(LN.pose_to_matrix(LN.se3_exp(d)), reg.se3_exp(d), atol=1e-14)
