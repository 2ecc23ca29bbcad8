"""-m gpu: localisation of a scan in the closed map (tl_localise.hip, tl_api_localise.hip) against its numpy
restatement (tests/closed_map_localise_np.py): ids, residuals and counts bit for bit, the sums within the bound of another
summation order, the iteration's counts, status and pose.  Keyframes are hand-made as in tests/test_gpu_closed_map_surfel.py."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_localise_np as LN  # noqa: E402
import closed_map_surfel_np as SN  # noqa: E402
import localise_scenes as LS  # noqa: E402
import test_gpu_closed_map_surfel as TS  # noqa: E402

pytestmark = pytest.mark.gpu

bits, invalid, not_ready, built, context, DUMMY = TS.bits, TS.invalid, TS.not_ready, TS.built, TS.context, TS.DUMMY
U = 2.0 ** -53


def surfeled(reg, poses, clouds, mask, voxel, origin=(0.0, 0.0, 0.0), min_points=5, min_planarity=0.05, **kw):
    """a context with the closed map built and its surfels gathered, and the restatement's view of them"""
    H, V = built(reg, poses, clouds, mask, voxel, origin, **kw)
    H.closed_map_surfel_configure(min_points=min_points)
    H.closed_map_localise_configure(min_planarity=min_planarity)
    H.closed_map_surfels()
    S, normals, evals, _ = SN.surfels(V, poses, clouds, mask, min_points)
    return H, LN.Target(V, S, normals, evals, min_points, min_planarity=min_planarity)


def check_linearise(H, T, pts, pose, tau):
    got, want = H.closed_map_linearise(pts, pose, tau), LN.linearise(T, pts, pose, tau)
    assert np.array_equal(got["ids"], want["ids"])
    assert bits(got["residuals"]) == bits(want["residuals"])
    assert (got["matched"], got["used"]) == (want["matched"], want["used"])
    terms = want["terms"]
    m = len(terms)
    have = np.concatenate([got["H"], got["g"], [got["cost"]]])
    exact = np.array([math.fsum(c) for c in terms.T])
    bound = m * U * np.array([math.fsum(np.abs(c)) for c in terms.T])   # any order of m terms: derived, not measured
    worst = float(np.max(np.abs(have - exact) / np.maximum(bound, 1e-300))) if m else 0.0
    print(f"n {len(pts)} tau {tau}: matched {got['matched']} used {got['used']} worst |sum - fsum| / bound {worst:.3g}")
    assert np.all(np.abs(have - exact) <= bound)
    return got


def log_bytes(log):
    return b"".join(bits(r["pose"]) + bits([r["tau"], r["cost"]]) + bits(r["d"]) + bytes([r["matched"] % 251, r["used"] % 251]) +
                    str((r["matched"], r["used"])).encode() for r in log)


def check_localise(H, T, pts, prior, want=None):
    pose, info = H.closed_map_localise(pts, prior)
    log = H.closed_map_localise_log()
    wpose, winfo, wlog = want if want is not None else LN.localise(T, pts, prior)
    print(info, LN.pose_error(pose, wpose))
    assert (info["status"], info["iterations"]) == (winfo["status"], winfo["iterations"]) and len(log) == len(wlog)
    assert [(r["matched"], r["used"]) for r in log] == [(r["matched"], r["used"]) for r in wlog]
    assert (info["matched"], info["used"]) == (winfo["matched"], winfo["used"]) and abs(info["rms"] - winfo["rms"]) <= 1e-9
    assert bits([r["tau"] for r in log]) == bits([r["tau"] for r in wlog]) and bits(log[0]["pose"]) == bits(wlog[0]["pose"])
    assert max(LN.pose_error(pose, wpose)) < 1e-9
    return pose, info, log


# ---- the scenes, built once --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corner(hip_module):
    poses, clouds, scan, truth = LS.corner()
    H, T = surfeled(hip_module, poses, clouds, CS.MASK, LS.CORNER["voxel"])
    yield H, T, scan, truth
    H.close()


@pytest.fixture(scope="module")
def wall(hip_module):
    poses, clouds, scan, truth = LS.wall()
    H, T = surfeled(hip_module, poses, clouds, CS.MASK, CS.GHOST["voxel"])
    yield H, T, scan, truth
    H.close()


@pytest.fixture(scope="module")
def static(hip_module):
    poses, clouds = CS.static_pass()
    scan, truth = LS.static_scan(poses)
    H, T = surfeled(hip_module, poses, clouds, CS.MASK, CS.STATIC["voxel"])
    runs = [LN.localise(T, scan, LS.offset(truth, *start)) for start in LS.STARTS]
    yield H, T, scan, truth, runs, (poses, clouds)
    H.close()


# ---- 1: one sweep ------------------------------------------------------------------------------------------------------------
def test_linearise_on_the_corner_and_the_wall(corner, wall):
    H, T, scan, truth = corner
    prior = LS.offset(truth, *LS.CORNER_START)
    final = LN.localise(T, scan, prior)[0]
    assert check_linearise(H, T, scan, prior, 1.0)["used"] > 1000
    assert check_linearise(H, T, scan, final, 0.1)["used"] == len(scan)
    H, T, scan, truth = wall
    prior = LS.offset(truth, 0.2, 0.03)
    got = check_linearise(H, T, scan, prior, 1.0)
    assert got["used"] > 500 and not got["H"][[0, 1, 2, 3, 4, 5, 11, 12, 13, 14, 18, 19]].any() and not got["g"][[0, 2, 4]].any()
    check_linearise(H, T, scan, truth, 0.1)


def test_linearise_on_the_static_pass(static):
    H, T, scan, truth, runs, _ = static
    got = check_linearise(H, T, scan, LS.offset(truth, *LS.STARTS[0]), 1.0)
    assert got["matched"] > 17000 and (got["ids"] < 0).sum() > 0
    check_linearise(H, T, scan, runs[0][0], 0.1)
    check_linearise(H, T, scan, truth, float("inf"))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_block_boundaries(static, n):
    H, T, scan, truth, _, _ = static
    pts = scan[5000:5000 + n]
    got = check_linearise(H, T, pts, LS.offset(truth, 0.1, 0.01), 0.5)
    assert got["matched"] <= n and (n < 63 or got["used"] > 0.5 * n)


def test_a_scan_that_matches_nothing(static, hip_module):
    H, T, scan, truth, _, _ = static
    far = scan[:300] + [0.0, 0.0, 500.0]
    got = check_linearise(H, T, far, truth, 1.0)
    assert got["matched"] == 0 and not got["H"].any() and not got["g"].any() and got["cost"] == 0.0 and (got["ids"] == -1).all()
    pose, info, log = check_localise(H, T, far, truth)
    assert info["status"] == hip_module.LOCALISE_DEGENERATE and info["rms"] == 0.0 and bits(pose) == bits(truth)
    bad = scan[:200].copy()
    bad[::7] = np.nan
    bad[3] = [np.inf, 0.0, 0.0]
    bad[4] = [2.0 ** 19 + 5.0, 0.0, 0.0]   # |i| >= 2^20 at v = 0.5
    got = check_linearise(H, T, bad, truth, 1.0)
    assert (got["ids"][::7] == -1).all() and got["ids"][3] == got["ids"][4] == -1 and got["matched"] > 100


# ---- 2: the iteration --------------------------------------------------------------------------------------------------------
def test_localise_on_the_corner(corner, hip_module):
    H, T, scan, truth = corner
    prior = LS.offset(truth, *LS.CORNER_START)
    pose, info, log = check_localise(H, T, scan, prior)
    assert info["status"] == hip_module.LOCALISE_CONVERGED and max(LN.pose_error(pose, truth)) < 1e-9
    again = H.closed_map_localise(scan, prior)
    assert bits(again[0]) == bits(pose) and {**again[1], "prepared": 0} == {**info, "prepared": 0} and log_bytes(H.closed_map_localise_log()) == log_bytes(log)


@pytest.mark.parametrize("start", range(len(LS.STARTS)))
def test_localise_on_the_static_pass(static, start):
    H, T, scan, truth, runs, _ = static
    pose, info, log = check_localise(H, T, scan, LS.offset(truth, *LS.STARTS[start]), want=runs[start])
    assert max(LN.pose_error(pose, truth)) < 1e-2 and info["launches"] == 40


def test_calls_and_contexts_give_the_same_bytes(static, hip_module):
    H, T, scan, truth, runs, (poses, clouds) = static
    prior = LS.offset(truth, *LS.STARTS[1])
    pose, info = H.closed_map_localise(scan, prior)
    log = log_bytes(H.closed_map_localise_log())
    lin = H.closed_map_linearise(scan, prior, 1.0)
    pose2, info2 = H.closed_map_localise(scan, prior)
    assert bits(pose2) == bits(pose) and info2 == info and log_bytes(H.closed_map_localise_log()) == log
    other, _ = surfeled(hip_module, poses, clouds, CS.MASK, CS.STATIC["voxel"], reserve_voxels=64)
    pose3, info3 = other.closed_map_localise(scan, prior)
    assert info3["prepared"] == 1 and {**info3, "prepared": 0} == {**info, "prepared": 0}
    assert bits(pose3) == bits(pose) and log_bytes(other.closed_map_localise_log()) == log
    lin3 = other.closed_map_linearise(scan, prior, 1.0)
    assert all(np.asarray(lin3[k]).tobytes() == np.asarray(lin[k]).tobytes() for k in lin)
    # a carve or a surfel pass before or after changes nothing, and a localise call changes nothing of theirs
    surfels = TS.surfel_bytes(other)
    other.closed_map_carve_configure(max_range=CS.STATIC["max_range"])
    other.closed_map_carve()
    misses = other.closed_map_misses().tobytes()
    pose4, info4 = other.closed_map_localise(scan, prior)
    assert info4["prepared"] == 0 and bits(pose4) == bits(pose) and log_bytes(other.closed_map_localise_log()) == log
    assert other.closed_map_misses().tobytes() == misses and TS.surfel_bytes(other) == surfels
    other.closed_map_surfels()
    pose5, info5 = other.closed_map_localise(scan, prior)
    assert info5["prepared"] == 1 and bits(pose5) == bits(pose) and log_bytes(other.closed_map_localise_log()) == log
    assert TS.surfel_bytes(other) == surfels
    other.close()


def test_the_ghost_wall(wall, hip_module):
    H, T, scan, truth = wall
    prior = LS.offset(truth, 0.2, 0.03)
    pose, info, log = check_localise(H, T, scan, prior)
    assert info["status"] == hip_module.LOCALISE_DEGENERATE and info["iterations"] == 1 and bits(pose) == bits(prior)
    assert np.isfinite(info["rms"]) and not log[0]["d"].any() and np.isfinite(log[0]["cost"])


# ---- 3: lifecycle ------------------------------------------------------------------------------------------------------------
def test_lifecycle(hip_module):
    reg = hip_module
    poses, clouds, scan, truth = LS.corner()
    v = LS.CORNER["voxel"]
    prior = LS.offset(truth, *LS.CORNER_START)
    H = context(reg, poses, clouds, voxel=v, cloud_mask=CS.MASK)
    for call in (lambda: H.closed_map_localise(scan, prior), lambda: H.closed_map_linearise(scan, prior, 1.0)):
        with not_ready(reg):
            call()                                   # before a build
    H.closed_map_build(2, poses)
    with not_ready(reg):
        H.closed_map_localise(scan, prior)           # before surfels
    assert H.closed_map_localise_log() == []
    H.closed_map_surfels()
    pose, info = H.closed_map_localise(scan, prior)
    log = log_bytes(H.closed_map_localise_log())
    assert info["prepared"] == 1 and info["launches"] == 40 and info["status"] == reg.LOCALISE_CONVERGED
    # refused calls leave everything as it was
    with invalid(reg):
        H.closed_map_localise(scan, 2.0 * np.eye(4))
    with invalid(reg):
        H.closed_map_localise(scan, np.full((4, 4), np.nan))
    with invalid(reg):
        H.closed_map_localise(np.zeros((0, 3)), prior)
    with invalid(reg):
        H.closed_map_linearise(scan, prior, -1.0)
    with invalid(reg):
        H.closed_map_linearise(scan, prior, float("nan"))
    for bad in (dict(max_iterations=0), dict(max_iterations=65), dict(shrink=0.0), dict(shrink=1.5), dict(max_residual0=0.0),
                dict(min_residual=-1.0), dict(max_sigma=float("nan")), dict(min_planarity=float("inf")), dict(step_tol_t=-1e-9),
                dict(step_tol_r=float("nan")), dict(min_pivot_ratio=1.0), dict(min_matches=0)):
        with invalid(reg):
            H.closed_map_localise_configure(**bad)
    assert log_bytes(H.closed_map_localise_log()) == log
    again, info2 = H.closed_map_localise(scan, prior)
    assert info2 == {**info, "prepared": 0} and bits(again) == bits(pose)       # the old configuration and the cached records
    # launches: the same for every input with the same max_iterations
    H.closed_map_localise_configure(max_iterations=7)
    seen = {H.closed_map_localise(p, q)[1]["launches"] for p, q in ((scan, prior), (scan[:10], prior), (scan + 100.0, truth))}
    assert seen == {14}
    assert H.closed_map_localise(scan, prior)[1]["status"] in (reg.LOCALISE_CONVERGED, reg.LOCALISE_MAX_ITERATIONS)
    H.closed_map_localise_configure(max_iterations=2)
    two, info3 = H.closed_map_localise(scan, prior)
    assert info3["status"] == reg.LOCALISE_MAX_ITERATIONS and info3["iterations"] == 2 and len(H.closed_map_localise_log()) == 2
    H.closed_map_localise_configure()
    # the gate's fields rebuild the records; the others do not
    ids = H.closed_map_linearise(scan, prior, 1.0)["ids"]
    H.closed_map_localise_configure(min_planarity=0.5)
    assert H.closed_map_localise(scan, prior)[1]["prepared"] == 1
    assert not np.array_equal(H.closed_map_linearise(scan, prior, 1.0)["ids"], ids)   # the elongated voxels are no candidates now
    H.closed_map_localise_configure(min_planarity=0.5, shrink=0.5)
    assert H.closed_map_localise(scan, prior)[1]["prepared"] == 0
    H.closed_map_localise_configure()
    assert H.closed_map_localise(scan, prior)[1]["prepared"] == 1
    # a surfel configuration drops the surfels and the records with them; a rebuild too; the result is a fresh context's
    H.closed_map_surfel_configure(min_points=7)
    with not_ready(reg):
        H.closed_map_localise(scan, prior)
    assert H.closed_map_localise_log() == []
    H.closed_map_surfels()
    p7, i7 = H.closed_map_localise(scan, prior)
    fresh = context(reg, poses, clouds, voxel=v, cloud_mask=CS.MASK)
    fresh.closed_map_surfel_configure(min_points=7)
    fresh.closed_map_build(2, poses)
    fresh.closed_map_surfels()
    f7, j7 = fresh.closed_map_localise(scan, prior)
    assert i7["prepared"] == 1 and i7 == j7 and bits(p7) == bits(f7)
    assert log_bytes(H.closed_map_localise_log()) == log_bytes(fresh.closed_map_localise_log())
    moved = poses.copy()
    moved[:, 0, 3] += 0.5
    H.closed_map_build(2, moved)                     # a rebuild: another map
    with not_ready(reg):
        H.closed_map_localise(scan, prior)
    H.closed_map_surfels()
    fresh.closed_map_build(2, moved)
    fresh.closed_map_surfels()
    a, b = H.closed_map_localise(scan, prior), fresh.closed_map_localise(scan, prior)
    assert a[1]["prepared"] == 1 and a[1] == b[1] and bits(a[0]) == bits(b[0])
    # the configuration persists across a reset
    H.closed_map_localise_configure(max_iterations=3)
    H.odometry_reset(None, TS.TC.odom_cfg(reg))
    for k in range(2):
        assert H.place_add_scan(DUMMY, np.eye(4), k) == k
        H.place_set_keyframe_clouds(k, *clouds[k])
    H.closed_map_build(2, poses)
    H.closed_map_surfels()
    assert H.closed_map_localise(scan, prior)[1]["launches"] == 6
    H.close(); fresh.close()
    # nranks > 1: every localisation call is refused
    H = reg.HipRegistration()
    H.comm_init_callback(0, 2, lambda dev, count, stream: 0)
    for call in (H.closed_map_localise_configure, lambda: H.closed_map_localise(scan, prior), H.closed_map_localise_log,
                 lambda: H.closed_map_linearise(scan, prior, 1.0)):
        with invalid(reg):
            call()
    H.close()


# ---- 4: the adversarial grid -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("voxel,origin", [(1.0, (1.0, -2.0, 0.5)), (0.3, (-0.37, 12.5, 0.11))])
def test_the_adversarial_grid(hip_module, voxel, origin):
    """negative cells, a non-zero origin and q = 2^24: the scan is the map's own centroids under a small pose offset"""
    poses, clouds = TS.adversarial_plus(voxel, origin)
    H, T = surfeled(hip_module, poses, clouds, 0xFF, voxel, origin, min_points=3, min_planarity=-1.0)   # every solved voxel with ev2 > 0
    assert (T.c < 0.0).any() and T.eligible.sum() >= 15
    pose = LS.offset(np.eye(4), 0.05 * voxel, 1e-4)
    scan = (T.c - pose[:3, 3]) @ pose[:3, :3]
    got = check_linearise(H, T, scan, pose, 1.0)
    assert got["matched"] >= 50 and got["used"] >= 50
    for base in ([1000, 1000, 0], [-2000, 500, 3]):   # the thousand-point voxels of the hand-made sets match themselves
        j = int(np.flatnonzero((T.cells == np.array(base) + [8, 0, 0]).all(axis=1))[0])
        assert got["ids"][j] == j
    check_linearise(H, T, scan, np.eye(4), 0.01)
    H.close()
