"""-m gpu: several hypotheses of one scan in one set of launches (k_loc_sweep, k_loc_step over B hypotheses)
against the single call from each prior: pose, info and log bit for bit, the pick by its rule, the lifecycle.  The scenes are
those of tests/test_gpu_closed_map_localise.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import localise_scenes as LS  # noqa: E402
import test_gpu_closed_map_localise as TL  # noqa: E402

pytestmark = pytest.mark.gpu

bits, invalid, not_ready, context, surfeled, log_bytes = TL.bits, TL.invalid, TL.not_ready, TL.context, TL.surfeled, TL.log_bytes
DEGENERATE = 2


def pick(infos, logs):
    """the header's rule, restated: not DEGENERATE, the largest used, the smaller cost of the last executed sweep, the lower index"""
    best = -1
    for h, (i, log) in enumerate(zip(infos, logs)):
        if i["status"] == DEGENERATE:
            continue
        key = (-i["used"], log[-1]["cost"])
        if best < 0 or key < (-infos[best]["used"], logs[best][-1]["cost"]):
            best = h
    return best


def singles(H, pts, priors):
    out = []
    for prior in priors:
        pose, info = H.closed_map_localise(pts, prior)
        out.append((pose, info, H.closed_map_localise_log()))
    return out


def check_batch(H, pts, priors, want=None):
    """a batch against the single calls from the same priors, bit for bit -> (poses, infos, best)"""
    want = want if want is not None else singles(H, pts, priors)
    poses, infos, best = H.closed_map_localise_batch(pts, np.array(priors))
    logs = [H.closed_map_localise_batch_log(h) for h in range(len(priors))]
    for h, (wpose, winfo, wlog) in enumerate(want):
        assert bits(poses[h]) == bits(wpose), h
        assert {**infos[h], "prepared": 0} == {**winfo, "prepared": 0}, h
        assert len(logs[h]) == winfo["iterations"] and log_bytes(logs[h]) == log_bytes(wlog), h
    assert best == pick(infos, logs)
    return poses, infos, best


@pytest.fixture(scope="module")
def corner(hip_module):
    poses, clouds, scan, truth = LS.corner()
    H, _ = surfeled(hip_module, poses, clouds, CS.MASK, LS.CORNER["voxel"])
    yield H, scan, truth
    H.close()


@pytest.fixture(scope="module")
def wall(hip_module):
    poses, clouds, scan, truth = LS.wall()
    H, _ = surfeled(hip_module, poses, clouds, CS.MASK, CS.GHOST["voxel"])
    yield H, scan, truth
    H.close()


@pytest.fixture(scope="module")
def static(hip_module):
    poses, clouds = CS.static_pass()
    scan, truth = LS.static_scan(poses)
    H, _ = surfeled(hip_module, poses, clouds, CS.MASK, CS.STATIC["voxel"])
    yield H, scan, truth, (poses, clouds)
    H.close()


def spread(truth, B):
    """B priors around `truth`: offsets growing from 0.05 m / 0.002 rad, all within the single call's reach"""
    return [LS.offset(truth, 0.05 + 0.02 * h, 0.002 + 0.001 * h) for h in range(B)]


# ---- 1: a batch against single calls -----------------------------------------------------------------------------------------
def test_the_static_pass_from_its_four_starts(static, hip_module):
    H, scan, truth, _ = static
    priors = [LS.offset(truth, *s) for s in LS.STARTS]
    poses, infos, best = check_batch(H, scan, priors)
    assert {i["launches"] for i in infos} == {40} and best >= 0
    assert len({i["iterations"] for i in infos}) > 1          # each ends at its own iteration
    assert max(TL.LN.pose_error(poses[best], truth)) < 1e-2


def test_the_corner_from_three_starts(corner, hip_module):
    H, scan, truth = corner
    priors = [LS.offset(truth, *LS.CORNER_START), LS.offset(truth, 0.1, -0.02), LS.offset(truth, -0.15, 0.01)]
    poses, infos, best = check_batch(H, scan, priors)
    assert all(i["status"] == hip_module.LOCALISE_CONVERGED for i in infos)
    assert max(TL.LN.pose_error(poses[best], truth)) < 1e-9


# ---- 2: batch shapes and scan sizes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 31, 32])
def test_batch_sizes(corner, B):
    H, scan, truth = corner
    check_batch(H, scan, spread(truth, B))


@pytest.fixture
def few_iterations(static):
    H = static[0]
    H.closed_map_localise_configure(max_iterations=4, min_matches=1)
    yield static
    H.closed_map_localise_configure()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_wave_and_block_edges(few_iterations, n):
    """the hypothesis stride of the partial rows: one block, exactly one, one and a point, five"""
    H, scan, truth, _ = few_iterations
    check_batch(H, scan[5000:5000 + n], spread(truth, 3))


# ---- 3: edge cases -----------------------------------------------------------------------------------------------------------
def test_a_mixed_batch(static, wall, hip_module):
    H, scan, truth, _ = static
    far = truth.copy()
    far[:3, 3] += [0.0, 0.0, 50.0]
    priors = [LS.offset(truth, *LS.STARTS[0]), far, LS.offset(truth, *LS.STARTS[3]), far]
    poses, infos, best = check_batch(H, scan, priors)
    assert [i["status"] == DEGENERATE for i in infos] == [False, True, False, True]
    assert infos[1]["iterations"] == 1 and infos[0]["iterations"] > 1 and bits(poses[1]) == bits(far) and best in (0, 2)
    # all degenerate: no pick, the priors come back
    poses, infos, best = check_batch(H, scan, [far, far.copy()])
    assert best == -1 and bits(poses) == bits(np.array([far, far]))
    # the wall's geometry: degenerate by the pivot test, not by the count
    W, wscan, wtruth = wall
    wpriors = [LS.offset(wtruth, 0.2, 0.03), LS.offset(wtruth, 0.1, 0.01)]
    poses, infos, best = check_batch(W, wscan, wpriors)
    assert best == -1 and all(i["status"] == DEGENERATE and i["used"] > 100 for i in infos) and bits(poses) == bits(np.array(wpriors))


def test_calls_and_contexts_give_the_same_bytes(static, hip_module):
    H, scan, truth, (poses, clouds) = static
    priors = np.array([LS.offset(truth, *s) for s in LS.STARTS])
    a = H.closed_map_localise_batch(scan, priors)
    alog = [log_bytes(H.closed_map_localise_batch_log(h)) for h in range(4)]
    b = H.closed_map_localise_batch(scan, priors)
    assert bits(a[0]) == bits(b[0]) and a[1:] == b[1:] and alog == [log_bytes(H.closed_map_localise_batch_log(h)) for h in range(4)]
    other, _ = surfeled(hip_module, poses, clouds, CS.MASK, CS.STATIC["voxel"], reserve_voxels=64)
    c = other.closed_map_localise_batch(scan, priors)
    assert all(i["prepared"] == 1 for i in c[1]) and bits(c[0]) == bits(a[0]) and c[2] == a[2]
    assert [{**i, "prepared": 0} for i in c[1]] == [{**i, "prepared": 0} for i in a[1]]
    assert alog == [log_bytes(other.closed_map_localise_batch_log(h)) for h in range(4)]
    other.close()


def test_lifecycle(hip_module):
    reg = hip_module
    poses, clouds, scan, truth = LS.corner()
    prior = LS.offset(truth, *LS.CORNER_START)
    priors = np.array([prior, LS.offset(truth, 0.1, -0.02)])
    H = context(reg, poses, clouds, voxel=LS.CORNER["voxel"], cloud_mask=CS.MASK)
    with not_ready(reg):
        H.closed_map_localise_batch(scan, priors)          # before a build
    H.closed_map_build(2, poses)
    with not_ready(reg):
        H.closed_map_localise_batch(scan, priors)          # before surfels
    with invalid(reg):
        H.closed_map_localise_batch_log(0)                 # no batch yet
    H.closed_map_surfels()
    H.closed_map_localise(scan, prior)
    single = log_bytes(H.closed_map_localise_log())
    got = H.closed_map_localise_batch(scan, priors)
    logs = [log_bytes(H.closed_map_localise_batch_log(h)) for h in range(2)]
    assert logs[0] == single and got[1][0]["launches"] == 40
    with invalid(reg):
        H.closed_map_localise_batch_log(2)
    # refused calls leave the single call's log and the batch's logs as they were
    bad = priors.copy()
    bad[1] *= 2.0
    nan = priors.copy()
    nan[0, 0, 3] = np.nan
    for p in (bad, nan, np.zeros((0, 4, 4)), np.repeat(priors[:1], 33, axis=0)):
        with invalid(reg):
            H.closed_map_localise_batch(scan, p)
    with invalid(reg):
        H.closed_map_localise_batch(np.zeros((0, 3)), priors)
    assert log_bytes(H.closed_map_localise_log()) == single
    assert [log_bytes(H.closed_map_localise_batch_log(h)) for h in range(2)] == logs
    # a single call leaves the batch's logs, a batch the single call's
    H.closed_map_localise(scan, priors[1])
    assert [log_bytes(H.closed_map_localise_batch_log(h)) for h in range(2)] == logs
    assert log_bytes(H.closed_map_localise_log()) == logs[1]
    # ... also from a prior that is in neither: one run path, two record stores
    H.closed_map_localise(scan, LS.offset(truth, -0.1, 0.01))
    alone = log_bytes(H.closed_map_localise_log())
    assert alone and alone not in logs
    assert [log_bytes(H.closed_map_localise_batch_log(h)) for h in range(2)] == logs
    H.closed_map_localise_batch(scan, priors)
    assert log_bytes(H.closed_map_localise_log()) == alone
    assert [log_bytes(H.closed_map_localise_batch_log(h)) for h in range(2)] == logs
    # launches: 2 max_iterations for every input
    H.closed_map_localise_configure(max_iterations=7)
    seen = {i["launches"] for p in (scan, scan[:10], scan + 100.0) for i in H.closed_map_localise_batch(p, priors)[1]}
    assert seen == {14}
    # the surfels go, and the logs with them
    H.closed_map_surfel_configure(min_points=7)
    with not_ready(reg):
        H.closed_map_localise_batch(scan, priors)
    with invalid(reg):
        H.closed_map_localise_batch_log(0)
    H.close()
    H = reg.HipRegistration()
    H.comm_init_callback(0, 2, lambda dev, count, stream: 0)
    for call in (lambda: H.closed_map_localise_batch(scan, priors), lambda: H.closed_map_localise_batch_log(0)):
        with invalid(reg):
            call()
    H.close()
