"""The diff of a scan against the closed map without a GPU: its numpy restatement
(tests/closed_map_diff_np.py) on the scenes of tests/diff_scenes.py and on the static pass.  Every figure here is an integer the
restatement gives; the device is held to the same ones bit for bit (tests/test_gpu_closed_map_diff.py)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_carve_np as CN  # noqa: E402
import closed_map_diff_np as DN  # noqa: E402
import diff_scenes as DS  # noqa: E402
import localise_scenes as LS  # noqa: E402

RANGE = dict(max_range=DS.MAX_RANGE)


def test_the_restatement_borrows_the_walk_and_the_association():
    src = open(os.path.join(HERE, "closed_map_diff_np.py")).read()
    assert "CN.Walk(" in src and "LN.associate(" in src and "class Walk" not in src and "def associate" not in src


@pytest.mark.parametrize("sensor,box_through", zip(DS.SENSORS, ((6, 28), (9, 32), (4, 18))))
def test_the_gone_scene(sensor, box_through):
    poses, clouds, scan, pose = DS.gone(sensor)
    V, _, _, _, T = LS.target(poses, clouds, CS.MASK, DS.VOXEL)
    assert len(scan) == 976 and len(V.keys) == 202
    R = DN.diff(T, V, scan, pose, RANGE)
    box = DS.box_voxels(V)
    rest = np.setdiff1d(np.arange(len(V.keys)), box)
    assert len(box) == 27
    assert (int(R["through"][box].min()), int(R["through"][box].max())) == box_through and not R["hits"][box].any()
    assert not R["through"][rest].any() and (R["hits"][rest] >= 1).all()
    assert np.array_equal(DN.read_gone(V, R["through"], R["hits"], **DN.GONE_DEFAULTS), box)
    assert np.array_equal(DN.read_gone(V, R["through"], R["hits"], DS.BOX_LO, DS.BOX_HI), box)
    assert len(DN.read_gone(V, R["through"], R["hits"], (0.0, 4.0, 0.0), (12.0, 6.0, 4.0))) == 0   # the wall's box
    if sensor == DS.SENSORS[0]:
        assert (R["info"]["steps"], R["info"]["tested"]) == (17298, 971)
    assert (R["labels"] == DN.SURFACE).all() and R["info"]["n_surface"] == 976
    # the scan as a one-keyframe carve IS the map side
    M, info = CN.carve(V, [pose], [CS.slot0(scan)], CS.MASK, **RANGE)
    assert np.array_equal(M, R["through"])
    assert (info["skipped_rays"], info["steps"], info["tested"], info["misses"], info["voxels_missed"]) == \
           tuple(R["info"][k] for k in ("skipped_rays", "steps", "tested", "through", "voxels_through"))


def test_the_appeared_scene():
    poses, clouds, scan, pose, is_box = DS.appeared()
    V, _, _, _, T = LS.target(poses, clouds, CS.MASK, DS.VOXEL)
    R = DN.diff(T, V, scan, pose, RANGE)
    assert is_box.sum() == 216 and (R["labels"][is_box] == DN.NEW).all() and (R["ids"][is_box] == -1).all()
    assert (R["labels"][~is_box] == DN.SURFACE).all() and (R["ids"][~is_box] >= 0).all()
    assert len(DN.read_gone(V, R["through"], R["hits"])) == 0
    assert R["info"]["n_new"] == 216 and R["info"]["n_surface"] == 976 and R["info"]["n_invalid"] == R["info"]["n_occupied"] == 0


def test_the_ghost_gate_scene():
    poses, clouds, scan, pose, is_box = DS.ghost_gate()
    V, _, _, _, T = LS.target(poses, clouds, CS.MASK, DS.VOXEL)
    M, _ = CN.carve(V, poses, clouds, CS.MASK, **RANGE)
    off = DN.diff(T, V, scan, pose, RANGE)
    on = DN.diff(T, V, scan, pose, dict(RANGE, carve_gate=1), misses=M)
    assert is_box.sum() == 64
    assert (off["labels"][is_box] == DN.OCCUPIED).all() and (off["ids"][is_box] >= 0).all()
    assert (on["labels"][is_box] == DN.NEW).all() and (on["ids"][is_box] == -1).all()
    for R in (off, on):
        assert (R["labels"][~is_box] == DN.SURFACE).all()
    # the counts are ungated
    assert np.array_equal(off["through"], on["through"]) and np.array_equal(off["hits"], on["hits"])


def test_accumulation_is_the_sum_of_the_single_results():
    poses, clouds, _, _ = DS.gone()
    V, _, _, _, T = LS.target(poses, clouds, CS.MASK, DS.VOXEL)
    singles = [DN.diff(T, V, *DS.gone(s)[2:], RANGE) for s in DS.SENSORS[:2]]
    both = DN.diff(T, V, *DS.gone(DS.SENSORS[1])[2:], RANGE, state=singles[0])
    assert np.array_equal(both["through"], singles[0]["through"] + singles[1]["through"])
    assert np.array_equal(both["hits"], singles[0]["hits"] + singles[1]["hits"])
    assert both["info"]["scans"] == 2 and both["info"]["through"] == singles[0]["info"]["through"] + singles[1]["info"]["through"]
    assert np.array_equal(both["labels"], singles[1]["labels"])   # the labels are per call


def test_invalid_points_are_skipped_rays():
    poses, clouds, scan, pose = DS.gone()
    V, _, _, _, T = LS.target(poses, clouds, CS.MASK, DS.VOXEL)
    bad = scan[:50].copy()
    bad[3] = np.nan
    bad[4] = [np.inf, 0.0, 0.0]
    bad[5] = [2.0 ** 19 + 5.0, 0.0, 0.0]   # |i| >= 2^20 at v = 0.5
    bad[6] = 0.0                            # at the sensor: a valid point, a skipped ray
    R = DN.diff(T, V, bad, pose, RANGE)
    assert list(R["labels"][3:7]) == [DN.INVALID, DN.INVALID, DN.INVALID, DN.NEW] and R["info"]["n_invalid"] == 3
    assert R["info"]["skipped_rays"] == 4 and (R["ids"][3:7] == -1).all()


@pytest.fixture(scope="module")
def static():
    poses, clouds = CS.static_pass()
    scan, truth = LS.static_scan(poses)
    V, _, _, _, T = LS.target(poses, clouds, CS.MASK, CS.STATIC["voxel"])
    return V, T, scan, truth


def test_the_static_figures(static):
    V, T, scan, truth = static
    assert len(V.keys) == 11557 and len(scan) == 18988
    R = DN.diff(T, V, scan, truth, dict(max_range=20.0))
    I = R["info"]
    assert (I["skipped_rays"], I["steps"], I["tested"], I["through"], I["voxels_through"], I["voxels_hit"]) == \
           (2076, 384950, 27726, 2507, 877, 3022)
    assert len(DN.read_gone(V, R["through"], R["hits"])) == 266
    assert (I["n_invalid"], I["n_surface"], I["n_occupied"], I["n_new"]) == (0, 17719, 773, 496)
    assert int((R["hits"].sum())) == 18988 - 824   # 824 points fall in an unoccupied cell
    far = DN.diff(T, V, scan, truth)
    J = far["info"]
    assert (J["skipped_rays"], J["steps"]) == (484, 511632) and len(DN.read_gone(V, far["through"], far["hits"])) == 291
    assert np.array_equal(far["labels"], R["labels"]) and np.array_equal(far["hits"], R["hits"])   # the range is the rays' alone
    # the ceiling on NEW: with plane_tol = 0 nothing here is SURFACE, and NEW is the points with no centroid of the 27 cells
    # within `near`.  Checked against every centroid of the map by brute force: the same count while near <= voxel (a centroid
    # that near lies in an adjacent cell), and fewer beyond it, where the ring of 27 cells no longer holds every such centroid
    E = CN.transform(truth, scan)
    C = V.centroids()
    nearest = np.full(len(E), np.inf)
    for a in range(0, len(E), 512):
        d = E[a:a + 512, None, :] - C[None, :, :]
        nearest[a:a + 512] = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(axis=1)
    for near, ceiling in ((0.5, 515), (0.25, 4409), (1.0, 226)):
        alone = DN.diff(T, V, scan, truth, dict(max_range=20.0, near=near, plane_tol=0.0))["info"]
        assert (alone["n_new"], alone["n_surface"], alone["n_invalid"]) == (ceiling, 0, 0)
        far = int((nearest > np.float64(near) * np.float64(near)).sum())
        assert far == ceiling if near <= V.voxel else far < ceiling
    M, info = CN.carve(V, [truth], [CS.slot0(scan)], CS.MASK, max_range=20.0)
    assert np.array_equal(M, R["through"]) and info["steps"] == I["steps"]
