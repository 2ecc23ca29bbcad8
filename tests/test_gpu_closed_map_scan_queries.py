"""What the closed map's scan queries share (tl_voxel.hpp: probe27, cell_voxel; tl_common.hpp: CarveGate):
the carve gate is one gate -- the diff, the ray-cast and the free space's occupancy return no voxel the carved read leaves out --
and the 27-cell probe stops at the grid's last cell.  The scenes' conditions are checked with the numpy restatements alone (the
tests without the gpu mark); the device is then held to the restatements byte for byte, as the neighbouring tests hold it."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_carve_np as CN  # noqa: E402
import closed_map_diff_np as DN  # noqa: E402
import closed_map_free_np as FN  # noqa: E402
import closed_map_localise_np as LN  # noqa: E402
import closed_map_raycast_np as RN  # noqa: E402
import closed_map_surfel_np as SN  # noqa: E402
import diff_scenes as DS  # noqa: E402

gpu = pytest.mark.gpu
GATE = dict(min_miss=3, miss_ratio=1.0)        # what closed_map_read_carved is called with (min_count = 1)
OCCUPIED = 3                                   # TLOAM_OCCUPANCY_OCCUPIED


def restated(poses, clouds, voxel, origin=(0.0, 0.0, 0.0), min_points=5, min_planarity=0.05):
    """the map and the localiser's target as the restatements see them (test_gpu_closed_map_localise.surfeled's defaults)"""
    V = CN.build_map(poses, clouds, CS.MASK, voxel, origin)
    S, normals, evals, _ = SN.surfels(V, poses, clouds, CS.MASK, min_points)
    return V, LN.Target(V, S, normals, evals, min_points, min_planarity=min_planarity)


# ---- the gate is one gate ----------------------------------------------------------------------------------------------------
def gate_scene():
    poses, clouds, _, _ = CS.ghost_scene()
    _, _, scan, pose, _ = DS.ghost_gate()       # a scan from DS.SENSORS[0] of the wall and of points inside the ghost box
    return poses, clouds, scan, pose


def test_the_gate_scene_meets_its_conditions():
    """restatements only: the carved read leaves voxels out, and with the gate off each of the three queries returns one of them"""
    poses, clouds, scan, pose = gate_scene()
    V, T = restated(poses, clouds, DS.VOXEL)
    M, _ = CN.carve(V, poses, clouds, CS.MASK, max_range=DS.MAX_RANGE)
    kept = CN.read_carved(V, M, min_count=1, **GATE)
    gone = np.setdiff1d(np.arange(len(V.keys)), kept)
    assert 0 < len(gone) < len(V.keys)
    G = FN.FreeNP(V, max_range=DS.MAX_RANGE, **GATE)
    assert G.reset(None, None, poses=poses)
    G.add_keyframes(poses, clouds, CS.MASK)
    state, occ, _ = G.occupancy(scan, pose, misses=M)
    assert np.isin(DN.diff(T, V, scan, pose, dict(max_range=DS.MAX_RANGE, **GATE), M)["ids"], gone).any()
    assert np.isin(RN.cast(T, V, scan, pose, dict(GATE), M)["ids"], gone).any()
    assert np.isin(occ[state == OCCUPIED], gone).any()


@gpu
def test_the_gate_is_one_gate(hip_module):
    import test_gpu_closed_map_diff as TD
    reg = hip_module
    assert reg.OCCUPANCY_OCCUPIED == OCCUPIED
    poses, clouds, scan, pose = gate_scene()
    H, _, _ = TD.surfeled_with_map(reg, poses, clouds, CS.MASK, DS.VOXEL)
    H.closed_map_carve_configure(max_range=DS.MAX_RANGE)
    H.closed_map_carve()
    row = {c.tobytes(): i for i, c in enumerate(H.closed_map_read()[0])}              # ids by centroid
    kept = np.array([row[c.tobytes()] for c in H.closed_map_read_carved(min_count=1, **GATE)[0]])
    gone = np.setdiff1d(np.arange(len(row)), kept)
    assert len(kept) + len(gone) == len(row) and 0 < len(gone) < len(row)

    def queries(gate):
        cfg = dict(carve_gate=gate, **GATE)
        H.closed_map_diff_configure(max_range=DS.MAX_RANGE, **cfg)
        H.closed_map_raycast_configure(**cfg)
        H.closed_map_free_configure(max_range=DS.MAX_RANGE, **cfg)
        H.closed_map_free_build()
        state, occ, _ = H.closed_map_occupancy(scan, pose, want_ids=True)
        return (H.closed_map_diff(scan, pose, want_ids=True)[1], H.closed_map_raycast(scan, pose, want_ids=True)[2],
                occ[state == reg.OCCUPANCY_OCCUPIED])

    for name, ids in zip(("diff", "raycast", "occupancy"), queries(1)):
        print(f"gate on, {name}: {(ids >= 0).sum()} ids, {np.isin(ids, gone).sum()} of them left out by read_carved")
        assert (ids >= 0).any() and np.isin(ids[ids >= 0], kept).all(), name
    assert (queries(1)[2] >= 0).all()                                                  # an OCCUPIED point has its voxel
    for name, ids in zip(("diff", "raycast", "occupancy"), queries(0)):
        print(f"gate off, {name}: {np.isin(ids, gone).sum()} ids left out by read_carved")
        assert np.isin(ids, gone).any(), name
    H.close()


# ---- the probe at the grid's last cell ---------------------------------------------------------------------------------------
EDGE = 2.0 ** 20 - 1.0                          # exact in double; voxel 1.0


def edge_scene(side):
    """side +1: every point in cell i_x = 2^20 - 1, the grid's last (origin_x = -(2^20 - 1)); side -1: in i_x = 1 - 2^20, its
    first.  Every x lies in [0, 1) -- a point at x >= 1 (x < 0) would put its whole keyframe beyond the grid -- over three cells
    in y and three in z: a floor patch in keyframe 0, a wall patch in keyframe 1 under a translated pose.  The scan: the map's own
    centroids and points under three small offsets, from a sensor inside the cell
    -> (poses, clouds, origin, scan, pose)"""
    origin = (-side * EDGE, 0.0, 0.0)
    xs = 0.125 + 0.1875 * np.arange(5)                                                 # 0.125 .. 0.875, dyadic
    ys = 0.1 + 0.2 * np.arange(15)                                                     # 0.1 .. 2.9: cells 0, 1, 2
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    floor = np.stack([X, Y, 1.25 + 0.125 * X], axis=-1).reshape(-1, 3)
    X, Z = np.meshgrid(xs, ys, indexing="ij")
    wall = np.stack([X, 3.5 + 0.125 * X, Z], axis=-1).reshape(-1, 3)
    P1 = DS.pose_at((0.25, 1.0, 0.5))
    poses = np.array([np.eye(4), P1])
    clouds = [CS.slot0(floor), CS.slot0(wall - P1[:3, 3])]
    V = CN.build_map(poses, clouds, CS.MASK, 1.0, origin)
    assert (V.i[:, 0] == side * (2 ** 20 - 1)).all() and len(np.unique(V.i[:, 1])) >= 3 and len(np.unique(V.i[:, 2])) >= 3
    world = np.concatenate([V.centroids(), CN.transform(poses[0], floor), CN.transform(P1, wall - P1[:3, 3])])
    world = np.concatenate([world + d for d in ([0.03125, 0.02, -0.02], [-0.0625, 0.3, 0.05], [0.0625, -0.2, 0.3])])   # two blocks
    assert (world[:, 0] >= 0.0).all() and (world[:, 0] < 1.0).all()
    sensor = (0.5, 1.5, 2.75)
    return poses, clouds, origin, DS.scan_from(world, sensor), DS.pose_at(sensor)


def device_sums(terms, ids_used, n):
    """the 28 sums in the device's order (tl_localise.hip): a point's terms in its lane, zero in a lane without a used point; the
    wave's 64 lanes by the xor butterfly (offsets 32 .. 1, lane 0's result); a block's four waves ((w0 + w1) + w2) + w3; the
    blocks' rows added in block order from 0.0.  ids_used: the scan indices of the rows of `terms`"""
    lanes = np.zeros((256 * ((n + 255) // 256), terms.shape[1]))
    lanes[ids_used] = terms
    idx = np.arange(64)
    total = np.zeros(terms.shape[1])
    for block in lanes.reshape(-1, 4, 64, terms.shape[1]):
        w = []
        for v in block:
            for off in (32, 16, 8, 4, 2, 1):
                v = v + v[idx ^ off]
            w.append(v[0])
        total = total + (((w[0] + w[1]) + w[2]) + w[3])
    return total


@pytest.mark.parametrize("side", [1, -1])
def test_the_edge_scene_meets_its_conditions(side):
    """restatements only: the diff explains a point and the linearise matches one -- the map is not empty to either"""
    poses, clouds, origin, scan, pose = edge_scene(side)
    V, T = restated(poses, clouds, 1.0, origin)
    labels = DN.diff(T, V, scan, pose)["labels"]
    assert ((labels == 1) | (labels == 2)).any()                                       # TLOAM_DIFF_SURFACE, _OCCUPIED
    assert LN.linearise(T, scan, pose, 1.0)["matched"] >= 1 and len(V.keys) <= 300 and len(scan) <= 3000


@gpu
@pytest.mark.parametrize("side", [1, -1])
def test_the_probe_at_the_grids_last_cell(hip_module, side):
    import test_gpu_closed_map_diff as TD
    import test_gpu_closed_map_localise as TL
    poses, clouds, origin, scan, pose = edge_scene(side)
    H, T, V = TD.surfeled_with_map(hip_module, poses, clouds, CS.MASK, 1.0, origin)
    info, want = TD.check_diff(H, T, V, scan, pose)                                    # labels, ids, counts, counters: bytes
    assert info["n_surface"] + info["n_occupied"] >= 1 and info["n_invalid"] == 0
    for tau in (1.0, 0.03):
        got, ref = TL.check_linearise(H, T, scan, pose, tau), LN.linearise(T, scan, pose, tau)
        used = np.flatnonzero((ref["ids"] >= 0) & (np.fabs(ref["residuals"]) <= tau))
        sums = device_sums(ref["terms"], used, len(scan))
        assert ref["matched"] >= 1 and got["ids"].tobytes() == ref["ids"].astype(got["ids"].dtype).tobytes()
        assert TL.bits(np.concatenate([got["H"], got["g"], [got["cost"]]])) == TL.bits(sums)
        assert (got["matched"], got["used"]) == (ref["matched"], ref["used"])
    H.close()
