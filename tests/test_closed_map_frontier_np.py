"""The restatement of the closed map's frontiers (tests/closed_map_frontier_np.py) against references it
does not share code with: scipy.ndimage.label with the full 3 x 3 x 3 structure for the partition, a loop over cells for the cost
join; and figures derived by hand: a run in unknown space, a solid block, a box that is all free, a voxel that splits a run, two
runs that touch at a vertex, min_cells at a cluster's size, and the wall scene's table as integers."""
import os
import sys

import numpy as np
import pytest
import scipy.ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_carve_np as CN  # noqa: E402
import closed_map_clearance_np as KN  # noqa: E402
import closed_map_free_np as FN  # noqa: E402
import closed_map_frontier_np as QN  # noqa: E402
import closed_map_route_np as RN  # noqa: E402
import frontier_scenes as QS  # noqa: E402
import localise_scenes as LS  # noqa: E402

U, F, O = FN.UNKNOWN, FN.FREE, FN.OCCUPIED


def unknown(nx, ny, nz):
    return np.full((nz, ny, nx), U, np.uint8)


def solved(state, lo=(0, 0, 0), min_cells=1):
    field, rec, kept, kept_of, counts, _ = QN.solve(state, lo, min_cells)
    assert counts["free_cells"] + counts["unknown_cells"] + counts["occupied_cells"] == state.size
    assert counts["clusters"] == len(rec) and counts["clusters_kept"] == len(kept) == int((kept_of >= 0).sum())
    assert int(rec["cells"].astype(np.int64).sum()) == counts["frontier_cells"] == int((field.astype(np.int64) < QN.OUTSIDE).sum())
    assert int(rec["unknown_faces"].astype(np.int64).sum()) == counts["unknown_faces"]
    assert (np.diff(rec["root"].astype(np.int64)) > 0).all() and (rec["reserved"] == 0).all()
    return field, rec, kept, kept_of, counts


@pytest.mark.parametrize("shape, share", [((12, 16, 20), 0.3), ((12, 16, 20), 0.6), ((8, 24, 24), 0.3), ((8, 24, 24), 0.6)])
def test_the_partition_is_scipys_and_every_label_is_the_least_index(shape, share):
    rng = np.random.default_rng(shape[0] * 100 + int(10 * share))
    nx, ny, nz = shape
    state = np.where(rng.random((nz, ny, nx)) < share, F, U).astype(np.uint8)
    state[rng.random(state.shape) < 0.05] = O                      # voxels sprinkled in
    field, rec, _, _, counts = solved(state)
    f = field.astype(np.int64)
    front = f < QN.OUTSIDE
    # the frontier cells by a loop-free definition of their own: FREE with an UNKNOWN face neighbour inside the box
    pad = np.pad(state, 1, constant_values=O)
    near = np.zeros(state.shape, bool)
    for axis in range(3):
        for s in (-1, 1):
            near |= np.roll(pad, s, axis)[1:-1, 1:-1, 1:-1] == U
    assert np.array_equal(front, (state == F) & near)
    assert np.array_equal(f[~front], np.where(state == O, QN.OCCUPIED, np.where(state == F, QN.FREE, QN.UNKNOWN))[~front])
    lab, n = ndi.label(front, structure=np.ones((3, 3, 3), int))
    assert n == counts["clusters"] and n >= 1                      # (at a free share of 0.6 nearly everything is one component)
    index = np.arange(state.size).reshape(state.shape)
    least = ndi.minimum(index, lab, np.arange(1, n + 1)).astype(np.int64)
    assert np.array_equal(f[front], least[lab[front] - 1])         # the same partition, and every label its component's least index
    assert np.array_equal(np.sort(least), rec["root"].astype(np.int64))
    sizes = ndi.sum(front, lab, np.arange(1, n + 1)).astype(np.int64)
    assert np.array_equal(sizes[np.argsort(least)], rec["cells"].astype(np.int64))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_run_in_unknown_space(axis):
    L = 9
    e = np.eye(3, dtype=np.int64)[axis]
    state = unknown(16, 16, 16)
    a = np.array([3, 4, 5])
    cells = a + np.arange(L)[:, None] * e
    state[cells[:, 2], cells[:, 1], cells[:, 0]] = F
    field, rec, _, _, counts = solved(state, lo=(-8, 4, 0))
    assert len(rec) == 1 and rec["cells"][0] == L and rec["unknown_faces"][0] == 4 * L + 2
    assert rec["root"][0] == (5 * 16 + 4) * 16 + 3 and (field[cells[:, 2], cells[:, 1], cells[:, 0]] == rec["root"][0]).all()
    assert rec["lo"][0].tolist() == (a + [-8, 4, 0]).tolist() and rec["hi"][0].tolist() == (a + (L - 1) * e + [-8, 4, 0]).tolist()
    assert rec["sum"][0].tolist() == cells.sum(axis=0).tolist()
    # clipped at the box's faces, which contribute nothing: the run from face to face loses its two end faces, and a run along
    # the box's edge loses two of its four sides as well
    state = unknown(16, 16, 16)
    full = np.zeros(3, np.int64) + np.arange(16)[:, None] * e
    state[full[:, 2], full[:, 1], full[:, 0]] = F
    _, rec, _, _, _ = solved(state)
    assert len(rec) == 1 and rec["cells"][0] == 16 and rec["unknown_faces"][0] == 2 * 16


def test_a_solid_block_and_a_box_that_is_all_free():
    state = unknown(15, 14, 13)
    state[4:9, 5:10, 3:8] = F
    lo = (10, -20, 30)
    field, rec, kept, _, counts = solved(state, lo=lo, min_cells=8)
    assert counts["frontier_cells"] == 125 - 27 == 98 and len(rec) == len(kept) == 1 and rec["unknown_faces"][0] == 150
    assert counts["free_cells"] == 125 and (field[5:8, 6:9, 4:7] == QN.FREE).all()          # the core is free, not frontier
    o, v = np.array([0.5, -1.0, 2.0]), 0.25
    centre = o + (np.array(lo) + np.array([5.0, 7.0, 6.0]) + 0.5) * v                        # the block's centre cell (5, 7, 6)
    assert QN.centroids(kept, lo, o, v).tobytes() == centre[None].tobytes()
    _, rec, _, _, counts = solved(np.full((8, 8, 8), F, np.uint8))
    assert len(rec) == 0 and counts["frontier_cells"] == 0 and counts["largest"] == 0 and counts["free_cells"] == 512


def test_a_voxel_splits_a_run_and_a_vertex_joins_two():
    state = unknown(20, 8, 8)
    state[4, 4, 2:15] = F
    assert len(solved(state)[1]) == 1
    state[4, 4, 8] = O
    _, rec, _, _, _ = solved(state)
    assert rec["cells"].tolist() == [6, 6] and rec["unknown_faces"].tolist() == [4 * 6 + 1, 4 * 6 + 1]   # the voxel's face is not unknown
    # two runs that touch only at a vertex: (2 .. 5, 2, 2) and (6 .. 9, 3, 3)
    state = unknown(12, 8, 8)
    state[2, 2, 2:6] = F
    state[3, 3, 6:10] = F
    field, rec, _, _, _ = solved(state)
    assert len(rec) == 1 and rec["cells"][0] == 8 and rec["root"][0] == (2 * 8 + 2) * 12 + 2
    state[3, 3, 6] = U                                             # one cell further apart: two
    assert solved(state)[1]["cells"].tolist() == [4, 3]


def test_min_cells_at_a_clusters_size_and_one_above():
    state = unknown(24, 8, 8)
    state[2, 2, 1:6] = F                                           # 5 cells
    state[5, 5, 3:11] = F                                          # 8 cells
    state[6, 1, 20] = F                                            # 1 cell
    for min_cells, want, index in ((1, [5, 8, 1], [0, 1, 2]), (2, [5, 8], [0, 1, -1]), (5, [5, 8], [0, 1, -1]), (6, [8], [-1, 0, -1]),
                                   (8, [8], [-1, 0, -1]), (9, [], [-1, -1, -1])):
        _, rec, kept, kept_of, counts = solved(state, min_cells=min_cells)
        assert rec["cells"].tolist() == [5, 8, 1] and kept["cells"].tolist() == want and kept_of.tolist() == index
        assert (counts["clusters"], counts["clusters_kept"], counts["cells_kept"], counts["largest"]) == (3, len(want), sum(want), 8)


def brute_join(field, kept, route, reach):
    """a loop over cells: per kept cluster the least (cost << 32) | linear within reach -> [key or None]"""
    nz, ny, nx = field.shape
    out = []
    for r in kept["root"].tolist():
        best = None
        for z, y, x in np.argwhere(field == r).tolist():
            for uz in range(max(z - reach, 0), min(z + reach, nz - 1) + 1):
                for uy in range(max(y - reach, 0), min(y + reach, ny - 1) + 1):
                    for ux in range(max(x - reach, 0), min(x + reach, nx - 1) + 1):
                        c = int(route[uz, uy, ux])
                        if c < RN.OUTSIDE:
                            key = (c << 32) | ((uz * ny + uy) * nx + ux)
                            best = key if best is None else min(best, key)
        out.append(best)
    return out


@pytest.mark.parametrize("reach", [0, 2, 4])
def test_the_cost_join(reach):
    """a room of free cells in unknown space with a corridor off it; the route over the free cells whose 26 neighbours are all
    free, from one goal: no frontier cell is traversable, so at reach 0 every cluster is unreached"""
    rng = np.random.default_rng(7)
    state = unknown(20, 14, 10)
    state[1:9, 1:13, 1:12] = F
    state[3:6, 5:9, 12:18] = F                                     # a corridor off the room
    state[rng.random(state.shape) < 0.01] = O
    field, rec, kept, _, _ = solved(state, lo=(4, 8, -4), min_cells=2)
    assert len(kept) >= 1
    not_free = np.pad(state != F, 1, constant_values=True)
    trav = ~ndi.binary_dilation(not_free, structure=np.ones((3, 3, 3), bool))[1:-1, 1:-1, 1:-1]   # no neighbour that is not free
    goals = np.argwhere(trav)[:1, ::-1]
    route, _ = RN.relax(trav, goals)
    o, v = np.array([1.0, 2.0, 3.0]), 0.5
    cost, approach = QN.cost_join(field, kept, route, reach, (4, 8, -4), o, v)
    want = brute_join(field, kept, route, reach)
    assert cost.dtype == np.uint32 and approach.shape == (len(kept), 3)
    for k, key in enumerate(want):
        if key is None:
            assert cost[k] == RN.UNREACHED and np.isnan(approach[k]).all()
        else:
            lin = key & 0xFFFFFFFF
            cell = np.array([lin % 20, lin // 20 % 14, lin // 280]) + (4, 8, -4)
            assert cost[k] == key >> 32 and approach[k].tobytes() == (o + (cell + 0.5) * v).tobytes()
    assert (cost == RN.UNREACHED).all() == (reach == 0) and (reach == 0 or (cost < RN.OUTSIDE).any())


def test_a_tie_goes_to_the_least_index():
    """two cells of equal cost within reach: the key's low half decides"""
    state = unknown(9, 5, 5)
    state[2, 2, 4] = F
    field, rec, kept, _, _ = solved(state)
    route = np.full(state.shape, RN.BLOCKED, np.uint32)
    route[2, 2, 2] = route[2, 2, 6] = route[1, 2, 4] = 7
    route[3, 2, 4] = 8
    cost, approach = QN.cost_join(field, kept, route, 2, (0, 0, 0), np.zeros(3), 1.0)
    assert cost.tolist() == [7] and approach.tolist() == [[4.5, 2.5, 1.5]]          # (4, 2, 1) has the least index of the three
    cost, approach = QN.cost_join(field, kept, route, 1, (0, 0, 0), np.zeros(3), 1.0)
    assert cost.tolist() == [7] and approach.tolist() == [[4.5, 2.5, 1.5]]
    cost, approach = QN.cost_join(field, kept, route, 0, (0, 0, 0), np.zeros(3), 1.0)
    assert cost.tolist() == [RN.UNREACHED] and np.isnan(approach).all()


def test_the_columns_form_is_the_field_of_one_layer():
    rng = np.random.default_rng(3)
    layer = np.where(rng.random((24, 40)) < 0.5, F, U).astype(np.uint8)
    layer[rng.random(layer.shape) < 0.05] = O
    field, rec, _, _, counts = solved(layer[None], lo=(0, 0, 12))
    lab, n = ndi.label(field[0].astype(np.int64) < QN.OUTSIDE, structure=np.ones((3, 3), int))     # 8-connected
    assert n == len(rec) and (rec["sum"][:, 2] == 0).all() and (rec["lo"][:, 2] == 12).all() and (rec["hi"][:, 2] == 12).all()
    faces = QN.unknown_faces(layer[None])
    assert faces.max() <= 4


def test_painted_runs_are_exact():
    """the painting the device tests rely on, in the restatement alone: exactly the runs' cells, the end cell never"""
    V = CN.build_map([np.eye(4)], [CS.slot0(np.array([[5000.5, 5000.5, 5000.5]]))], CS.MASK, 1.0)
    G = FN.FreeNP(V, **QS.PAINT)
    assert G.reset((0, 0, 0), (39, 11, 7))
    runs = [((2, 3, 4), (30, 3, 4)), ((2, 3, 4), (2, 9, 4)), ((5, 5, 5), (5, 5, 5)), ((39, 0, 0), (33, 0, 0)), ((7, 7, 0), (7, 7, 7))]
    want = QS.paint(G, runs)
    assert len(want) == 29 + 6 + 1 + 7 + 8 and QS.free_set(G) == want
    assert len(QS.paint(G, QS.block_runs((10, 6, 1), (12, 8, 3)))) == 27
    assert len(QS.paint(G, QS.serpentine_runs())) == 2 * (4 * 32 + 3) + 1


# the wall scene (unknown_is_obstacle plays no part), carve gate off / on ->
# (free, unknown, occupied, frontier cells, clusters, kept at min_cells = 8, cells kept, largest, unknown faces)
# (the wall has no ghost: the gate carves no voxel away and the two rows agree; the sensor's fan of rays ends in one shell)
WALL_TABLE = {0: (875, 237286, 175, 520, 1, 1, 520, 520, 740), 1: (875, 237286, 175, 520, 1, 1, 520, 520, 740)}


def test_the_wall():
    poses, clouds, _, _ = LS.wall()
    V = CN.build_map(poses, clouds, CS.MASK, 0.5)
    M, _ = CN.carve(V, poses, clouds, CS.MASK, max_range=12.0)
    got = {}
    for gate in (0, 1):
        G = FN.FreeNP(V, max_range=12.0, end_margin=1.0, carve_gate=gate)
        assert G.reset(poses=poses)
        G.add_keyframes(poses, clouds, CS.MASK)
        N = QN.FrontierNP(G)
        assert N.build(M if gate else None)
        info = N.info()
        assert info["n_cells"] == (76, 56, 56) and info["bytes"] == 4 * 76 * 56 * 56 + 8 * 3 * 7 * 14
        got[gate] = tuple(info[k] for k in ("free_cells", "unknown_cells", "occupied_cells", "frontier_cells", "clusters", "clusters_kept",
                                            "cells_kept", "largest", "unknown_faces"))
        rec, cen = N.clusters()
        assert len(rec) == info["clusters_kept"] and np.isfinite(cen).all()
        centres, roots = N.cells()
        assert len(centres) == info["cells_kept"] and set(roots.tolist()) == set(rec["root"].tolist())
    print(got)
    assert got == WALL_TABLE
