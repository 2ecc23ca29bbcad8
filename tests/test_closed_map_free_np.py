"""The free space's restatement (tests/closed_map_free_np.py) without a GPU: the three scenes' conditions
and their static figures as integers, the free condition on single rays, and the grid's additivity."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_carve_np as CN  # noqa: E402
import closed_map_free_np as FN  # noqa: E402
import diff_scenes as DS  # noqa: E402
import localise_scenes as LS  # noqa: E402
import voxel_map_np as VN  # noqa: E402

I, U, F, X = FN.INVALID, FN.UNKNOWN, FN.FREE, FN.OCCUPIED


def grid_of(poses, clouds, voxel, **cfg):
    V = CN.build_map(poses, clouds, CS.MASK, voxel)
    G = FN.FreeNP(V, **cfg)
    assert G.reset(poses=poses)
    return V, G, G.add_keyframes(poses, clouds, CS.MASK)


@pytest.fixture(scope="module")
def wall():
    poses, clouds, _, _ = LS.wall()
    return (poses, clouds) + grid_of(poses, clouds, 0.5, max_range=12.0, end_margin=1.0)


@pytest.fixture(scope="module")
def static():
    poses, clouds = CS.static_pass()
    return (poses, clouds) + grid_of(poses, clouds, CS.STATIC["voxel"], max_range=CS.STATIC["max_range"])


def test_the_wall(wall):
    poses, clouds, V, G, info = wall
    assert (info["rays"], info["skipped_rays"], info["cells_marked"], G.visited) == (5757, 0, 98767, 112169)
    assert (info["free_cells"], info["cells_outside"], info["n_bricks"]) == (875, 0, (19, 14, 14))
    assert info["bytes"] == 8 * 19 * 14 * 14 and info["keyframes"] == 6 and len(G.marked_keys) == 875
    assert len(G.free_cells()) == 875 and not np.isin(G.marked_keys, V.keys).any()          # none of them a voxel
    probes = [((6, 2, 1.5), F), ((6, 3.9, 1.5), F), ((6, 0, 1.5), F), ((6, 5.2, 1.5), X), ((6, 4.7, 1.5), U), ((6, 5.7, 1.5), U),
              ((6, 7, 1.5), U), ((6, -3, 1.5), U), ((6, 2, 4.5), U), ((6, 2, -0.5), U)]
    state, ids, counts = G.occupancy(np.array([p for p, _ in probes], np.float64))
    assert list(state) == [s for _, s in probes] and list(counts) == [0, 6, 3, 1]
    assert (ids[state == X] >= 0).all() and (ids[state != X] == -1).all()
    # the columns over the band of z cells 1 .. 5
    assert G.band(0.5, 2.9) == (1, 5)
    col = G.columns(0.5, 2.9)
    x0, y0 = -info["lo_cells"][0], -info["lo_cells"][1]        # the column of cell (0, 0)
    assert col.shape == (56, 76) and (col[y0 + 10, x0:x0 + 25] == X).all()
    assert not (col[y0 + 11:] == F).any() and not (col[:y0] == F).any() and (col == F).sum() > 100
    assert (G.columns(0.5, 2.9, min_free=6) == F).sum() == 0 and 0 < (G.columns(0.5, 2.9, min_free=5) == F).sum() < (col == F).sum()
    assert G.band(-100.0, -50.0) == (1, 0) and (G.columns(-100.0, -50.0) == U).all()
    # a metric box on the centres, and the order of the list: word index ascending, then bit ascending
    cen = G.free_cells()
    inside, idx, bit = G.locate(np.floor(cen / 0.5).astype(np.int64))
    assert inside.all() and (np.diff(idx * 64 + bit) > 0).all()
    part = G.free_cells(lo=(5.0, 0.0, 1.0), hi=(7.0, 3.0, 2.0))
    sel = (cen >= (5.0, 0.0, 1.0)).all(axis=1) & (cen <= (7.0, 3.0, 2.0)).all(axis=1)
    assert 0 < len(part) < len(cen) and part.tobytes() == cen[sel].tobytes()


def test_the_ghost_gate():
    poses, clouds, _, _, _ = DS.ghost_gate()
    V, G, info = grid_of(poses, clouds, DS.VOXEL, max_range=DS.MAX_RANGE)
    assert (info["rays"], info["cells_marked"], info["free_cells"]) == (5821, 99423, 875)
    M, _ = CN.carve(V, poses, clouds, CS.MASK, max_range=DS.MAX_RANGE)
    box = DS.box_voxels(V)
    C = V.centroids()[box]
    assert len(box) == 8
    state, ids, _ = G.occupancy(C)
    assert (state == X).all() and np.array_equal(ids, box)
    G.cfg["carve_gate"] = 1
    state, ids, _ = G.occupancy(C, misses=M)
    assert (state == F).all() and (ids == -1).all()        # a voxel the carve saw through reads as free space
    assert len(G.free_cells(misses=M)) == 875 and len(G.free_cells(lo=DS.BOX_LO, hi=DS.BOX_HI, misses=M)) == 8


def test_the_static_pass(static):
    poses, clouds, V, G, info = static
    assert (info["rays"], info["skipped_rays"], info["cells_marked"], G.visited) == (152074, 15702, 2870271, 3150076)
    assert (info["free_cells"], info["cells_outside"], info["n_bricks"]) == (16575, 0, (29, 22, 22))
    assert int(np.isin(G.marked_keys, V.keys).sum()) == 3263 and len(G.free_cells()) == 16575 - 3263
    state, _, counts = G.occupancy(V.centroids())
    assert (state == X).all() and counts[X] == len(V.keys)


def test_the_free_condition_on_single_rays():
    v, o = 0.5, (0.0, 0.0, 0.0)
    t = np.array([6.25, 0.25, 1.25])   # a cell centre
    one = lambda E, **kw: FN.marked(t[None], np.asarray(E, np.float64)[None], v, o, **kw)  # noqa: E731
    cells, skipped, visited = one(t + [4.0, 0.0, 0.0], max_range=12.0, end_margin=1.0)
    # eight steps along x; t_in = (k - 0.5) / 8 for cell k >= 1 against tlim = 0.75: cells 0 .. 6
    assert (skipped, visited) == (0, 8) and cells.tolist() == [[12 + k, 0, 2] for k in range(7)]
    assert len(one(t + [4.0, 0.0, 0.0], end_margin=0.0)[0]) == 8           # the end cell is never visited
    assert len(one(t + [1.0, 0.0, 0.0], end_margin=1.0)[0]) == 0           # L <= end_margin: not even the start cell
    assert len(one(t + [0.5, 0.5, 0.0], end_margin=np.sqrt(0.5))[0]) == 0
    assert one(t + [0.125, 0.0625, -0.125])[1:] == (0, 0) and len(one(t + [0.125, 0.0625, -0.125])[0]) == 0   # inside one cell
    for E in ([np.nan, 0.0, 0.0], [np.inf, 0.0, 0.0], t, t + [0.0, 30.0, 0.0], [2.0 ** 19 + 5.0, 0.0, 0.0]):
        assert one(E, max_range=12.0)[1:] == (1, 0)                        # skipped
    # a diagonal whose tMax ties on three axes: x, then y, then z, a brick change at nearly every step
    cells, _, visited = one(t + [2.0, 2.0, 2.0], end_margin=0.0)
    assert visited == 12 and cells[:4].tolist() == [[12, 0, 2], [13, 0, 2], [13, 1, 2], [13, 1, 3]]
    # the marked cells are a prefix of the carve's visited cells
    rng = np.random.default_rng(4)
    for _ in range(50):
        O, E = rng.uniform(-6.0, 6.0, 3), rng.uniform(-6.0, 6.0, 3)
        seen, _ = CN.walk(O / v, E / v)
        cells = FN.marked(O[None], E[None], v, o, end_margin=float(rng.uniform(0.0, 3.0)))[0]
        assert cells.tolist() == seen[:len(cells)].tolist()


def test_the_brick_layout_floors_negative_cells():
    V = VN.VoxelMapNP(0.5, (0.0, 0.0, 0.0))
    G = FN.FreeNP(V)
    assert G.reset(lo=(-5, -1, 3), hi=(2, 0, 3))
    assert G.blo.tolist() == [-2, -1, 0] and G.nb.tolist() == [3, 2, 1] and G.info()["lo_cells"] == (-8, -4, 0)
    inside, idx, bit = G.locate([[-5, -1, 3], [-4, 0, 3], [-1, -1, 0], [3, 0, 3], [4, 0, 3], [-9, 0, 3]])
    assert inside.tolist() == [True, True, True, True, False, False]
    assert idx[:4].tolist() == [0, 4, 1, 5] and bit[:4].tolist() == [3 | (3 << 2) | (3 << 4), 3 << 4, 3 | (3 << 2), 3 | (3 << 4)]
    for lo, hi in (((1, 0, 0), (0, 0, 0)), ((-2 ** 20, 0, 0), (0, 0, 0)), ((0, 0, 0), (0, 2 ** 20, 0))):
        assert not G.reset(lo=lo, hi=hi)
    assert not FN.FreeNP(V, max_bytes=40).reset(lo=(-5, -1, 3), hi=(2, 0, 3)) and FN.FreeNP(V, max_bytes=48).reset(lo=(-5, -1, 3), hi=(2, 0, 3))
    assert [a.tolist() for a in FN.auto_box(np.zeros((0, 4, 4)), 0.5, (0, 0, 0), 60.0)] == [[0, 0, 0], [0, 0, 0]]
    lo, hi = FN.auto_box(np.eye(4)[None], 1e-5, (0, 0, 0), 60.0)   # R = 6 000 001 cells: clamped
    assert lo.tolist() == [-(2 ** 20 - 1)] * 3 and hi.tolist() == [2 ** 20 - 1] * 3


def test_additivity(wall):
    poses, clouds, V, G, info = wall
    # add_keyframes over all K is the OR of K single-keyframe grids
    words = np.zeros_like(G.words)
    marked = 0
    for k in range(len(poses)):
        one = FN.FreeNP(V, **{key: G.cfg[key] for key in ("max_range", "end_margin")})
        one.reset(poses=poses)
        marked += one.add_keyframes(poses[k:k + 1], clouds[k:k + 1], CS.MASK)["cells_marked"]
        words |= one.words
    assert words.tobytes() == G.words.tobytes() and marked == info["cells_marked"]
    # keyframes added in two goes, as after an extend
    two = FN.FreeNP(V, max_range=12.0)
    two.reset(poses=poses)
    two.add_keyframes(poses[:4], clouds[:4], CS.MASK)
    assert two.add_keyframes(poses, clouds, CS.MASK)["keyframes"] == 6 and two.words.tobytes() == G.words.tobytes()
    # a scan fed as a one-keyframe input is add_scan of it
    scan, pose = CN.concatenation(clouds[2], CS.MASK), LS.offset(np.asarray(poses[2]), 0.3, 0.2)
    a, b = FN.FreeNP(V, max_range=12.0), FN.FreeNP(V, max_range=12.0)
    a.reset(poses=poses), b.reset(poses=poses)
    ia, ib = a.add_keyframes([pose], [clouds[2]], CS.MASK), b.add_scan(scan, pose)
    assert a.words.tobytes() == b.words.tobytes() and ia["cells_marked"] == ib["cells_marked"] > 0
    assert (ia["keyframes"], ia["scans"], ib["keyframes"], ib["scans"]) == (1, 0, 0, 1)
