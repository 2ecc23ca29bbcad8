"""The route's restatement (tests/closed_map_route_np.py) without a GPU: the fixpoint of the shifted-array
sweeps against a heap Dijkstra written here and against scipy's, need on and just off an integer, the properties of every
descended path, a tie the contract's order decides, and the wall scene's figures as integers."""
import heapq
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_carve_np as CN  # noqa: E402
import closed_map_clearance_np as KN  # noqa: E402
import closed_map_free_np as FN  # noqa: E402
import closed_map_route_np as RN  # noqa: E402
import localise_scenes as LS  # noqa: E402

U, BL, OUT = RN.UNREACHED, RN.BLOCKED, RN.OUTSIDE


def heap_dijkstra(trav, goals):
    """the textbook algorithm over the same graph -> the field (nz, ny, nx) uint32"""
    nz, ny, nx = trav.shape
    dist = {}
    heap = [(0, int(z), int(y), int(x)) for x, y, z in goals]
    heapq.heapify(heap)
    while heap:
        d, z, y, x = heapq.heappop(heap)
        if (z, y, x) in dist:
            continue
        dist[(z, y, x)] = d
        for step in RN.STEPS:
            uz, uy, ux = z + step[0], y + step[1], x + step[2]
            if 0 <= uz < nz and 0 <= uy < ny and 0 <= ux < nx and trav[uz, uy, ux] and (uz, uy, ux) not in dist:
                heapq.heappush(heap, (d + RN.weight(step), uz, uy, ux))
    out = np.where(trav, U, BL).astype(np.uint32)
    for (z, y, x), d in dist.items():
        out[z, y, x] = d
    return out


def random_scene(rng, shape, share, n_goals):
    """shape (nx, ny, nz) -> (trav (nz, ny, nx), goals (n, 3) local cells, all traversable and distinct)"""
    trav = rng.random(shape[::-1]) >= share
    free = np.argwhere(trav)[:, ::-1]
    return trav, free[rng.choice(len(free), n_goals, replace=False)]


def test_the_sweeps_end_at_a_heap_dijkstras_distances():
    rng = np.random.default_rng(11)
    for shape, share, n_goals in (((20, 16, 12), 0.2, 1), ((12, 16, 20), 0.35, 2), ((8, 24, 24), 0.5, 1), ((33, 9, 5), 0.3, 3),
                                  ((40, 30, 1), 0.3, 1), ((1, 1, 1), 0.0, 1)):
        trav, goals = random_scene(rng, shape, share, n_goals)
        got, sweeps = RN.relax(trav, goals)
        want = heap_dijkstra(trav, goals)
        assert got.dtype == np.uint32 and got.tobytes() == want.tobytes(), shape
    # no goal at all: every traversable cell is UNREACHED
    trav = rng.random((4, 5, 6)) >= 0.3
    got, _ = RN.relax(trav, np.zeros((0, 3), np.int64))
    assert ((got == U) == trav).all() and ((got == BL) == ~trav).all()
    # the weights on an empty box: a face, an edge and a vertex step, and a knight's move
    got, _ = RN.relax(np.ones((3, 3, 4), bool), [(0, 0, 0)])
    assert [int(got[0, 0, 1]), int(got[0, 1, 1]), int(got[1, 1, 1]), int(got[0, 1, 2]), int(got[2, 2, 3])] == [3, 4, 5, 7, 13]


def test_the_sweeps_end_at_scipys_distances():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra

    rng = np.random.default_rng(13)
    for shape in ((12, 16, 20), (8, 24, 24)):
        for share in (0.35, 0.5):
            for n_goals in (1, 2):
                trav, goals = random_scene(rng, shape, share, n_goals)
                nz, ny, nx = trav.shape
                idx = np.arange(trav.size).reshape(trav.shape)
                rows, cols, w = [], [], []
                for dz, dy, dx in RN.STEPS:
                    a = (slice(max(0, -dz), nz - max(0, dz)), slice(max(0, -dy), ny - max(0, dy)), slice(max(0, -dx), nx - max(0, dx)))
                    b = (slice(max(0, dz), nz - max(0, -dz)), slice(max(0, dy), ny - max(0, -dy)), slice(max(0, dx), nx - max(0, -dx)))
                    ok = trav[a] & trav[b]
                    rows.append(idx[a][ok]); cols.append(idx[b][ok]); w.append(np.full(int(ok.sum()), RN.weight((dz, dy, dx))))
                graph = coo_matrix((np.concatenate(w), (np.concatenate(rows), np.concatenate(cols))), shape=(trav.size,) * 2).tocsr()
                d = dijkstra(graph, directed=True, indices=idx[goals[:, 2], goals[:, 1], goals[:, 0]], min_only=True)
                want = np.where(trav.ravel(), np.where(np.isfinite(d), d, U), BL).astype(np.uint32).reshape(trav.shape)
                got, _ = RN.relax(trav, goals)
                assert got.tobytes() == want.tobytes(), (shape, share, n_goals)


def scene(d2, lo=(0, 0, 0), voxel=1.0, origin=(0.0, 0.0, 0.0), R=8, **cfg):
    """a RouteNP over a hand-made clearance array d2 (nz, ny, nx)"""
    d2 = np.asarray(d2, np.uint16)
    G = types.SimpleNamespace(o=np.asarray(origin, np.float64), v=float(voxel))
    K = types.SimpleNamespace(d2=d2, lo=np.asarray(lo, np.int64), n=np.array(d2.shape[::-1], np.int64), R=R, G=G)
    return RN.RouteNP(K, **cfg)


def centre(cell, voxel=1.0):
    return (np.asarray(cell, np.float64) + 0.5) * voxel


def test_need_on_and_just_off_an_integer():
    # voxel 0.5, a corridor whose cells have d2 = 4: q = radius / 0.5, need = ceil(q * q)
    d2 = np.zeros((1, 1, 8), np.uint16)
    d2[0, 0, :] = 4
    d2[0, 0, 3] = 3
    for radius, need, reached in ((0.0, 0, 8), (0.5, 1, 8), (0.8660254037844386, 3, 8), (0.8660254037844387, 4, 3), (1.0, 4, 3),
                                  (1.0000000000000002, 5, 0)):
        N = scene(d2, voxel=0.5)
        assert N.build([centre((0, 0, 0), 0.5)], radius) and N.info()["need"] == need, radius
        assert N.info()["reached_cells"] == reached and N.info()["goals_accepted"] == (1 if reached else 0), radius
    assert [KN.need_d2(r, 0.5, 8) for r in (4.03, 4.04, -0.1, np.nan, np.inf)] == [65, None, None, None, None]
    for bad in (4.04, -0.1, np.nan, np.inf):
        assert not scene(d2, voxel=0.5).build([centre((0, 0, 0), 0.5)], bad)
    # BEYOND passes every need; d2 = 0 passes none, need 0 included
    d2 = np.array([[[KN.BEYOND, 0, KN.BEYOND]]], np.uint16)
    N = scene(d2)
    assert N.build([centre((0, 0, 0))], 8.0) and N.info()["need"] == 64 and N.cost[0, 0].tolist() == [0, BL, U]
    assert N.build([centre((0, 0, 0))], 0.0) and N.cost[0, 0].tolist() == [0, BL, U]


def test_refusals_and_rejected_goals():
    d2 = np.full((4, 8, 32), 9, np.uint16)
    d2[1, 2, 3] = 0
    assert RN.field_bytes((32, 8, 4)) == 4 * 1024 + 8 and RN.field_bytes((33, 9, 5)) == 4 * 33 * 9 * 5 + 8 * 8
    assert not scene(d2, max_bytes=4 * 1024 + 7).build([centre((0, 0, 0))])
    N = scene(d2, lo=(-4, 8, 0), max_bytes=4 * 1024 + 8)
    goals = [centre((-4, 8, 0)), centre((-4, 8, 0)), centre((-1, 10, 1)), centre((-5, 8, 0)), (np.nan, 0, 0), centre((28, 8, 0)),
             (2.0 ** 21, 0, 0)]
    assert N.build(goals)
    info = N.info()
    assert (info["goals_accepted"], info["goals_rejected"]) == (2, 5) and info["lo_cells"] == (-4, 8, 0) and info["n_cells"] == (32, 8, 4)
    assert info["traversable_cells"] == info["reached_cells"] == 1023 and int(N.cost[1, 2, 3]) == BL
    assert N.build(goals[2:]) and N.info()["reached_cells"] == 0 and N.info()["max_cost"] == 0 and N.info()["sum_cost"] == 0
    cost, dist, counts = N.points([centre((-4, 8, 0)), centre((-1, 10, 1)), centre((-5, 8, 0)), (np.nan, 0, 0)])
    assert cost.tolist() == [U, BL, OUT, OUT] and counts.tolist() == [0, 1, 1, 2] and dist[0] == np.inf and np.isnan(dist[1:]).all()
    assert N.paths([centre((0, 9, 0))], 0) is None and scene(d2, max_bytes=4 * 1024 + 8).paths(np.zeros((10, 3)), 18) is None


def check_paths(N, starts, max_cells):
    """every property the contract gives a path; -> what paths() returned"""
    status, count, cost, centres = N.paths(starts, max_cells)
    cells, valid = N.cells_of(starts)
    for i in range(len(cells)):
        if status[i] not in (RN.PATH_REACHED, RN.PATH_TRUNCATED):
            assert count[i] == 0 and (centres[i] == 0.0).all()
            continue
        walk = np.floor((centres[i, :count[i]] - N.K.G.o) / N.K.G.v).astype(np.int64)
        assert (walk[0] == cells[i]).all()                                             # the first cell is the start's
        along = N.value(walk, np.ones(len(walk), bool))
        assert along[0] == cost[i] and (np.diff(along) < 0).all()                      # the costs strictly fall
        steps = np.abs(np.diff(walk, axis=0))
        assert (steps.max(axis=1) == 1).all() if len(steps) else True
        assert (-np.diff(along) == 2 + (steps != 0).sum(axis=1)).all()                 # each step's weight is the cost difference
        assert count[i] <= cost[i] // 3 + 1
        if status[i] == RN.PATH_REACHED:
            assert along[-1] == 0
        else:
            assert count[i] == max_cells and along[-1] > 0
        assert (centres[i, count[i]:] == 0.0).all()
    return status, count, cost, centres


def test_every_path_descends_to_a_goal():
    rng = np.random.default_rng(17)
    d2 = np.where(rng.random((10, 14, 18)) < 0.3, 0, 5).astype(np.uint16)
    N = scene(d2, lo=(-5, 3, -2), voxel=0.25, origin=(0.1, -0.2, 0.3))
    free = np.argwhere(d2 > 0)[:, ::-1] + N.K.lo
    assert N.build(N.K.G.o + (free[:2] + 0.5) * 0.25)
    starts = N.K.G.o + (np.concatenate([free[::7], np.argwhere(d2 == 0)[:5, ::-1] + N.K.lo, [[-6, 3, -2]]]) + 0.5) * 0.25
    status, count, cost, centres = check_paths(N, starts, 64)
    assert set(status.tolist()) >= {RN.PATH_REACHED, RN.PATH_BLOCKED, RN.PATH_OUTSIDE} and RN.PATH_TRUNCATED not in status
    longest = int(count.max())
    assert longest > 4
    # max_cells exactly the longest path's length, one less (the prefix equal), and 1
    for m in (longest, longest - 1, 1):
        s2, c2, cost2, cen2 = check_paths(N, starts, m)
        assert (cost2 == cost).all() and (cen2 == centres[:, :m]).all() and (c2 == np.minimum(count, m)).all()
        assert ((s2 == RN.PATH_TRUNCATED) == (count > m)).all()
    # a start on a goal: one waypoint
    s, c, k, cen = N.paths(N.K.G.o + (free[:1] + 0.5) * 0.25, 5)
    assert (s[0], c[0], k[0]) == (RN.PATH_REACHED, 1, 0)
    # a damaged field cannot make the walk loop: a plateau has no neighbour with c + w == k
    N.cost[...] = np.where(N.cost < OUT, 7, N.cost)
    s, c, _, _ = N.paths(starts[:3], 64)
    assert (s == RN.PATH_TRUNCATED).all() and (c == 1).all()


def test_a_tie_the_order_decides():
    """an open 9 x 1 x 1 line with goals at both ends and the start in the middle: both neighbours have cost 9 = 12 - 3, and
    dx = -1 comes before dx = +1; in a 5 x 5 plane with goals at two opposite corners of the start, (dy, dx) = (-1, -1) wins"""
    N = scene(np.full((1, 1, 9), 5, np.uint16))
    assert N.build([centre((0, 0, 0)), centre((8, 0, 0))])
    assert N.cost[0, 0].tolist() == [0, 3, 6, 9, 12, 9, 6, 3, 0]
    status, count, cost, centres = N.paths([centre((4, 0, 0))], 9)
    assert (status[0], count[0], cost[0]) == (RN.PATH_REACHED, 5, 12)
    assert centres[0, :5, 0].tolist() == [4.5, 3.5, 2.5, 1.5, 0.5]                      # towards x = 0: dx = -1 is first
    N = scene(np.full((1, 5, 5), 5, np.uint16))
    assert N.build([centre((0, 0, 0)), centre((4, 4, 0)), centre((4, 0, 0)), centre((0, 4, 0))])
    status, count, cost, centres = N.paths([centre((2, 2, 0))], 9)
    assert (status[0], count[0], cost[0]) == (RN.PATH_REACHED, 3, 8)
    assert centres[0, :3, :2].tolist() == [[2.5, 2.5], [1.5, 1.5], [0.5, 0.5]]          # dy = -1 before +1, then dx = -1
    # along z: goals above and below, dz = -1 wins
    N = scene(np.full((5, 1, 1), 5, np.uint16))
    assert N.build([centre((0, 0, 0)), centre((0, 0, 4))])
    assert N.paths([centre((0, 0, 2))], 9)[3][0, :3, 2].tolist() == [2.5, 1.5, 0.5]


def test_the_columns_form_is_the_field_of_one_layer():
    rng = np.random.default_rng(19)
    d2 = np.where(rng.random((1, 24, 40)) < 0.3, 0, 3).astype(np.uint16)
    N = scene(d2)
    free = np.argwhere(d2[0] > 0)[:, ::-1]
    goal = np.array([free[0][0], free[0][1], 0])
    assert N.build([centre(goal)])
    flat = heap_dijkstra(d2 > 0, [goal])
    assert N.cost.tobytes() == flat.tobytes()
    reached = N.cost[N.cost < OUT]
    assert ((reached % 1) == 0).all() and int(N.cost[0, free[0][1], free[0][0]]) == 0
    # only 3 and 4 occur as steps: no cost of 1, 2 or 5
    assert not np.isin(reached, (1, 2, 5)).any() and np.isin(reached, (3, 4)).any()


@pytest.fixture(scope="module")
def wall():
    poses, clouds, _, _ = LS.wall()
    V = CN.build_map(poses, clouds, CS.MASK, 0.5)
    G = FN.FreeNP(V, max_range=12.0, end_margin=1.0)
    assert G.reset(poses=poses)
    G.add_keyframes(poses, clouds, CS.MASK)
    return G


GOAL = np.array([[6.25, 0.25, 1.25]])       # the wall scene's sensor cell (12, 0, 2)
# (unknown_is_obstacle, radius) -> goals accepted, traversable, reached, sum_cost, max_cost at R = 8, voxel 0.5
# (radius 0 and radius = voxel both give max(need, 1) = 1: the same field; at two voxels with unknown an obstacle the sensor's own
# cell is too close to unknown space and the goal is rejected)
WALL_TABLE = {(0, 0.0): (1, 238161, 238161, 22807412, 177), (0, 0.5): (1, 238161, 238161, 22807412, 177),
              (0, 1.0): (1, 237607, 237607, 22799964, 177), (1, 0.0): (1, 875, 875, 23929, 48), (1, 0.5): (1, 875, 875, 23929, 48),
              (1, 1.0): (0, 219, 0, 0, 0)}


def test_the_wall(wall):
    got = {}
    for wrap in (0, 1):
        K = KN.ClearNP(wall, max_distance=4.0, unknown_is_obstacle=wrap)
        assert K.build() and K.R == 8
        for radius in (0.0, 0.5, 1.0):
            N = RN.RouteNP(K)
            assert N.build(GOAL, radius)
            info = N.info()
            assert info["need"] == round(4 * radius * radius) and info["n_cells"] == (76, 56, 56) and info["bytes"] == 4 * 76 * 56 * 56 + 8 * 3 * 7 * 14
            got[(wrap, radius)] = (info["goals_accepted"], info["traversable_cells"], info["reached_cells"], info["sum_cost"], info["max_cost"])
            if not info["goals_accepted"]:
                continue
            reached = np.argwhere(N.cost < OUT)[::max(info["reached_cells"] // 40, 1), ::-1] + K.lo
            starts = np.concatenate([wall.o + (reached + 0.5) * wall.v, GOAL])
            status, count, cost, _ = check_paths(N, starts, info["max_cost"] // 3 + 1)
            assert (status == RN.PATH_REACHED).all() and count[-1] == 1 and count.max() > 10
    assert got == WALL_TABLE
