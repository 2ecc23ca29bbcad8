"""-m gpu: the route through the closed map (tl_route.hip, tl_api_route.hip) against its numpy restatement
(tests/closed_map_route_np.py), bit for bit: every byte of the field, the info without its four diagnostics, every cost,
distance, status, waypoint and counter.  The scenes and helpers are tests/test_gpu_closed_map_clearance.py's; a hand-made maze is
voxels as walls in a caller-given box with unknown_is_obstacle = 0, so the box's faces close it and every other cell is open.

The device's tile is 32 x 8 x 4 cells (x, y, z) and it relaxes a tile at most 64 times in LDS before it hands it to the next
round; the shapes below are chosen around those numbers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_carve_np as CN  # noqa: E402
import closed_map_clearance_np as KN  # noqa: E402
import closed_map_route_np as RN  # noqa: E402
import diff_scenes as DS  # noqa: E402
import localise_scenes as LS  # noqa: E402
import test_gpu_closed_map_clearance as TK  # noqa: E402
import test_gpu_closed_map_free as TF  # noqa: E402
import test_gpu_closed_map_localise as TL  # noqa: E402
import test_gpu_closed_map_surfel as TS  # noqa: E402
from tloam_amd import map_io  # noqa: E402

pytestmark = pytest.mark.gpu

bits, invalid, not_ready, built, log_bytes = TF.bits, TF.invalid, TF.not_ready, TF.built, TF.log_bytes
hand_map, boxed, cleared, wall = TK.hand_map, TK.boxed, TK.cleared, TK.wall
U, BL, OUT = RN.UNREACHED, RN.BLOCKED, RN.OUTSIDE
GOAL = np.array([[6.25, 0.25, 1.25]])       # the wall scene's sensor cell


def hip_error(reg, what):
    return pytest.raises(reg.TloamHipError, match=what)


def plain(info):
    return {k: v for k, v in info.items() if k not in RN.DIAGNOSTICS}


def same_field(H, N, info=None):
    """the device's field and info (without the diagnostics) are the restatement's"""
    got = H.closed_map_route_info()
    if info is not None:
        assert plain(info) == plain(got)
    assert plain(got) == N.info(), (plain(got), N.info())
    assert got["rounds"] >= 1 and got["waits"] >= 2 and got["launches"] >= 4 and got["tile_updates"] >= min(got["goals_accepted"], 1)
    cost = H.closed_map_route_field()
    assert cost.dtype == np.uint32 and cost.shape == N.cost.shape
    assert cost.tobytes() == N.cost.tobytes(), np.argwhere(cost != N.cost)[:5]
    return got


def routed(H, K, goals, radius=0.0, pose=None, **cfg):
    """the field built on the device and in the restatement -> (N, info)"""
    if cfg:
        H.closed_map_route_configure(**cfg)
    N = RN.RouteNP(K, **cfg)
    assert N.build(goals, radius, pose)
    info = H.closed_map_route_build(goals, radius, pose)
    print(f"radius {radius} {cfg}: {info}")
    return N, same_field(H, N, info)


def same_points(H, N, pts, pose=None):
    cost, dist, counts = H.closed_map_route_points(pts, pose)
    wc, wd, wn = N.points(pts, pose)
    assert cost.dtype == np.uint32 and dist.dtype == np.float64
    assert cost.tobytes() == wc.tobytes() and bits(dist) == bits(wd) and counts.tobytes() == wn.tobytes()
    return cost, dist, counts


def same_paths(H, N, starts, max_cells, pose=None):
    status, count, cost, centres = H.closed_map_route_paths(starts, max_cells, pose)
    ws, wn, wc, wcen = N.paths(starts, max_cells, pose)
    assert status.dtype == np.uint8 and count.dtype == np.int32 and cost.dtype == np.uint32 and centres.shape == (len(ws), max_cells, 3)
    assert status.tobytes() == ws.tobytes() and count.tobytes() == wn.tobytes() and cost.tobytes() == wc.tobytes()
    assert bits(centres) == bits(wcen)
    return status, count, cost, centres


def centres_of(K, cells):
    return K.G.o + (np.asarray(cells, np.float64).reshape(-1, 3) + 0.5) * K.G.v


def cells_where(K, mask):
    """the cells (m, 3) of the box where mask (nz, ny, nx) holds"""
    return np.argwhere(mask)[:, ::-1] + K.lo


def same_queries(H, N, seed=1, n=600, misses=None):
    """points in the map frame and under a pose, and paths from all over the box, are the restatement's; every returned path
    keeps the clearance it was promised"""
    K = N.K
    rng = np.random.default_rng(seed)
    pts = TF.probes(K.G, rng, misses, n=n)
    cost, _, counts = same_points(H, N, pts)
    lo, hi = TK.box_metric(K.G)
    pose = LS.offset(np.eye(4), 0.7, 0.4)
    pose[:3, 3] += 0.5 * (lo + hi)
    local = np.ascontiguousarray((pts[:-5] - pose[:3, 3]) @ pose[:3, :3])
    same_points(H, N, local, pose)
    assert H.closed_map_route_points(pts, want_distance=False)[1] is None
    reached = cost[cost < OUT]
    m = int(reached.max()) // 3 + 1 if len(reached) else 1
    status, count, _, centres = same_paths(H, N, pts[:: max(len(pts) // 65, 1)][:65], m)
    assert RN.PATH_TRUNCATED not in status                      # a whole path has at most cost / 3 + 1 cells
    same_paths(H, N, local[:: max(len(local) // 33, 1)][:33], max(m // 2, 1), pose)
    paths_keep_their_clearance(H, N, status, count, centres)
    return cost, counts


def paths_keep_their_clearance(H, N, status, count, centres):
    """Every waypoint's own cell has d2 >= max(need, 1): that is all the contract promises of a path -- moves have no corner
    rule, so the straight piece between two diagonal neighbours passes exactly through the shared edge or corner, and the two
    (or six) face-adjacent cells the segment walk may step through there can be walls.  A face step's segment visits the two
    cells alone: there the walk of tloam_closed_map_clearance_segments at radius 0 must report min_d2 >= max(need, 1)."""
    need = max(N.info()["need"], 1)
    a, b = [], []
    for i in np.flatnonzero(count > 1):
        a.append(centres[i, :count[i] - 1])
        b.append(centres[i, 1:count[i]])
    way = np.concatenate([centres[i, :count[i]] for i in np.flatnonzero(count > 0)] or [np.zeros((0, 3))])
    if len(way):
        d2 = H.closed_map_clearance_points(way)[1]
        assert (d2 >= need).all()
    if a:
        a, b = np.concatenate(a), np.concatenate(b)
        face = (np.abs(a - b) > 0.25 * N.K.G.v).sum(axis=1) == 1
        if face.any():
            st, least, _, _ = H.closed_map_clearance_segments(a[face], b[face], 0.0)
            assert (st == KN.CLEAR).all() and (least >= need).all()


# ---- the wall --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrap, radius, want", [(0, 0.0, (1, 238161, 238161, 22807412, 177)), (0, 0.5, (1, 238161, 238161, 22807412, 177)),
                                                (1, 0.0, (1, 875, 875, 23929, 48)), (1, 0.5, (1, 875, 875, 23929, 48))])
def test_the_wall(wall, tmp_path, wrap, radius, want):
    H, V, G, _, _, scan, truth = wall
    K, _ = cleared(H, G, max_distance=4.0, unknown_is_obstacle=wrap)
    N, info = routed(H, K, GOAL, radius)
    assert (info["goals_accepted"], info["traversable_cells"], info["reached_cells"], info["sum_cost"], info["max_cost"]) == want
    assert info["n_cells"] == (76, 56, 56) and info["bytes"] == 4 * 76 * 56 * 56 + 8 * 3 * 7 * 14 and info["need"] == round(4 * radius * radius)
    same_queries(H, N)
    # two builds give the same bytes; so do goals given in a pose's sensor frame
    before = H.closed_map_route_field().tobytes()
    assert plain(H.closed_map_route_build(GOAL, radius)) == plain(info) and H.closed_map_route_field().tobytes() == before
    pose = LS.offset(np.eye(4), 0.3, -0.2)
    pose[:3, 3] = [5.0, 1.0, 1.0]
    goals = np.concatenate([GOAL, GOAL + [[1.0, -2.0, 0.0]]])
    N2, _ = routed(H, K, np.ascontiguousarray((goals - pose[:3, 3]) @ pose[:3, :3]), radius, pose)
    same_queries(H, N2, seed=2, n=300)
    if wrap == 1 and radius == 0.0:
        # the PCD exports, read back
        routed(H, K, GOAL, radius)
        for ascii in (False, True):
            path = str(tmp_path / f"route{int(ascii)}.pcd")
            cen = G.free_cells()
            assert map_io.write_route_pcd(path, H, ascii=ascii) == 875
            c2, dist = map_io.read_route_pcd(path)
            assert bits(c2) == bits(cen) and bits(dist) == bits(N.points(cen)[1]) and np.isfinite(dist).all()
            status, count, cost, centres = N.paths(cen[::100], 20)
            path = str(tmp_path / f"paths{int(ascii)}.pcd")
            assert map_io.write_route_paths_pcd(path, H, cen[::100], 20, ascii=ascii) == int(count.sum())
            way, index = map_io.read_route_paths_pcd(path)
            assert bits(way) == bits(np.concatenate([centres[i, :count[i]] for i in range(len(count))]))
            assert index.tolist() == [i for i in range(len(count)) for _ in range(count[i])]


@pytest.mark.parametrize("n", [1, 2, 64, 1025])
def test_goal_batches(wall, n):
    H, V, G, _, _, scan, truth = wall
    K, _ = cleared(H, G, max_distance=4.0, unknown_is_obstacle=1)
    rng = np.random.default_rng(n)
    cen = G.free_cells()
    goals = np.concatenate([cen[rng.integers(0, len(cen), n - n // 3)], rng.uniform(-2.0, 14.0, (n // 3, 3))])[:n]
    N, info = routed(H, K, goals)
    assert info["goals_accepted"] + info["goals_rejected"] == n and info["goals_accepted"] >= n - n // 3
    same_queries(H, N, n=200)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_path_batches(wall, n):
    H, V, G, _, _, scan, truth = wall
    K, _ = cleared(H, G, max_distance=4.0, unknown_is_obstacle=1)
    N, info = routed(H, K, GOAL)
    cen = G.free_cells()
    far = cen[np.argmax(N.points(cen)[0])]                                            # a start with the longest path
    starts = np.concatenate([[far], cen[:: max(len(cen) // n, 1)]])[:n]
    full = info["max_cost"] // 3 + 1
    status, count, cost, centres = same_paths(H, N, starts, full)
    assert (status == RN.PATH_REACHED).all() and cost[0] == info["max_cost"]
    longest = int(count.max())
    for m in (longest, longest - 1, 1):                                               # exactly the length, one less, one
        s2, c2, k2, cen2 = same_paths(H, N, starts, m)
        assert ((s2 == RN.PATH_TRUNCATED) == (count > m)).all() and (k2 == cost).all() and bits(cen2) == bits(centres[:, :m])
    # starts in a wall, outside the box, no cell at all, and on the goal
    odd = np.concatenate([centres_of(K, cells_where(K, K.d2 == 0)[:1]), [[6.0, 40.0, 1.5]], [[np.nan, 0.0, 0.0]], GOAL, starts])[:max(n, 4)]
    status, count, cost, _ = same_paths(H, N, odd, 7)
    assert status[:4].tolist() == [RN.PATH_BLOCKED, RN.PATH_OUTSIDE, RN.PATH_OUTSIDE, RN.PATH_REACHED]
    assert count[:4].tolist() == [0, 0, 0, 1] and cost[:4].tolist() == [BL, OUT, OUT, 0]
    same_paths(H, N, np.ascontiguousarray(starts - truth[:3, 3]) @ truth[:3, :3], longest, truth)


# ---- hand-made mazes --------------------------------------------------------------------------------------------------------------
def maze(reg, walls, lo, hi, **clear_cfg):
    """-> (H, K): voxels `walls` in the box [lo, hi] (cells), every other cell open"""
    H, V = hand_map(reg, walls)
    G = boxed(H, V, lo, hi)
    K, _ = cleared(H, G, unknown_is_obstacle=0, **clear_cfg)
    return H, K


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_long_corridors(hip_module, axis):
    """a 4 x 4 x 600 box and its turns, no wall at all: the goal at one end, every tile seam crossed in sequence (19, 75 and 150
    tiles along x, y and z); then goals at both ends; then max_rounds = 1 and the two extremes of rounds_per_wait"""
    reg = hip_module
    hi = np.full(3, 3, np.int64)
    hi[axis] = 599
    e = np.eye(3, dtype=np.int64)[axis]
    H, K = maze(reg, np.zeros((0, 3), np.int64), (0, 0, 0), hi)
    one = centres_of(K, [1, 2, 3] * (1 - e))
    N, info = routed(H, K, one)
    assert info["reached_cells"] == 16 * 600 and info["max_cost"] >= 3 * 599
    first = H.closed_map_route_field().tobytes()
    same_queries(H, N, n=300)
    both = np.concatenate([one, centres_of(K, [1, 2, 3] * (1 - e) + 599 * e)])
    N2, info2 = routed(H, K, both)
    assert info2["max_cost"] < info["max_cost"] // 2 + 12
    same_queries(H, N2, n=300)
    # max_rounds = 1: the build fails, names the cap and drops the field; a rebuild with the defaults is the first
    H.closed_map_route_configure(max_rounds=1)
    with hip_error(reg, "max_rounds = 1"):
        H.closed_map_route_build(one)
    assert H.closed_map_route_info() == reg.RouteInfo().as_dict()
    with not_ready(reg):
        H.closed_map_route_field()
    H.closed_map_route_configure()
    assert plain(H.closed_map_route_build(one)) == plain(info) and H.closed_map_route_field().tobytes() == first
    for per_wait in (1, 1024):
        H.closed_map_route_configure(rounds_per_wait=per_wait)
        got = H.closed_map_route_build(one)
        assert plain(got) == plain(info) and H.closed_map_route_field().tobytes() == first
        assert got["waits"] == (got["rounds"] + 1 if per_wait == 1 else 2)
    H.close()


def serpentine():
    """one tile, 32 x 8 x 4: in the layers z = 0 and z = 2 the rows y = 0, 2, 4, 6 are corridors joined at alternating ends,
    the layers z = 1 and z = 3 are solid but for the hole (0, 6, 1) that joins the two -> (walls, the path's two ends)"""
    walls = []
    for z in range(4):
        for y in range(8):
            for x in range(32):
                if z in (1, 3):
                    open_ = (x, y, z) == (0, 6, 1)
                elif y % 2 == 0:
                    open_ = True
                else:
                    open_ = y < 7 and x == (31 if y % 4 == 1 else 0)
                if not open_:
                    walls.append((x, y, z))
    return np.array(walls, np.int64), (0, 0, 0), (0, 0, 2)


def test_a_serpentine_in_one_tile(hip_module):
    """263 open cells and a path of 249 inside a single tile: longer than the 64 passes a tile gets in LDS per round, so the tile meets the cap
    and hands itself to the next round (the rounds are printed: they are a diagnostic)"""
    walls, a, b = serpentine()
    H, K = maze(hip_module, walls, (0, 0, 0), (31, 7, 3))
    N, info = routed(H, K, centres_of(K, a))
    assert info["traversable_cells"] == info["reached_cells"] == 32 * 8 * 4 - len(walls) and info["n_cells"] == (32, 8, 4)
    status, count, cost, _ = same_paths(H, N, centres_of(K, b), 400)
    assert status[0] == RN.PATH_REACHED and count[0] == 249 and cost[0] == info["max_cost"]
    same_queries(H, N, n=200)
    H.close()


def test_a_u_turn_through_the_neighbouring_tile(hip_module):
    """two tiles along x; a wall at y = 1 from x = 0 to 39 at every z: from the goal at (0, 0, 0) the cells (0, 2 .., .) of the
    same tile are reached only through the second tile, so the first is relaxed a second time"""
    walls = [(x, 1, z) for x in range(40) for z in range(4)]
    H, K = maze(hip_module, walls, (0, 0, 0), (63, 7, 3))
    N, info = routed(H, K, centres_of(K, (0, 0, 0)))
    assert info["reached_cells"] == 64 * 8 * 4 - 160 and info["tile_updates"] >= 3
    assert int(N.cost[0, 2, 0]) > 3 * 79
    same_queries(H, N, n=200)
    H.close()


def test_a_diagonal_across_a_tile_corner(hip_module):
    """2 x 2 x 2 tiles of which only the chain (28 + k, 4 + k, k), k = 0 .. 7, is open: between k = 3 and k = 4 it crosses the
    corner (32, 8, 4) by a vertex step, and only the mark of the vertex-neighbour tile carries the cost on"""
    chain = {(28 + k, 4 + k, k) for k in range(8)}
    walls = [(x, y, z) for z in range(8) for y in range(12) for x in range(36) if (x, y, z) not in chain]
    H, K = maze(hip_module, walls, (0, 0, 0), (35, 11, 7))
    N, info = routed(H, K, centres_of(K, (28, 4, 0)))
    assert info["reached_cells"] == info["traversable_cells"] == 8 and info["max_cost"] == 35 and info["sum_cost"] == 5 * 28
    status, count, cost, _ = same_paths(H, N, centres_of(K, (35, 11, 7)), 8)
    assert (status[0], count[0], cost[0]) == (RN.PATH_REACHED, 8, 35)
    same_queries(H, N, n=200)
    # ... and across the edges: chains in a plane, (28 + k, 4 + k, 1) and (28 + k, 5, k)
    for chain in ({(28 + k, 4 + k, 1) for k in range(8)}, {(28 + k, 5, k) for k in range(8)}, {(30, 4 + k, k) for k in range(8)}):
        cells = sorted(chain)
        walls = [(x, y, z) for z in range(8) for y in range(12) for x in range(36) if (x, y, z) not in chain]
        H2, K2 = maze(hip_module, walls, (0, 0, 0), (35, 11, 7))
        _, info = routed(H2, K2, centres_of(K2, cells[0]))
        assert info["reached_cells"] == 8 and info["max_cost"] == 28
        H2.close()
    H.close()


def test_box_shapes(hip_module):
    shapes = [((0, 0, 0), (3, 3, 3)),            # one brick
              ((-8, -4, -12), (-1, -1, -5)),     # at negative cells
              ((-6, -3, -2), (9, 4, 5)),         # straddling 0, lo not a multiple of 4
              ((1, 2, 3), (70, 9, 6)),           # lo not a multiple of 4; three tiles along x, the last 8 cells wide
              ((0, 0, 0), (39, 19, 3)),          # one tile thick; sides that are no multiple of the tile
              ((0, 0, 0), (35, 11, 9))]          # every axis with a partial last tile
    for lo, hi in shapes:
        blo, bhi = 4 * (np.array(lo) >> 2), 4 * (np.array(hi) >> 2) + 3      # the box the bricks make
        n = bhi - blo + 1
        rng = np.random.default_rng(int(n.prod()))
        walls = blo + np.argwhere(rng.random(n) < 0.25)
        H, K = maze(hip_module, walls, lo, hi)
        open_ = cells_where(K, K.d2 > 0)
        goals = centres_of(K, np.concatenate([open_[:1], open_[-1:], blo[None] - 1]))      # two corners' ends and one outside
        N, info = routed(H, K, goals)
        assert info["lo_cells"] == tuple(blo) and info["n_cells"] == tuple(n) and info["goals_accepted"] == 2 and info["goals_rejected"] == 1
        same_queries(H, N, n=300)
        # the column form over the same box: a band of one layer and of all of them
        for z_lo, z_hi in ((float(blo[2]) + 0.5, float(blo[2]) + 0.5), (-1e6, 1e6)):
            same_columns(H, N, z_lo, z_hi, goals, 0.0)
        H.close()


def same_columns(H, N, z_lo, z_hi, goals, radius, min_free=1, pose=None):
    state, d2, cost, info = H.closed_map_route_columns(z_lo, z_hi, goals, radius, min_free, pose)
    ws, wd, wc, winfo = N.columns(z_lo, z_hi, goals, radius, min_free, pose)
    assert state.tobytes() == ws.tobytes() and d2.tobytes() == wd.tobytes() and cost.dtype == np.uint32 and cost.shape == wc.shape
    assert cost.tobytes() == wc.tobytes() and plain(info) == winfo, (plain(info), winfo)
    assert state.tobytes() == H.closed_map_clearance_columns(z_lo, z_hi, min_free)[0].tobytes()
    return cost, info


def test_a_door_and_a_closed_pocket(hip_module):
    """a wall at x = 10 with a door three cells wide (y = 4 .. 6, every z): the door's centre cells have d2 = 4, so a body of
    radius 2 voxels (need 4) passes and one a step above (need 5) does not; a second wall at x = 16 without a door closes a
    pocket behind it"""
    reg = hip_module
    walls = [(10, y, z) for y in range(12) for z in range(8) if not 4 <= y <= 6] + [(16, y, z) for y in range(12) for z in range(8)]
    H, K = maze(reg, walls, (0, 0, 0), (23, 11, 7), max_distance=4.0)
    goal, behind, pocket = centres_of(K, (3, 5, 4)), centres_of(K, (13, 5, 4)), centres_of(K, (20, 5, 4))
    assert int(K.d2[4, 5, 10]) == 4
    for radius, passes in ((0.0, True), (1.0, True), (2.0, True), (2.0000001, False), (3.0, False)):
        N, info = routed(H, K, goal, radius)
        cost = same_points(H, N, np.concatenate([goal, behind, pocket]))[0]
        assert cost[0] == 0 and (cost[1] < OUT) == passes and cost[1] in ((30,) if passes else (U, BL)), (radius, cost)
        assert cost[2] in (U, BL)
        status = same_paths(H, N, np.concatenate([behind, pocket]), 40)[0]
        assert status[0] == (RN.PATH_REACHED if passes else RN.PATH_UNREACHED) or cost[1] == BL
        same_queries(H, N, n=200)
    N, _ = routed(H, K, goal, 0.0)
    status, count, cost, _ = same_paths(H, N, pocket, 40)
    assert (status[0], count[0], cost[0]) == (RN.PATH_UNREACHED, 0, U)
    # rejected goals: in a wall, outside the box, NaN; with all of them rejected the build is OK and nothing is reached
    bad = np.concatenate([centres_of(K, (10, 0, 0)), centres_of(K, (24, 0, 0)), [[np.nan, 0.0, 0.0]], [[0.0, 2.0 ** 21, 0.0]]])
    N, info = routed(H, K, bad)
    assert (info["goals_accepted"], info["goals_rejected"], info["reached_cells"], info["sum_cost"], info["max_cost"]) == (0, 4, 0, 0, 0)
    assert info["traversable_cells"] == 24 * 12 * 8 - len(walls) and set(np.unique(H.closed_map_route_field()).tolist()) == {U, BL}
    assert same_paths(H, N, goal, 5)[0][0] == RN.PATH_UNREACHED
    N, info = routed(H, K, np.concatenate([bad, goal, goal]))
    assert (info["goals_accepted"], info["goals_rejected"]) == (2, 4)
    # a hand-made 2-D maze: the columns of the same walls, the band anywhere
    for radius in (0.0, 2.0, 2.0000001):
        cost, info = same_columns(H, N, 0.5, 3.5, np.concatenate([goal, bad]), radius)
        assert info["n_cells"] == (24, 12, 1) and info["goals_accepted"] == 1 and (cost[5, 13] < OUT) == (radius <= 2.0)
        assert cost[5, 20] == U
    H.close()


def test_the_walls_columns(wall):
    H, V, G, _, _, scan, truth = wall
    for wrap in (0, 1):
        K, _ = cleared(H, G, max_distance=4.0, unknown_is_obstacle=wrap)
        N = RN.RouteNP(K)
        for band in ((0.5, 2.9, 1), (-1.0, 0.7, 2), (-1e6, 1e6, 3), (1e4, 1e4 + 10.0, 1)):
            for radius in (0.0, 0.5):
                same_columns(H, N, band[0], band[1], GOAL, radius, band[2])
        pose = LS.offset(np.eye(4), 0.3, -0.2)
        pose[:3, 3] = [5.0, 1.0, 1.0]
        same_columns(H, N, 0.5, 2.9, np.ascontiguousarray((GOAL - pose[:3, 3]) @ pose[:3, :3]), 0.5, 1, pose)


# ---- lifetime ----------------------------------------------------------------------------------------------------------------------
def test_what_drops_the_field(hip_module):
    reg = hip_module
    poses, clouds, scan, truth = LS.wall()
    v = CS.GHOST["voxel"]
    H, V = built(reg, poses, clouds, CS.MASK, v)
    zero = reg.RouteInfo().as_dict()
    assert H.closed_map_route_info() == zero
    with not_ready(reg):
        H.closed_map_route_build(GOAL)                                                # no grid
    H.closed_map_free_configure(**TF.WALL)
    H.closed_map_free_build()
    with not_ready(reg):
        H.closed_map_route_build(GOAL)                                                # no clearance field
    H.closed_map_route_columns(0.5, 2.9, GOAL)                                        # (computed from the grid: no field needed)
    cfg = dict(max_distance=4.0, unknown_is_obstacle=1)
    H.closed_map_clearance_configure(**cfg)
    H.closed_map_clearance_build()

    def gone():
        assert H.closed_map_route_info() == zero
        for call in (H.closed_map_route_field, lambda: H.closed_map_route_points(scan), lambda: H.closed_map_route_paths(scan[:5], 4)):
            with not_ready(reg):
                call()
        return True

    assert gone()
    info = H.closed_map_route_build(GOAL, 0.5)
    field = H.closed_map_route_field().tobytes()
    clearance = H.closed_map_clearance_field().tobytes()
    H.closed_map_route_columns(0.5, 2.9, GOAL)                                        # leaves the built field alone
    assert plain(H.closed_map_route_info()) == plain(info) and H.closed_map_route_field().tobytes() == field
    drops = [H.closed_map_route_configure, H.closed_map_clearance_build, lambda: H.closed_map_clearance_configure(**cfg),
             H.closed_map_free_add_keyframes, lambda: H.closed_map_free_add_scan(scan[:50], truth), H.closed_map_carve,
             lambda: H.closed_map_carve_configure(max_range=11.0), H.closed_map_free_reset,
             lambda: H.closed_map_free_configure(**TF.WALL)]
    for k, drop in enumerate(drops):
        drop()
        assert gone(), k
        H.closed_map_free_build()                                                     # back to the keyframes' grid
        H.closed_map_clearance_build()
        assert H.closed_map_clearance_field().tobytes() == clearance, k
        assert plain(H.closed_map_route_build(GOAL, 0.5)) == plain(info) and H.closed_map_route_field().tobytes() == field, k
    # a fresh context gives the same bytes; the configuration persists across an odometry reset
    F, _ = built(reg, poses, clouds, CS.MASK, v)
    F.closed_map_free_configure(**TF.WALL)
    F.closed_map_free_build()
    F.closed_map_clearance_configure(**cfg)
    F.closed_map_clearance_build()
    F.closed_map_route_configure(rounds_per_wait=3)
    got = F.closed_map_route_build(GOAL, 0.5)
    assert plain(got) == plain(info) and F.closed_map_route_field().tobytes() == field
    blob = F.closed_map_save()
    F.closed_map_load(blob)
    assert F.closed_map_route_info() == zero
    F.odometry_reset(None, TS.TC.odom_cfg(reg))
    assert F.closed_map_route_info() == zero
    for k in range(len(poses)):
        assert F.place_add_scan(TS.DUMMY, np.eye(4), k) == k
        F.place_set_keyframe_clouds(k, *clouds[k])
    F.closed_map_build(2, poses)
    F.closed_map_free_build()
    F.closed_map_clearance_build()
    again = F.closed_map_route_build(GOAL, 0.5)
    assert plain(again) == plain(info) and F.closed_map_route_field().tobytes() == field
    assert again["waits"] == -(-again["rounds"] // 3) + 1                             # rounds_per_wait 3: still there
    H.close(); F.close()


def test_refusals_leave_the_field(wall, hip_module):
    reg = hip_module
    H, V, G, poses, clouds, scan, truth = wall
    K, _ = cleared(H, G, max_distance=4.0, unknown_is_obstacle=1)
    H.closed_map_route_configure()
    N, info = routed(H, K, GOAL, 0.5)
    field = H.closed_map_route_field().tobytes()

    def untouched():
        return H.closed_map_route_field().tobytes() == field and H.closed_map_route_info() == info

    for bad in (dict(max_bytes=3), dict(max_bytes=-1), dict(max_rounds=0), dict(max_rounds=-5), dict(rounds_per_wait=0),
                dict(rounds_per_wait=1025), dict(rounds_per_wait=-1)):
        with invalid(reg):
            H.closed_map_route_configure(**bad)
    with pytest.raises(KeyError):
        H.closed_map_route_configure(radius=1.0)
    assert untouched()
    for radius in (-0.5, float("nan"), float("inf"), 4.04, 1e200):
        with invalid(reg):
            H.closed_map_route_build(GOAL, radius)
        with invalid(reg):
            H.closed_map_route_columns(0.5, 2.9, GOAL, radius)
    for bad_pose in (2.0 * np.eye(4), np.full((4, 4), np.nan), np.diag([1.0, 1.0, -1.0, 1.0])):
        for call in (lambda: H.closed_map_route_build(GOAL, 0.5, bad_pose), lambda: H.closed_map_route_points(scan, bad_pose),
                     lambda: H.closed_map_route_paths(scan, 5, bad_pose), lambda: H.closed_map_route_columns(0.5, 2.9, GOAL, 0.5, 1, bad_pose)):
            with invalid(reg):
                call()
    with invalid(reg):
        H.closed_map_route_build(np.zeros((0, 3)))
    with invalid(reg):
        H.closed_map_route_paths(scan, 0)
    assert untouched()
    # the raw entry points: NULL arguments, n == 0, ranges
    L = H.L
    n = len(scan)
    flat = np.ascontiguousarray(scan).ctypes.data_as(C.POINTER(C.c_double))
    cost, status, cells = np.full(n, 9, np.uint32), np.full(n, 9, np.uint8), np.full(n, 9, np.int32)
    cen = np.full((n, 2, 3), 9.0)
    cp, sp, ip, dp = (cost.ctypes.data_as(C.POINTER(C.c_uint32)), status.ctypes.data_as(C.POINTER(C.c_uint8)),
                      cells.ctypes.data_as(C.POINTER(C.c_int32)), cen.ctypes.data_as(C.POINTER(C.c_double)))
    assert L.tloam_closed_map_route_build(H.h, None, 1, None, 0.5, None) == -1
    assert L.tloam_closed_map_route_points(H.h, None, n, None, cp, None, None) == -1
    assert L.tloam_closed_map_route_points(H.h, flat, 0, None, cp, None, None) == -1
    assert L.tloam_closed_map_route_points(H.h, flat, n, None, None, None, None) == -1
    for args in ((None, n, None, 2, sp, ip, cp, dp), (flat, 0, None, 2, sp, ip, cp, dp), (flat, n, None, 0, sp, ip, cp, dp),
                 (flat, n, None, 2, None, ip, cp, dp), (flat, n, None, 2, sp, None, cp, dp), (flat, n, None, 2, sp, ip, None, dp),
                 (flat, n, None, 2, sp, ip, cp, None)):
        assert L.tloam_closed_map_route_paths(H.h, *args) == -1
    assert (cost == 9).all() and (status == 9).all() and (cells == 9).all() and (cen == 9.0).all() and untouched()
    assert L.tloam_closed_map_route_points(H.h, flat, n, None, cp, None, None) == 0 and cost.tobytes() == N.points(scan)[0].tobytes()
    total = 76 * 56 * 56
    one = np.zeros(4, np.uint32)
    op = one.ctypes.data_as(C.POINTER(C.c_uint32))
    assert L.tloam_closed_map_read_route(H.h, total, 1, op) == -1 and L.tloam_closed_map_read_route(H.h, total, 0, op) == 0
    assert L.tloam_closed_map_read_route(H.h, total - 1, 1, op) == 0 and one[0] == N.cost.ravel()[-1]
    assert L.tloam_closed_map_read_route(H.h, 5, 3, op) == 0 and one[:3].tobytes() == N.cost.ravel()[5:8].tobytes()
    assert L.tloam_closed_map_read_route(H.h, 0, 1, None) == -1 and untouched()
    # the columns: the capacity convention
    nx, ny = C.c_size_t(0), C.c_size_t(0)
    col = np.full(76 * 56, 9, np.uint32)
    up = col.ctypes.data_as(C.POINTER(C.c_uint32))
    goal = GOAL.ctypes.data_as(C.POINTER(C.c_double))
    assert L.tloam_closed_map_route_columns(H.h, 0.5, 2.9, 1, goal, 1, None, 0.5, None, None, up, 76 * 56 - 1, C.byref(nx), C.byref(ny), None) == -1
    assert (nx.value, ny.value) == (76, 56) and (col == 9).all()
    assert L.tloam_closed_map_route_columns(H.h, 0.5, 2.9, 1, goal, 1, None, 0.5, None, None, None, 76 * 56, C.byref(nx), C.byref(ny), None) == -1
    assert L.tloam_closed_map_route_columns(H.h, 0.5, 2.9, 1, None, 1, None, 0.5, None, None, up, 76 * 56, C.byref(nx), C.byref(ny), None) == -1
    assert L.tloam_closed_map_route_columns(H.h, 0.5, 2.9, 1, goal, 0, None, 0.5, None, None, up, 76 * 56, C.byref(nx), C.byref(ny), None) == -1
    assert L.tloam_closed_map_route_columns(H.h, 0.5, 2.9, 1, goal, 1, None, 0.5, None, None, up, 76 * 56, C.byref(nx), C.byref(ny), None) == 0
    assert col.tobytes() == N.columns(0.5, 2.9, GOAL, 0.5)[2].tobytes() and untouched()
    # max_bytes: the field and its flags; a path call's centres.  A configure drops the field, so what stays is that there is none
    zero = reg.RouteInfo().as_dict()
    need = 4 * total + 8 * 3 * 7 * 14
    H.closed_map_route_configure(max_bytes=need - 1)
    with invalid(reg):
        H.closed_map_route_build(GOAL, 0.5)
    assert H.closed_map_route_info() == zero
    H.closed_map_route_configure(max_bytes=need)
    assert plain(H.closed_map_route_build(GOAL, 0.5)) == plain(info)
    with invalid(reg):
        H.closed_map_route_paths(scan[:100], need // 2400 + 1)
    assert bits(H.closed_map_route_paths(scan[:100], need // 2400)[3]) == bits(N.paths(scan[:100], need // 2400)[3])
    H.closed_map_route_configure(max_bytes=4 * 76 * 56 + 8 * 3 * 7 - 1)
    with invalid(reg):
        H.closed_map_route_columns(0.5, 2.9, GOAL)
    H.closed_map_route_configure(max_bytes=4 * 76 * 56 + 8 * 3 * 7)
    H.closed_map_route_columns(0.5, 2.9, GOAL)
    H.closed_map_route_configure()
    assert plain(H.closed_map_route_build(GOAL, 0.5)) == plain(info) and H.closed_map_route_field().tobytes() == field
    # nranks > 1: every call is refused
    X = reg.HipRegistration()
    X.comm_init_callback(0, 2, lambda dev, count, stream: 0)
    for call in (X.closed_map_route_configure, X.closed_map_route_info, lambda: X.closed_map_route_build(GOAL),
                 lambda: X.closed_map_route_points(scan), lambda: X.closed_map_route_paths(scan, 3)):
        with invalid(reg):
            call()
    assert X.L.tloam_closed_map_read_route(X.h, 0, 0, None) == -1
    assert X.L.tloam_closed_map_route_columns(X.h, 0.0, 1.0, 1, goal, 1, None, 0.0, None, None, up, 0, C.byref(nx), C.byref(ny), None) == -1
    X.close()


def test_the_route_changes_nothing_else(hip_module):
    reg = hip_module
    poses, clouds, scan, pose, _ = DS.ghost_gate()
    H, T = TL.surfeled(reg, poses, clouds, CS.MASK, DS.VOXEL)
    V = CN.build_map(poses, clouds, CS.MASK, DS.VOXEL)
    cfg = dict(max_range=DS.MAX_RANGE)
    H.closed_map_carve_configure(**cfg)
    H.closed_map_carve()
    H.closed_map_diff_configure(**cfg)
    H.closed_map_diff(scan, pose)
    G, _ = TF.free_built(H, V, poses, clouds, carve_gate=1, **cfg)
    M = H.closed_map_misses()
    K, _ = cleared(H, G, misses=M, unknown_is_obstacle=1)
    prior = LS.offset(pose, 0.1, 0.01)

    def everything(X):
        rows = X.closed_map_read()
        found = X.closed_map_localise(scan, prior)
        through, hits = X.closed_map_diff_counts()
        return (bits(rows[0]) + rows[1].tobytes(), X.closed_map_misses().tobytes(), TS.surfel_bytes(X), X.closed_map_free_words().tobytes(),
                X.closed_map_free_info(), X.closed_map_clearance_field().tobytes(), X.closed_map_clearance_info(),
                through.tobytes() + hits.tobytes(), bits(found[0]), {**found[1], "prepared": 0},
                log_bytes(X.closed_map_localise_log()), {**X.closed_map_diff_info(), "prepared": 0, "launches": 0},
                X.closed_map_save(), X.closed_map_save(clouds=True))

    before = everything(H)
    cen = G.free_cells(misses=M)
    for radius in (0.0, DS.VOXEL):
        N, info = routed(H, K, cen[:2], radius)
        assert info["goals_accepted"] >= 1
        same_queries(H, N, n=400, misses=M)
        H.closed_map_route_columns(0.0, 2.0, cen[:2], radius)
        assert everything(H) == before
    # the stages that do not change what the field was built from leave it: a surfel pass, a diff, a localise
    field, info = H.closed_map_route_field().tobytes(), H.closed_map_route_info()
    H.closed_map_surfels(); H.closed_map_diff(scan, pose)
    assert everything(H) == before and H.closed_map_route_field().tobytes() == field and H.closed_map_route_info() == info
    H.close()
