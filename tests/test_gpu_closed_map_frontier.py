"""-m gpu: the frontiers of the closed map (tl_frontier.hip, tl_api_frontier.hip) against their numpy
restatement (tests/closed_map_frontier_np.py), bit for bit: every byte of the field, the info without its four diagnostics, the
cluster records and centroids, the cells, the point queries, the cost join and the columns.  The scenes and helpers are
tests/test_gpu_closed_map_clearance.py's; exact free cells are painted by tests/frontier_scenes.py.

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
import closed_map_frontier_np as QN  # noqa: E402
import closed_map_route_np as RN  # noqa: E402
import diff_scenes as DS  # noqa: E402
import frontier_scenes as QS  # noqa: E402
import localise_scenes as LS  # noqa: E402
import test_gpu_closed_map_clearance as TK  # noqa: E402
import test_gpu_closed_map_free as TF  # noqa: E402
import test_gpu_closed_map_localise as TL  # noqa: E402
import test_gpu_closed_map_route as TR  # noqa: E402
import test_gpu_closed_map_surfel as TS  # noqa: E402
from test_closed_map_frontier_np import WALL_TABLE  # noqa: E402
from tloam_amd import map_io  # noqa: E402

pytestmark = pytest.mark.gpu

bits, invalid, not_ready, built, log_bytes = TF.bits, TF.invalid, TF.not_ready, TF.built, TF.log_bytes
hand_map, boxed, cleared, wall = TK.hand_map, TK.boxed, TK.cleared, TK.wall
GOAL = TR.GOAL                               # the wall scene's sensor cell
TABLE = ("free_cells", "unknown_cells", "occupied_cells", "frontier_cells", "clusters", "clusters_kept", "cells_kept", "largest",
         "unknown_faces")


def hip_error(reg, what):
    return pytest.raises(reg.TloamHipError, match=what)


def plain(info):
    return {k: v for k, v in info.items() if k not in QN.DIAGNOSTICS}


def same_field(H, N, info=None):
    """the device's field and info (without the diagnostics) are the restatement's"""
    got = H.closed_map_frontier_info()
    if info is not None:
        assert plain(info) == plain(got)
    assert plain(got) == N.info(), (plain(got), N.info())
    assert got["rounds"] >= 1 and got["waits"] >= 2 and got["launches"] >= 5 and got["tile_updates"] >= min(got["frontier_cells"], 1)
    assert got["free_cells"] + got["unknown_cells"] + got["occupied_cells"] == int(np.prod(got["n_cells"]))
    label = H.closed_map_frontier_field()
    assert label.dtype == np.uint32 and label.shape == N.label.shape
    assert label.tobytes() == N.label.tobytes(), np.argwhere(label != N.label)[:5]
    return got


def fronted(H, G, misses=None, **cfg):
    """the field configured and built on the device and in the restatement -> (N, info)"""
    H.closed_map_frontier_configure(**cfg)
    N = QN.FrontierNP(G, **cfg)
    assert N.build(misses) is True
    info = H.closed_map_frontier_build()
    print(f"{cfg}: {info}")
    return N, same_field(H, N, info)


def same_lists(H, N):
    """the kept clusters, their centroids and the cells (of all kept clusters, of single ones, of roots that are not kept)"""
    rec, cen = H.closed_map_frontier_clusters()
    want, wcen = N.clusters()
    assert rec.dtype == QN.CLUSTER and rec.tobytes() == want.tobytes(), (rec, want)
    assert bits(cen) == bits(wcen)
    centres, roots = H.closed_map_frontier_cells()
    wc, wr = N.cells()
    assert roots.dtype == np.uint32 and bits(centres) == bits(wc) and roots.tobytes() == wr.tobytes()
    assert len(roots) == N.info()["cells_kept"]
    for root in list(want["root"][:2]) + list(want["root"][-1:]):
        centres, roots = H.closed_map_frontier_cells(int(root))
        wc, wr = N.cells(int(root))
        assert bits(centres) == bits(wc) and roots.tobytes() == wr.tobytes() and (roots == root).all() and len(roots) > 0
    dropped = [int(r) for r in N.roots if r not in set(want["root"].tolist())][:1]
    for root in dropped + [int(N.label.size) + 5, QN.OUTSIDE, QN.UNKNOWN]:       # a component not kept; no root at all
        centres, roots = H.closed_map_frontier_cells(root)
        assert centres.shape == (0, 3) and len(roots) == 0
    return rec


def same_points(H, N, pts, pose=None):
    label, cluster, counts = H.closed_map_frontier_points(pts, pose)
    wl, wc, wn = N.points(pts, pose)
    assert label.dtype == np.uint32 and cluster.dtype == np.int32
    assert label.tobytes() == wl.tobytes() and cluster.tobytes() == wc.tobytes() and counts.tobytes() == wn.tobytes()
    return label, cluster, counts


def same_queries(H, N, seed=1, n=600, misses=None):
    """points in the map frame and under a pose: all over the box and beyond it, the kept cells' own centres among them"""
    G = N.G
    rng = np.random.default_rng(seed)
    kept = N.cells()[0]
    pts = np.concatenate([kept[:: max(len(kept) // 200, 1)], TF.probes(G, rng, misses, n=n)])
    label, cluster, counts = same_points(H, N, pts)
    assert counts.sum() == len(pts) and counts[4] >= 5
    lo, hi = TK.box_metric(G)
    pose = LS.offset(np.eye(4), 0.7, 0.4)
    pose[:3, 3] += 0.5 * (lo + hi)
    local = np.ascontiguousarray((pts[:-5] - pose[:3, 3]) @ pose[:3, :3])
    same_points(H, N, local, pose)
    return label, cluster, counts


def same_costs(H, N, route):
    cost, approach = H.closed_map_frontier_costs()
    wc, wa = N.costs(route)
    assert cost.dtype == np.uint32 and cost.tobytes() == wc.tobytes() and bits(approach) == bits(wa)
    return cost, approach


def same_columns(H, N, z_lo, z_hi, min_free=1, misses=None):
    label, rec, cen, info = H.closed_map_frontier_columns(z_lo, z_hi, min_free)
    wl, wrec, winfo = N.columns(z_lo, z_hi, min_free, misses)
    assert label.dtype == np.uint32 and label.shape == wl.shape and label.tobytes() == wl.tobytes()
    assert rec.tobytes() == wrec.tobytes() and plain(info) == winfo, (plain(info), winfo)
    assert bits(cen) == bits(QN.centroids(wrec, winfo["lo_cells"], N.G.o, N.G.v))
    assert (rec["sum"][:, 2] == 0).all() and (rec["lo"][:, 2] == winfo["lo_cells"][2]).all() and (rec["hi"][:, 2] == winfo["lo_cells"][2]).all()
    return label, rec, info


def scene(reg, voxels, lo, hi, runs):
    """-> (H, G): voxels `voxels` in the box [lo, hi] (cells), exactly the runs' cells seen through"""
    H, V = hand_map(reg, np.asarray(voxels, np.int64).reshape(-1, 3))
    G = boxed(H, V, lo, hi, **QS.PAINT)
    QS.paint(G, runs, H, TF.scan_and_compare)
    return H, G


# ---- the wall --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", [0, 1])
def test_the_wall(wall, hip_module, tmp_path, gate):
    H, V, G, poses, clouds, scan, truth = wall
    M = None
    if gate:
        H.closed_map_carve_configure(max_range=12.0)
        H.closed_map_carve()
        M = H.closed_map_misses()
        assert M.tobytes() == CN.carve(V, poses, clouds, CS.MASK, max_range=12.0)[0].tobytes()
        G, _ = TF.free_built(H, V, poses, clouds, carve_gate=1, **TF.WALL)
    N, info = fronted(H, G, M)
    assert tuple(info[k] for k in TABLE) == WALL_TABLE[gate]
    assert info["n_cells"] == (76, 56, 56) and info["bytes"] == 4 * 76 * 56 * 56 + 8 * 3 * 7 * 14
    same_lists(H, N)
    same_queries(H, N, misses=M)
    # two builds give the same bytes
    before = H.closed_map_frontier_field().tobytes()
    assert plain(H.closed_map_frontier_build()) == plain(info) and H.closed_map_frontier_field().tobytes() == before
    # the join with the route: a clearance and a route build (and their configures) leave the frontier field alone
    for wrap, radii in ((0, (0.0,)), (1, (0.0, 1.0))):
        K, _ = cleared(H, G, misses=M, max_distance=4.0, unknown_is_obstacle=wrap)
        for radius in radii:
            R, rinfo = TR.routed(H, K, GOAL, radius)
            for reach in (0, 2, 4):
                # (reach is read by the join alone; a configure drops the field, so it is built again: the same bytes)
                H.closed_map_frontier_configure(reach=reach)
                N.cfg["reach"] = reach
                assert plain(H.closed_map_frontier_build()) == plain(info) and H.closed_map_frontier_field().tobytes() == before
                cost, approach = same_costs(H, N, R.cost)
                if wrap == 1 and radius == 1.0 and reach == 0:
                    assert (cost == RN.UNREACHED).all() and np.isnan(approach).all()
                if wrap == 0:
                    assert (cost < RN.OUTSIDE).all() and np.isfinite(approach).all()
            H.closed_map_route_configure()                                            # drops the route, not the frontier
            assert H.closed_map_frontier_field().tobytes() == before
            with not_ready(hip_module):
                H.closed_map_frontier_costs()
    if gate == 0:
        # the PCD exports, read back
        K, _ = cleared(H, G, max_distance=4.0, unknown_is_obstacle=0)
        R, _ = TR.routed(H, K, GOAL, 0.0)
        N, _ = fronted(H, G)
        rec, cen = N.clusters()
        for ascii in (False, True):
            path = str(tmp_path / f"frontier{int(ascii)}.pcd")
            assert map_io.write_frontier_pcd(path, H, ascii=ascii) == info["cells_kept"]
            c2, index = map_io.read_frontier_pcd(path)
            wc, wr = N.cells()
            assert bits(c2) == bits(wc) and index.tolist() == np.searchsorted(rec["root"], wr).tolist()
            path = str(tmp_path / f"clusters{int(ascii)}.pcd")
            assert map_io.write_frontier_clusters_pcd(path, H, ascii=ascii) == len(rec)
            c2, cells, faces, cost = map_io.read_frontier_clusters_pcd(path)
            assert bits(c2) == bits(cen) and cells.tolist() == rec["cells"].tolist() and faces.tolist() == rec["unknown_faces"].tolist()
            assert cost.tolist() == N.costs(R.cost)[0].astype(np.float64).tolist()
    if gate:
        TF.free_built(H, V, poses, clouds, **TF.WALL)                                 # the fixture's grid again


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_query_batches(wall, n):
    H, V, G, _, _, scan, truth = wall
    N, info = fronted(H, G)
    cen = N.cells()[0]
    pts = np.concatenate([cen[:: max(len(cen) // n, 1)], scan])[:n]
    label, cluster, counts = same_points(H, N, pts)
    assert len(label) == n and counts.sum() == n
    same_points(H, N, np.ascontiguousarray(pts - truth[:3, 3]) @ truth[:3, :3], truth)
    assert (same_points(H, N, cen[:1])[1] == 0).all()                                 # a kept cluster's own cell: its index


def test_the_walls_columns(wall):
    H, V, G, _, _, scan, truth = wall
    N, info = fronted(H, G)
    field = H.closed_map_frontier_field().tobytes()
    seen = 0
    for min_cells in (1, 8):
        N, _ = fronted(H, G, min_cells=min_cells)
        for band in ((0.5, 2.9, 1), (-1.0, 0.7, 2), (-1e6, 1e6, 3), (1e4, 1e4 + 10.0, 1)):
            label, rec, cinfo = same_columns(H, N, *band)
            assert cinfo["n_cells"] == (76, 56, 1)
            seen += len(rec)
        assert plain(H.closed_map_frontier_info()) == plain(info) | {"clusters_kept": N.info()["clusters_kept"], "cells_kept": N.info()["cells_kept"]}
        assert H.closed_map_frontier_field().tobytes() == field                       # a built field is left alone
    assert seen > 0


# ---- painted cells ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_painted_runs_cross_every_seam(hip_module, axis):
    """a run of 600 cells along each axis (19, 75 and 150 tiles in sequence): one cluster, so the label crosses every seam; then
    max_rounds = 1 and the two extremes of rounds_per_wait"""
    reg = hip_module
    hi = np.full(3, 7, np.int64)
    hi[axis] = 603
    e = np.eye(3, dtype=np.int64)[axis]
    a = np.array([1, 2, 5]) * (1 - e) + 2 * e
    H, G = scene(reg, np.zeros((0, 3), np.int64), (0, 0, 0), hi, [(a, a + 599 * e)])
    N, info = fronted(H, G)
    assert (info["clusters"], info["clusters_kept"], info["cells_kept"], info["largest"], info["unknown_faces"]) == (1, 1, 600, 600, 2402)
    assert info["rounds"] >= 2                                    # (of the order of 19, 75 and 150: a diagnostic, printed)
    first = H.closed_map_frontier_field().tobytes()
    rec = same_lists(H, N)
    assert rec["lo"][0].tolist() == a.tolist() and rec["hi"][0].tolist() == (a + 599 * e).tolist()
    same_queries(H, N, n=300)
    H.closed_map_frontier_configure(max_rounds=1)
    with hip_error(reg, "max_rounds = 1"):
        H.closed_map_frontier_build()
    assert H.closed_map_frontier_info() == reg.FrontierInfo().as_dict()
    with not_ready(reg):
        H.closed_map_frontier_field()
    for per_wait in (1, 1024):
        H.closed_map_frontier_configure(rounds_per_wait=per_wait)
        got = H.closed_map_frontier_build()
        assert plain(got) == plain(info) and H.closed_map_frontier_field().tobytes() == first
        assert got["waits"] >= got["rounds"] + 2 if per_wait == 1 else got["waits"] <= 4
    H.close()


def test_a_serpentine_in_one_tile(hip_module):
    """263 cells in a single tile whose end-to-end path exceeds the 64 passes a tile gets in LDS per round: the tile meets the cap
    and hands itself to the next round"""
    H, G = scene(hip_module, np.zeros((0, 3), np.int64), (0, 0, 0), (31, 7, 3), QS.serpentine_runs())
    N, info = fronted(H, G)
    assert (info["n_cells"], info["clusters"], info["frontier_cells"], info["free_cells"]) == ((32, 8, 4), 1, 263, 263)
    assert info["rounds"] > 1
    same_lists(H, N)
    same_queries(H, N, n=200)
    H.close()


def test_a_u_turn_through_the_neighbouring_tile(hip_module):
    """two tiles along x; the chain leaves the first tile along y = 0, turns in the second and comes back along y = 4: the first
    tile's second row gets its label only through the second tile"""
    runs = [((20, 0, 0), (40, 0, 0)), ((40, 0, 0), (40, 4, 0)), ((40, 4, 0), (20, 4, 0))]
    H, G = scene(hip_module, np.zeros((0, 3), np.int64), (0, 0, 0), (63, 7, 3), runs)
    N, info = fronted(H, G)
    assert (info["clusters"], info["frontier_cells"]) == (1, 45) and info["tile_updates"] >= 3 and info["rounds"] >= 2
    assert int(N.label[0, 4, 20]) == 20
    same_lists(H, N)
    same_queries(H, N, n=200)
    H.close()


@pytest.mark.parametrize("runs", [[((28, 7, 3), (31, 7, 3)), ((32, 8, 4), (35, 8, 4))],      # across the corner (32, 8, 4)
                                  [((28, 7, 1), (31, 7, 1)), ((32, 8, 1), (35, 8, 1))],      # across the edge along z
                                  [((28, 5, 3), (31, 5, 3)), ((32, 5, 4), (35, 5, 4))],      # across the edge along y
                                  [((30, 4, 3), (30, 7, 3)), ((30, 8, 4), (30, 11, 4))]])    # across the edge along x
def test_two_runs_meeting_across_a_tile_boundary(hip_module, runs):
    """one cluster, carried by the vertex- or edge-neighbour tile's flag alone"""
    H, G = scene(hip_module, np.zeros((0, 3), np.int64), (0, 0, 0), (39, 15, 7), runs)
    N, info = fronted(H, G)
    assert (info["clusters"], info["clusters_kept"], info["frontier_cells"], info["largest"]) == (1, 1, 8, 8)
    root = (runs[0][0][2] * 16 + runs[0][0][1]) * 40 + runs[0][0][0]
    assert same_lists(H, N)["root"].tolist() == [root]
    same_queries(H, N, n=200)
    H.close()


def test_two_blocks_and_the_gap_between_them(hip_module):
    """two solid blocks one unknown cell apart are two clusters; with the gap painted they are one"""
    runs = QS.block_runs((2, 2, 2), (4, 4, 4)) + QS.block_runs((6, 2, 2), (8, 4, 4))
    H, G = scene(hip_module, np.zeros((0, 3), np.int64), (0, 0, 0), (11, 7, 7), runs)
    N, info = fronted(H, G)
    assert (info["clusters"], info["clusters_kept"], info["frontier_cells"], info["free_cells"]) == (2, 2, 52, 54)
    same_lists(H, N)
    QS.paint(G, QS.block_runs((5, 2, 2), (5, 4, 4)), H, TF.scan_and_compare)
    with not_ready(hip_module):
        H.closed_map_frontier_field()                                                 # the add dropped the field
    N, info = fronted(H, G)
    assert (info["clusters"], info["frontier_cells"], info["free_cells"]) == (1, 58, 63)
    same_lists(H, N)
    same_queries(H, N, n=200)
    H.close()


def test_a_run_cut_by_a_voxel_and_joined_by_the_gate(hip_module):
    """a voxel in the middle of a run splits it in two; four rays of the keyframe pass through that voxel, so under the ghost
    gate it is carved away and the run joins again"""
    reg = hip_module
    pose = np.eye(4)
    pose[:3, 3] = [0.5, 0.5, 0.5]
    world = np.array([[8.5, 0.5, 0.5], [12.5, 0.5, 0.5], [13.5, 0.5, 0.5], [14.5, 0.5, 0.5], [15.5, 0.5, 0.5]])
    poses, clouds = [pose], [CS.slot0(world - pose[:3, 3])]
    H, V = built(reg, poses, clouds, CS.MASK, 1.0)
    H.closed_map_carve_configure()
    H.closed_map_carve()
    M = H.closed_map_misses()
    assert M.tolist() == CN.carve(V, poses, clouds, CS.MASK)[0].tolist() and M[0] >= 3
    want = {0: [6, 3], 1: [10]}
    for gate in (0, 1):
        G = TF.fresh(H, V, lo=(0, 0, 0), hi=(23, 3, 3), carve_gate=gate, **QS.PAINT)
        QS.paint(G, [((2, 0, 0), (11, 0, 0))], H, TF.scan_and_compare)
        N, info = fronted(H, G, M if gate else None, min_cells=1)
        assert same_lists(H, N)["cells"].tolist() == want[gate]
        same_queries(H, N, n=200, misses=M if gate else None)
    # the gate on a map that is not carved: no build, no columns
    H.closed_map_carve_configure(max_range=11.0)
    for call in (H.closed_map_frontier_build, H.closed_map_frontier_field, lambda: H.closed_map_frontier_columns(0.0, 1.0)):
        with not_ready(reg):
            call()
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
        voxels = blo + np.argwhere(rng.random(n) < 0.1)
        H, V = hand_map(hip_module, voxels)
        centre = 0.5 * (blo + bhi + 1.0) + 0.01
        G = boxed(H, V, lo, hi, rays=TK.star(centre, 0.45 * float(n.max()), n=150, seed=int(n.sum())), max_range=200.0, end_margin=0.0)
        for min_cells in (1, 3):
            N, info = fronted(H, G, min_cells=min_cells)
            assert info["lo_cells"] == tuple(blo) and info["n_cells"] == tuple(n) and info["frontier_cells"] > 0
            same_lists(H, N)
            same_queries(H, N, n=300)
            # the column form over the same box: a band of one layer and of all of them
            for z_lo, z_hi in ((float(blo[2]) + 0.5, float(blo[2]) + 0.5), (-1e6, 1e6)):
                same_columns(H, N, z_lo, z_hi)
        H.close()


def test_no_frontier_at_all(hip_module):
    """nothing seen through: every cell UNKNOWN or OCCUPIED, TLOAM_OK and empty lists"""
    H, V = hand_map(hip_module, [(1, 1, 1), (5, 2, 3)])
    G = boxed(H, V, (0, 0, 0), (39, 11, 7))
    N, info = fronted(H, G)
    assert tuple(info[k] for k in TABLE) == (0, 40 * 12 * 8 - 2, 2, 0, 0, 0, 0, 0, 0) and info["rounds"] == 1
    rec, cen = H.closed_map_frontier_clusters()
    assert len(rec) == 0 and cen.shape == (0, 3)
    assert H.closed_map_frontier_cells()[0].shape == (0, 3) and H.closed_map_frontier_cells(0)[0].shape == (0, 3)
    same_queries(H, N, n=100)
    label, rec, cinfo = same_columns(H, N, -1e6, 1e6)
    assert len(rec) == 0 and cinfo["frontier_cells"] == 0
    K, _ = cleared(H, G, unknown_is_obstacle=0)
    TR.routed(H, K, G.o + (np.array([[0, 0, 0]]) + 0.5) * G.v)
    cost, approach = H.closed_map_frontier_costs()
    assert len(cost) == 0 and approach.shape == (0, 3)
    H.close()


def test_more_singletons_than_a_block_scans(hip_module):
    """1050 free cells, each between two voxels of a run along x: 1050 clusters of one cell, more than four blocks of the kept
    list's compaction; min_cells 1 keeps them all, 2 keeps none"""
    voxels = [(2 * k + 1, 1, 1) for k in range(1050)]
    H, G = scene(hip_module, voxels, (0, 0, 0), (2103, 3, 3), [((0, 1, 1), (2099, 1, 1))])
    N, info = fronted(H, G, min_cells=1)
    assert (info["clusters"], info["clusters_kept"], info["cells_kept"], info["largest"], info["occupied_cells"]) == (1050, 1050, 1050, 1, 1050)
    rec = same_lists(H, N)
    assert rec["root"].tolist() == [(1 * 4 + 1) * 2104 + 2 * k for k in range(1050)] and (rec["unknown_faces"] == 4).all()
    label, cluster, _ = same_queries(H, N, n=300)
    assert cluster.max() > 1024 and same_points(H, N, N.cells()[0][-1:])[1].tolist() == [1049]
    N, info = fronted(H, G, min_cells=2)
    assert (info["clusters"], info["clusters_kept"], info["cells_kept"]) == (1050, 0, 0)
    assert len(same_lists(H, N)) == 0 and (same_queries(H, N, n=300)[1] == -1).all()
    H.close()


# ---- lifetime ----------------------------------------------------------------------------------------------------------------------
def test_what_drops_the_field_and_what_does_not(hip_module):
    reg = hip_module
    poses, clouds, scan, truth = LS.wall()
    v = CS.GHOST["voxel"]
    H, V = built(reg, poses, clouds, CS.MASK, v)
    zero = reg.FrontierInfo().as_dict()
    assert H.closed_map_frontier_info() == zero
    with not_ready(reg):
        H.closed_map_frontier_build()                                                 # no grid
    with not_ready(reg):
        H.closed_map_frontier_columns(0.5, 2.9)
    H.closed_map_free_configure(**TF.WALL)
    H.closed_map_free_build()
    H.closed_map_frontier_columns(0.5, 2.9)                                           # (computed from the grid: no field needed)

    def gone():
        assert H.closed_map_frontier_info() == zero
        for call in (H.closed_map_frontier_field, H.closed_map_frontier_clusters, H.closed_map_frontier_cells,
                     lambda: H.closed_map_frontier_points(scan), H.closed_map_frontier_costs):
            with not_ready(reg):
                call()
        return True

    assert gone()
    info = H.closed_map_frontier_build()                                              # no clearance field is needed
    field = H.closed_map_frontier_field().tobytes()
    clusters = H.closed_map_frontier_clusters()[0].tobytes()

    def there():
        return (plain(H.closed_map_frontier_info()) == plain(info) and H.closed_map_frontier_field().tobytes() == field
                and H.closed_map_frontier_clusters()[0].tobytes() == clusters)

    cfg = dict(max_distance=4.0, unknown_is_obstacle=1)
    keeps = [lambda: H.closed_map_frontier_columns(0.5, 2.9), lambda: H.closed_map_clearance_configure(**cfg), H.closed_map_clearance_build,
             H.closed_map_route_configure, lambda: H.closed_map_route_build(GOAL, 0.5), lambda: H.closed_map_route_columns(0.5, 2.9, GOAL),
             lambda: H.closed_map_clearance_columns(0.5, 2.9), H.closed_map_frontier_costs,
             lambda: H.closed_map_occupancy(scan), lambda: H.closed_map_free_columns(0.5, 2.9)]
    for k, keep in enumerate(keeps):
        keep()
        assert there(), k
    drops = [H.closed_map_frontier_configure, H.closed_map_free_add_keyframes, lambda: H.closed_map_free_add_scan(scan[:50], truth),
             H.closed_map_carve, lambda: H.closed_map_carve_configure(max_range=11.0), H.closed_map_free_reset,
             lambda: H.closed_map_free_configure(**TF.WALL)]
    for k, drop in enumerate(drops):
        drop()
        assert gone(), k
        H.closed_map_free_build()                                                     # back to the keyframes' grid
        assert plain(H.closed_map_frontier_build()) == plain(info) and there(), k
    # a fresh context gives the same bytes; the configuration persists across an odometry reset; nothing in a snapshot
    F, _ = built(reg, poses, clouds, CS.MASK, v)
    F.closed_map_free_configure(**TF.WALL)
    F.closed_map_free_build()
    F.closed_map_frontier_configure(rounds_per_wait=3, min_cells=8)
    got = F.closed_map_frontier_build()
    assert plain(got) == plain(info) and F.closed_map_frontier_field().tobytes() == field
    assert F.closed_map_frontier_clusters()[0].tobytes() == clusters
    blob = F.closed_map_save()
    F.closed_map_load(blob)
    assert F.closed_map_frontier_info() == zero
    F.odometry_reset(None, TS.TC.odom_cfg(reg))
    assert F.closed_map_frontier_info() == zero
    for k in range(len(poses)):
        assert F.place_add_scan(TS.DUMMY, np.eye(4), k) == k
        F.place_set_keyframe_clouds(k, *clouds[k])
    F.closed_map_build(2, poses)
    F.closed_map_free_build()
    again = F.closed_map_frontier_build()
    assert plain(again) == plain(info) and F.closed_map_frontier_field().tobytes() == field
    assert again["waits"] >= -(-again["rounds"] // 3) + 2 and again["waits"] <= -(-again["rounds"] // 3) + 3   # rounds_per_wait 3: still there
    H.close(); F.close()


def test_an_extend_drops_the_field(hip_module):
    """a successful extend changes the map's voxels: the frontier field goes with the clearance field, the grid stays"""
    reg = hip_module
    poses, clouds, _, _ = LS.wall()
    v = CS.GHOST["voxel"]
    A = TF.context(reg, poses, clouds, keep=range(5), voxel=v, cloud_mask=CS.MASK)
    A.closed_map_build(2, poses[:5])
    A.closed_map_free_configure(**TF.WALL)
    A.closed_map_free_build()
    first = A.closed_map_frontier_build()
    assert first["frontier_cells"] > 0
    assert A.place_add_scan(TS.DUMMY, poses[5], 5) == 5
    A.place_set_keyframe_clouds(5, *clouds[5])
    A.closed_map_extend(2, poses[5:6])
    assert A.closed_map_frontier_info() == reg.FrontierInfo().as_dict() and A.closed_map_free_info()["free_cells"] > 0
    with not_ready(reg):
        A.closed_map_frontier_field()
    again = A.closed_map_frontier_build()
    assert again["n_cells"] == first["n_cells"] and again["occupied_cells"] >= first["occupied_cells"]
    A.close()


def test_refusals_leave_the_field(wall, hip_module):
    reg = hip_module
    H, V, G, poses, clouds, scan, truth = wall
    N, info = fronted(H, G)
    info = H.closed_map_frontier_info()
    field = H.closed_map_frontier_field().tobytes()

    def untouched():
        return H.closed_map_frontier_field().tobytes() == field and H.closed_map_frontier_info() == info

    for bad in (dict(max_bytes=3), dict(max_bytes=-1), dict(min_cells=0), dict(min_cells=-2), dict(reach=-1), dict(reach=5),
                dict(max_rounds=0), dict(max_rounds=-5), dict(rounds_per_wait=0), dict(rounds_per_wait=1025), dict(rounds_per_wait=-1)):
        with invalid(reg):
            H.closed_map_frontier_configure(**bad)
    with pytest.raises(KeyError):
        H.closed_map_frontier_configure(radius=1.0)
    assert untouched()
    for bad_pose in (2.0 * np.eye(4), np.full((4, 4), np.nan), np.diag([1.0, 1.0, -1.0, 1.0])):
        with invalid(reg):
            H.closed_map_frontier_points(scan, bad_pose)
    for bad_band in ((np.nan, 1.0, 1), (0.0, 1.0, 0), (2.0, 1.0, 1)):
        with invalid(reg):
            H.closed_map_frontier_columns(*bad_band)
    assert untouched()
    # the raw entry points: NULL arguments, n == 0, ranges, capacities 0, one short and exact
    L = H.L
    n = len(scan)
    flat = np.ascontiguousarray(scan).ctypes.data_as(C.POINTER(C.c_double))
    label, cluster = np.full(n, 9, np.uint32), np.full(n, 9, np.int32)
    lp, ip = label.ctypes.data_as(C.POINTER(C.c_uint32)), cluster.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.tloam_closed_map_frontier_points(H.h, None, n, None, lp, ip, None) == -1
    assert L.tloam_closed_map_frontier_points(H.h, flat, 0, None, lp, ip, None) == -1
    assert L.tloam_closed_map_frontier_points(H.h, flat, n, None, None, ip, None) == -1
    assert (label == 9).all() and (cluster == 9).all() and untouched()
    assert L.tloam_closed_map_frontier_points(H.h, flat, n, None, lp, None, None) == 0 and label.tobytes() == N.points(scan)[0].tobytes()
    total = 76 * 56 * 56
    one = np.zeros(4, np.uint32)
    op = one.ctypes.data_as(C.POINTER(C.c_uint32))
    assert L.tloam_closed_map_read_frontier(H.h, total, 1, op) == -1 and L.tloam_closed_map_read_frontier(H.h, total, 0, op) == 0
    assert L.tloam_closed_map_read_frontier(H.h, total - 1, 1, op) == 0 and one[0] == N.label.ravel()[-1]
    assert L.tloam_closed_map_read_frontier(H.h, 5, 3, op) == 0 and one[:3].tobytes() == N.label.ravel()[5:8].tobytes()
    assert L.tloam_closed_map_read_frontier(H.h, 0, 1, None) == -1 and untouched()
    k, m = info["clusters_kept"], info["cells_kept"]
    assert k >= 1 and m >= 8
    got = C.c_size_t(77)
    rec = np.zeros(k + 1, QN.CLUSTER)
    rec["reserved"] = 9
    assert L.tloam_closed_map_frontier_clusters(H.h, k, rec.ctypes.data, None) == -1
    for cap in (0, k - 1):
        assert L.tloam_closed_map_frontier_clusters(H.h, cap, rec.ctypes.data, C.byref(got)) == -1 and got.value == k and (rec["reserved"] == 9).all()
    assert L.tloam_closed_map_frontier_clusters(H.h, k, None, C.byref(got)) == 0 and got.value == k
    assert L.tloam_closed_map_frontier_clusters(H.h, k, rec.ctypes.data, C.byref(got)) == 0 and rec[:k].tobytes() == N.kept.tobytes() and rec["reserved"][k] == 9
    cen, roots = np.full((m + 1, 3), 9.0), np.full(m + 1, 9, np.uint32)
    cp, rp = cen.ctypes.data_as(C.POINTER(C.c_double)), roots.ctypes.data_as(C.POINTER(C.c_uint32))
    ALL = reg.FRONTIER_ALL
    assert L.tloam_closed_map_read_frontier_cells(H.h, ALL, m, cp, rp, None) == -1
    for cap in (0, m - 1):
        assert L.tloam_closed_map_read_frontier_cells(H.h, ALL, cap, cp, rp, C.byref(got)) == -1 and got.value == m
    assert (cen == 9.0).all() and (roots == 9).all()
    assert L.tloam_closed_map_read_frontier_cells(H.h, ALL, m, None, None, C.byref(got)) == 0 and got.value == m
    assert L.tloam_closed_map_read_frontier_cells(H.h, ALL, m, cp, None, C.byref(got)) == 0 and bits(cen[:m]) == bits(N.cells()[0]) and (cen[m] == 9.0).all()
    assert L.tloam_closed_map_read_frontier_cells(H.h, ALL, m, None, rp, C.byref(got)) == 0 and roots[:m].tobytes() == N.cells()[1].tobytes() and roots[m] == 9
    assert L.tloam_closed_map_read_frontier_cells(H.h, 3, 0, cp, rp, C.byref(got)) == 0 and got.value == 0        # no kept cluster's root
    K, _ = cleared(H, G, max_distance=4.0, unknown_is_obstacle=0)
    R, _ = TR.routed(H, K, GOAL)
    cost, app = np.full(k + 1, 9, np.uint32), np.full((k + 1, 3), 9.0)
    kp, ap = cost.ctypes.data_as(C.POINTER(C.c_uint32)), app.ctypes.data_as(C.POINTER(C.c_double))
    assert L.tloam_closed_map_frontier_costs(H.h, k, kp, ap, None) == -1
    for cap in (0, k - 1):
        assert L.tloam_closed_map_frontier_costs(H.h, cap, kp, ap, C.byref(got)) == -1 and got.value == k and (cost == 9).all() and (app == 9.0).all()
    assert L.tloam_closed_map_frontier_costs(H.h, k, kp, None, C.byref(got)) == 0 and cost[:k].tobytes() == N.costs(R.cost)[0].tobytes() and cost[k] == 9
    assert L.tloam_closed_map_frontier_costs(H.h, k, None, ap, C.byref(got)) == 0 and bits(app[:k]) == bits(N.costs(R.cost)[1]) and untouched()
    # the columns: the clusters' capacity convention
    wl, wrec, winfo = N.columns(0.5, 2.9)
    kc = len(wrec)
    assert kc >= 1
    col = np.full(76 * 56, 9, np.uint32)
    up = col.ctypes.data_as(C.POINTER(C.c_uint32))
    crec = np.zeros(kc + 1, QN.CLUSTER)
    assert L.tloam_closed_map_frontier_columns(H.h, 0.5, 2.9, 1, up, kc, crec.ctypes.data, None, None) == -1 and (col == 9).all()
    assert L.tloam_closed_map_frontier_columns(H.h, 0.5, 2.9, 1, None, kc - 1, crec.ctypes.data, C.byref(got), None) == -1 and got.value == kc
    assert L.tloam_closed_map_frontier_columns(H.h, 0.5, 2.9, 1, up, kc, crec.ctypes.data, C.byref(got), None) == 0
    assert col.tobytes() == wl.tobytes() and crec[:kc].tobytes() == wrec.tobytes() and untouched()
    # max_bytes: the field and its flags; the cluster table once the roots are counted.  A configure drops the field
    zero = reg.FrontierInfo().as_dict()
    need = 4 * total + 8 * 3 * 7 * 14
    H.closed_map_frontier_configure(max_bytes=need - 1)
    with invalid(reg):
        H.closed_map_frontier_build()
    assert H.closed_map_frontier_info() == zero
    H.closed_map_frontier_configure(max_bytes=need + 136 * info["clusters"] - 1)
    with hip_error(reg, "clusters does not fit under max_bytes"):
        H.closed_map_frontier_build()
    assert H.closed_map_frontier_info() == zero
    H.closed_map_frontier_configure(max_bytes=need + 136 * info["clusters"])
    assert plain(H.closed_map_frontier_build()) == plain(info)
    # the defaults again: the same bytes
    H.closed_map_frontier_configure()
    assert plain(H.closed_map_frontier_build()) == plain(info) and H.closed_map_frontier_field().tobytes() == field
    # nranks > 1: every call is refused
    X = reg.HipRegistration()
    X.comm_init_callback(0, 2, lambda dev, count, stream: 0)
    for call in (X.closed_map_frontier_configure, X.closed_map_frontier_info, X.closed_map_frontier_build,
                 lambda: X.closed_map_frontier_points(scan)):
        with invalid(reg):
            call()
    assert X.L.tloam_closed_map_read_frontier(X.h, 0, 0, None) == -1
    assert X.L.tloam_closed_map_frontier_clusters(X.h, 0, None, C.byref(got)) == -1
    assert X.L.tloam_closed_map_read_frontier_cells(X.h, ALL, 0, None, None, C.byref(got)) == -1
    assert X.L.tloam_closed_map_frontier_costs(X.h, 0, None, None, C.byref(got)) == -1
    assert X.L.tloam_closed_map_frontier_columns(X.h, 0.0, 1.0, 1, None, 0, None, C.byref(got), None) == -1
    X.close()


def test_the_frontier_changes_nothing_else(hip_module):
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
    cen = G.free_cells(misses=M)
    R, _ = TR.routed(H, K, cen[:2], 0.0)
    prior = LS.offset(pose, 0.1, 0.01)

    def everything(X):
        rows = X.closed_map_read()
        found = X.closed_map_localise(scan, prior)
        through, hits = X.closed_map_diff_counts()
        return (bits(rows[0]) + rows[1].tobytes(), X.closed_map_misses().tobytes(), TS.surfel_bytes(X), X.closed_map_free_words().tobytes(),
                X.closed_map_free_info(), X.closed_map_clearance_field().tobytes(), X.closed_map_clearance_info(),
                X.closed_map_route_field().tobytes(), X.closed_map_route_info(),
                through.tobytes() + hits.tobytes(), bits(found[0]), {**found[1], "prepared": 0},
                log_bytes(X.closed_map_localise_log()), {**X.closed_map_diff_info(), "prepared": 0, "launches": 0},
                X.closed_map_save(), X.closed_map_save(clouds=True))

    before = everything(H)
    for min_cells in (1, 8):
        N, info = fronted(H, G, M, min_cells=min_cells)
        assert info["frontier_cells"] > 0
        same_lists(H, N)
        same_queries(H, N, n=400, misses=M)
        same_costs(H, N, R.cost)
        same_columns(H, N, 0.0, 2.0, misses=M)
        assert everything(H) == before
    # the stages that do not change what the field was built from leave it: a surfel pass, a diff, a localise
    field, info = H.closed_map_frontier_field().tobytes(), H.closed_map_frontier_info()
    H.closed_map_surfels(); H.closed_map_diff(scan, pose)
    assert everything(H) == before and H.closed_map_frontier_field().tobytes() == field and H.closed_map_frontier_info() == info
    H.close()
