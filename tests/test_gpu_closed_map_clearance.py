"""-m gpu: the clearance of the closed map (tl_clear.hip, tl_api_clear.hip) against its numpy restatement
(tests/closed_map_clearance_np.py), bit for bit: every byte of the field, every state, d2, distance, status, min_d2, t_block and
every counter.  The scenes and the context helpers are tests/test_gpu_closed_map_free.py's; the hand-made maps have one keyframe
whose cloud puts a point at the centre of every cell that is to be a voxel."""
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
import closed_map_free_np as FN  # noqa: E402
import diff_scenes as DS  # noqa: E402
import localise_scenes as LS  # noqa: E402
import test_gpu_closed_map_free as TF  # noqa: E402
import test_gpu_closed_map_localise as TL  # noqa: E402
import test_gpu_closed_map_surfel as TS  # noqa: E402
from tloam_amd import map_io  # noqa: E402

pytestmark = pytest.mark.gpu

bits, invalid, not_ready, built, context, log_bytes = TF.bits, TF.invalid, TF.not_ready, TF.built, TF.context, TF.log_bytes
WALL, Rz90 = TF.WALL, TF.Rz90
LAUNCHES = 6          # seed | voxels | x | y | z | count: the same for every input
B, O = KN.BEYOND, KN.OUTSIDE


def same_field(H, K, info=None):
    """the device's field and info are the restatement's"""
    got = H.closed_map_clearance_info()
    if info is not None:
        assert info == got
    assert got["launches"] == LAUNCHES
    assert {k: v for k, v in got.items() if k != "launches"} == K.info()
    d2 = H.closed_map_clearance_field()
    assert d2.dtype == np.uint16 and d2.shape == K.d2.shape and d2.tobytes() == K.d2.tobytes()
    return got


def cleared(H, G, misses=None, **cfg):
    """the field configured and built on the device and in the restatement -> (K, info)"""
    H.closed_map_clearance_configure(**cfg)
    K = KN.ClearNP(G, **cfg)
    assert K.build(misses)
    info = H.closed_map_clearance_build()
    print(f"{cfg}: {info}")
    same_field(H, K, info)
    return K, info


def same_points(H, K, pts, pose=None, misses=None):
    state, d2, dist, counts = H.closed_map_clearance_points(pts, pose)
    ws, wd, wdist, wc = K.points(pts, pose, misses)
    assert state.dtype == np.uint8 and d2.dtype == np.uint16 and dist.dtype == np.float64
    assert state.tobytes() == ws.tobytes() and d2.tobytes() == wd.tobytes() and bits(dist) == bits(wdist) and counts.tobytes() == wc.tobytes()
    return state, d2, dist, counts


def same_segments(H, K, S, E, radius, pose=None):
    status, d2, t, counts = H.closed_map_clearance_segments(S, E, radius, pose)
    ws, wd, wt, wc = K.segments(S, E, radius, pose)
    assert status.dtype == np.uint8 and d2.dtype == np.uint16 and t.dtype == np.float64
    assert status.tobytes() == ws.tobytes() and d2.tobytes() == wd.tobytes() and bits(t) == bits(wt) and counts.tobytes() == wc.tobytes()
    return status, d2, t, counts


def box_metric(G):
    lo = G.o + G.v * 4.0 * G.blo
    return lo, lo + G.v * 4.0 * G.nb


def same_queries(H, K, misses=None, seed=1, n=1500, bands=((0.5, 2.9, 1), (-1.0, 0.7, 2), (-1e6, 1e6, 3), (1e4, 1e4 + 10.0, 1))):
    """points (in the map frame and under a pose), segments at several radii and the columns are the restatement's"""
    G = K.G
    rng = np.random.default_rng(seed)
    pts = TF.probes(G, rng, misses, n=n)
    same_points(H, K, pts, misses=misses)
    lo, hi = box_metric(G)
    pose = LS.offset(np.eye(4), 0.7, 0.4)
    pose[:3, 3] += 0.5 * (lo + hi)
    local = np.ascontiguousarray((pts[:-5] - pose[:3, 3]) @ pose[:3, :3])
    same_points(H, K, local, pose, misses=misses)
    assert H.closed_map_clearance_points(pts, want_distance=False)[2] is None
    # segments all over the box and a little beyond it, short and long
    S = rng.uniform(lo - 1.0, hi + 1.0, (n, 3))
    E = np.where(rng.random((n, 1)) < 0.5, S + rng.normal(0.0, 2.0, (n, 3)), rng.uniform(lo - 1.0, hi + 1.0, (n, 3)))
    seen = set()
    for radius in (0.0, G.v, 0.5 * G.v * K.R, G.v * K.R):
        seen |= set(same_segments(H, K, S, E, radius)[0].tolist())
    assert len(seen) >= 2
    same_segments(H, K, np.ascontiguousarray((S - pose[:3, 3]) @ pose[:3, :3]), np.ascontiguousarray((E - pose[:3, 3]) @ pose[:3, :3]),
                  G.v, pose)
    assert len(bands) == 4 and G.band(*bands[3][:2]) == (1, 0)                     # four bands, the last one missing the box
    for z_lo, z_hi, min_free in bands:
        state, d2 = H.closed_map_clearance_columns(z_lo, z_hi, min_free)
        ws, wd = K.columns(z_lo, z_hi, min_free, misses)
        if G.band(z_lo, z_hi) == (1, 0):        # every column UNKNOWN: all obstacles, or none at all
            assert (ws == FN.UNKNOWN).all() and (wd == (0 if K.cfg["unknown_is_obstacle"] else B)).all()
        assert state.dtype == np.uint8 and d2.dtype == np.uint16 and d2.shape == (4 * G.nb[1], 4 * G.nb[0])
        assert state.tobytes() == ws.tobytes() == H.closed_map_free_columns(z_lo, z_hi, min_free).tobytes() and d2.tobytes() == wd.tobytes()


# ---- the scenes ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wall(hip_module):
    poses, clouds, scan, truth = LS.wall()
    H, V = built(hip_module, poses, clouds, CS.MASK, CS.GHOST["voxel"])
    G, _ = TF.free_built(H, V, poses, clouds, **WALL)
    yield H, V, G, poses, clouds, scan, truth
    H.close()


@pytest.mark.parametrize("R, wrap, want", [(4, 0, (175, 3023, 22548, 16)), (8, 0, (175, 10467, 324336, 64)),
                                           (4, 1, (237461, 238336, 1776, 9)), (8, 1, (237461, 238336, 1776, 9))])
def test_the_wall(wall, tmp_path, R, wrap, want):
    H, V, G, _, _, _, _ = wall
    K, info = cleared(H, G, max_distance=0.5 * R, unknown_is_obstacle=wrap)
    assert (info["obstacle_cells"], info["finite_cells"], info["sum_d2"], info["max_d2"]) == want
    assert (info["n_cells"], info["bytes"], info["radius_cells"]) == ((76, 56, 56), 4 * 76 * 56 * 56, R)
    same_queries(H, K)
    if R == 8:
        pts = np.array([(6, 2, 1.5), (6, 3.9, 1.5), (6, 0, 1.5), (6, 5.2, 1.5), (6, 4.7, 1.5), (6, 7, 1.5)], np.float64)
        assert same_points(H, K, pts)[1].tolist() == ([4, 4, 1, 0, 0, 0] if wrap else [36, 9, B, 0, 1, 16])
        state, d2 = H.closed_map_clearance_columns(0.5, 2.9)
        fin = d2[d2 != B].astype(np.int64)
        assert (len(fin), int(fin.sum()), int(fin.max())) == ((4256, 1674, 25) if wrap else (605, 15976, 64))
        # the PCD export, read back
        for ascii in (False, True):
            path = str(tmp_path / f"clear{int(ascii)}.pcd")
            cen = G.free_cells()
            assert map_io.write_clearance_pcd(path, H, ascii=ascii) == 875
            c2, dist = map_io.read_clearance_pcd(path)
            assert bits(c2) == bits(cen) and bits(dist) == bits(K.points(cen)[2]) and (np.isfinite(dist).sum() == (875 if wrap else 791))
        # two builds give the same bytes
        before = H.closed_map_clearance_field().tobytes()
        assert H.closed_map_clearance_build() == info and H.closed_map_clearance_field().tobytes() == before


def test_the_ghost_gate(hip_module):
    poses, clouds, _, _, _ = DS.ghost_gate()
    H, V = built(hip_module, poses, clouds, CS.MASK, DS.VOXEL)
    H.closed_map_carve_configure(max_range=DS.MAX_RANGE)
    H.closed_map_carve()
    M, _ = CN.carve(V, poses, clouds, CS.MASK, max_range=DS.MAX_RANGE)
    G, _ = TF.free_built(H, V, poses, clouds, max_range=DS.MAX_RANGE)
    K0, with_box = cleared(H, G, unknown_is_obstacle=0)
    same_queries(H, K0)
    G, _ = TF.free_built(H, V, poses, clouds, max_range=DS.MAX_RANGE, carve_gate=1)
    with not_ready(hip_module):
        H.closed_map_clearance_field()                                               # the free configure dropped the field
    K1, without = cleared(H, G, misses=M, unknown_is_obstacle=0)
    assert with_box["obstacle_cells"] - without["obstacle_cells"] == 8               # eight obstacles disappear from the field
    same_queries(H, K1, misses=M)
    C8 = V.centroids()[DS.box_voxels(V)]
    assert (K0.points(C8)[1] == 0).all() and (same_points(H, K1, C8, misses=M)[1] > 0).all()
    K, _ = cleared(H, G, misses=M, unknown_is_obstacle=1)
    same_queries(H, K, misses=M)
    # the gate on a map that is not carved: no build, no columns
    H.closed_map_carve_configure(max_range=11.0)
    for call in (H.closed_map_clearance_build, H.closed_map_clearance_field, lambda: H.closed_map_clearance_columns(0.0, 1.0),
                 lambda: H.closed_map_clearance_points(C8)):
        with not_ready(hip_module):
            call()
    H.close()


def test_the_static_pass_and_two_contexts(hip_module):
    poses, clouds = CS.static_pass()
    cfg = dict(max_range=CS.STATIC["max_range"])
    H, V = built(hip_module, poses, clouds, CS.MASK, CS.STATIC["voxel"])
    G, _ = TF.free_built(H, V, poses, clouds, **cfg)
    K, info = cleared(H, G, max_distance=4.0, unknown_is_obstacle=0)
    assert info["n_cells"] == (116, 88, 88) and info["radius_cells"] == 8 and 0 < info["obstacle_cells"] <= len(V.keys)
    same_queries(H, K, bands=((0.0, 2.0, 1), (-3.0, 6.0, 4), (-1e6, 1e6, 2), (1e4, 1e4 + 10.0, 1)))
    field = H.closed_map_clearance_field().tobytes()
    other, _ = built(hip_module, poses, clouds, CS.MASK, CS.STATIC["voxel"], reserve_voxels=64)
    other.closed_map_free_configure(**cfg)
    other.closed_map_free_build()
    other.closed_map_clearance_configure(max_distance=4.0, unknown_is_obstacle=0)
    assert other.closed_map_clearance_build() == info and other.closed_map_clearance_field().tobytes() == field
    K, info1 = cleared(H, G, max_distance=4.0, unknown_is_obstacle=1)
    assert info1["finite_cells"] == 116 * 88 * 88 and info1["launches"] == info["launches"]
    same_queries(H, K, bands=((0.0, 2.0, 1), (-3.0, 6.0, 4), (-1e6, 1e6, 2), (1e4, 1e4 + 10.0, 1)))
    H.close(); other.close()


# ---- hand-made maps over caller-given boxes --------------------------------------------------------------------------------------
def hand_map(reg, cells, voxel=1.0, origin=(0.0, 0.0, 0.0)):
    """a closed map whose voxels are exactly `cells` (and one far from every box, so that the map is never empty)"""
    cells = np.concatenate([np.asarray(cells, np.int64).reshape(-1, 3), [[5000, 5000, 5000]]])
    pts = np.asarray(origin, np.float64) + (cells.astype(np.float64) + 0.5) * voxel
    H, V = built(reg, [np.eye(4)], [CS.slot0(pts)], CS.MASK, voxel, origin)
    assert {tuple(c) for c in V.i.tolist()} == {tuple(c) for c in cells.tolist()}
    return H, V


def boxed(H, V, lo, hi, rays=None, **free_cfg):
    """the grid reset over [lo, hi]; rays: (scan, pose) walked into it, so that some cells are FREE"""
    G = TF.fresh(H, V, lo=lo, hi=hi, **free_cfg)
    if rays is not None:
        TF.scan_and_compare(H, G, *rays)
    return G


def corners(lo, hi):
    return [(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]


def star(centre, reach, n=400, seed=2):
    """a scan of n rays from `centre`, up to `reach` long -> (scan, pose)"""
    rng = np.random.default_rng(seed)
    pose = np.eye(4)
    pose[:3, 3] = centre
    d = rng.normal(size=(n, 3))
    return np.ascontiguousarray(d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.5, reach, (n, 1))), pose


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_long_lines(hip_module, axis):
    """1 x 1 x 150 bricks and the same along x and y at R = 128: 600-cell lines, every halo and tile seam crossed"""
    lo, hi = np.zeros(3, np.int64), np.full(3, 3, np.int64)
    hi[axis] = 599
    e = np.eye(3, dtype=np.int64)[axis]
    # the first and the last cell of the line, two obstacles R and R + 1 apart from their neighbours, a run of close ones
    at = [0, 599, 130, 130 + 128, 130 + 128 + 129, 400, 403, 404, 470]
    cells = [lo + k * e + np.array([1, 2, 3]) * (1 - e) for k in at]
    H, V = hand_map(hip_module, cells)
    G = boxed(H, V, lo, hi)
    K, info = cleared(H, G, max_distance=128.0, unknown_is_obstacle=0)
    assert info["radius_cells"] == 128 and info["obstacle_cells"] == len(at)
    line = [slice(None)] * 3
    for a in range(3):
        if a != axis:
            line[2 - a] = int(cells[0][a])
    row = K.d2[tuple(line)].astype(np.int64)
    assert row[130 + 64] == 64 * 64 and row[258 + 64] == 64 * 64 and row[258 + 65] == 64 * 64
    same_queries(H, K, n=600)
    # a second field: R = 127, so that 128 apart is beyond the truncation on the line itself
    K, _ = cleared(H, G, max_distance=127.0, unknown_is_obstacle=0)
    assert K.d2[tuple(line)][130 + 64] == 64 * 64 and K.R == 127
    # unknown an obstacle, after rays along the line have made cells FREE
    scan = np.array([(k + 0.25) * e + 0.0 for k in (5, 100, 300, 590)], np.float64)
    pose = np.eye(4)
    pose[:3, 3] = np.array([1.5, 2.5, 3.5]) * (1 - e) + 2.5 * e
    G = boxed(H, V, lo, hi, rays=(scan, pose), max_range=700.0, end_margin=0.0)
    K, info = cleared(H, G, max_distance=128.0, unknown_is_obstacle=1)
    assert info["finite_cells"] == 16 * 600 and 0 < info["obstacle_cells"] < 16 * 600
    same_queries(H, K, n=600)
    H.close()


def test_box_shapes_and_obstacle_placement(hip_module):
    reg = hip_module
    shapes = [((0, 0, 0), (3, 3, 3)),            # one brick
              ((-8, -4, -12), (-1, -1, -5)),     # at negative cells
              ((-6, -3, -2), (9, 4, 5)),         # straddling 0, lo not a multiple of 4
              ((1, 2, 3), (290, 9, 6))]          # lo not a multiple of 4, longer than one window's output on x at R = 128
    for lo, hi in shapes:
        blo, bhi = 4 * (np.array(lo) >> 2), 4 * (np.array(hi) >> 2) + 3      # the box the bricks make
        cells = corners(blo, bhi) + [tuple(blo + 1)]
        H, V = hand_map(reg, cells)
        G = boxed(H, V, lo, hi)
        for R in (1, 2, 128):
            K, info = cleared(H, G, max_distance=float(R), unknown_is_obstacle=0)
            assert info["obstacle_cells"] == 9 and info["radius_cells"] == R
            assert info["lo_cells"] == tuple(blo) and info["n_cells"] == tuple(bhi - blo + 1)
        same_queries(H, K, n=300, bands=((0.5, 2.5, 1), (-2.0, 0.9, 2), (-1e6, 1e6, 1), (1e4, 1e4 + 10.0, 1)))
        # rays from the middle, then unknown is an obstacle
        G = boxed(H, V, lo, hi, rays=star(0.5 * (blo + bhi + 1.0), 6.0), max_range=60.0, end_margin=0.0)
        for R in (1, 2, 128):
            K, info = cleared(H, G, max_distance=float(R), unknown_is_obstacle=1)
        assert info["finite_cells"] == int(np.prod(bhi - blo + 1))        # (R = 128: no cell is that far from the outside)
        same_queries(H, K, n=300, bands=((0.5, 2.5, 1), (-2.0, 0.9, 2), (-1e6, 1e6, 1), (1e4, 1e4 + 10.0, 1)))
        H.close()


def test_the_truncation_edge_and_empty_fields(hip_module):
    R = 5
    # pairs R and R + 1 apart on an axis and on a diagonal ((3, 4, 0) is 5 long, (3, 4, 1) is not)
    cells = [(0, 0, 0), (40, 0, 0), (0, 30, 0), (0, 0, 20), (40, 30, 20)]
    H, V = hand_map(hip_module, cells)
    G = boxed(H, V, (-8, -8, -8), (47, 39, 31))
    K, info = cleared(H, G, max_distance=float(R), unknown_is_obstacle=0)
    at = lambda c: int(K.d2[c[2] + 8, c[1] + 8, c[0] + 8])  # noqa: E731
    assert [at(c) for c in ((R, 0, 0), (R + 1, 0, 0), (0, -R, 0), (0, -R - 1, 0), (3, 4, 0), (3, 4, 1), (40, 30, 20 - R), (40, 30, 19 - R))] \
        == [R * R, B, R * R, B, R * R, B, R * R, B]
    assert info["max_d2"] == R * R and info["obstacle_cells"] == 5
    same_queries(H, K, n=400, bands=((0.5, 2.5, 1), (-2.0, 0.9, 2), (-1e6, 1e6, 1), (1e4, 1e4 + 10.0, 1)))
    # a box narrower than R on every axis
    G = boxed(H, V, (0, 0, 0), (3, 3, 3))
    K, info = cleared(H, G, max_distance=100.0, unknown_is_obstacle=0)
    assert info["finite_cells"] == 64 and info["max_d2"] == 27 and info["radius_cells"] == 100
    K, info = cleared(H, G, max_distance=100.0, unknown_is_obstacle=1)
    assert info["obstacle_cells"] == 64                                              # a freshly reset grid: all 0
    # no obstacle at all
    G = boxed(H, V, (100, 100, 100), (111, 107, 103))
    K, info = cleared(H, G, max_distance=3.0, unknown_is_obstacle=0)
    assert (info["obstacle_cells"], info["finite_cells"], info["sum_d2"], info["max_d2"]) == (0, 0, 0, 0)
    assert (H.closed_map_clearance_field() == B).all()
    state, d2 = H.closed_map_clearance_columns(-1e6, 1e6)
    assert (d2 == B).all() and (state == FN.UNKNOWN).all()
    same_queries(H, K, n=200, bands=((0.5, 2.5, 1), (-2.0, 0.9, 2), (-1e6, 1e6, 1), (1e4, 1e4 + 10.0, 1)))
    K, info = cleared(H, G, max_distance=3.0, unknown_is_obstacle=1)
    assert info["obstacle_cells"] == 12 * 8 * 4 and (H.closed_map_clearance_field() == 0).all()
    H.close()


# ---- segments --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025])
def test_segment_batches(wall, n):
    H, V, G, _, _, scan, truth = wall
    K, _ = cleared(H, G, unknown_is_obstacle=0)
    idx = np.arange(100, 100 + n) % len(scan)
    S = np.tile(truth[:3, 3], (n, 1)) + 0.01 * (idx[:, None] % 7)
    status, _, _, counts = same_segments(H, K, S, CN.transform(truth, scan[idx]), 0.5)
    assert counts.sum() == n and counts[KN.BLOCKED] > 0
    same_segments(H, K, np.ascontiguousarray(S - truth[:3, 3]), scan[idx], 0.25, truth)


@pytest.mark.parametrize("t", [(6.25, 0.25, 1.25), (6.0, 0.0, 2.0), (-1.75, -3.25, -0.75)])
def test_hand_made_segments(wall, hip_module, t):
    """section 29's ray list: NaN and Inf ends, zero length, ends beyond the grid, a segment inside one cell, axis-parallel ones
    along a brick edge, diagonals whose tMax ties on two and three axes"""
    H, V, G, _, _, _, _ = wall
    t = np.array(t)
    world = np.concatenate([TF.hand_made_world(t), [t + [0.0, 130.0, 0.0]]])          # ... and one beyond max_segment
    S = np.tile(t, (len(world), 1))
    for wrap in (0, 1):
        K, _ = cleared(H, G, unknown_is_obstacle=wrap)
        radii = (0.0, 0.5, 1.0, 1.25, 4.0, 4.03)         # 0, k * voxel, and the largest the field allows: need = 65 = R * R + 1
        for radius in radii:
            status, _, _, counts = same_segments(H, K, S, world, radius)
            assert counts[KN.SKIPPED] == 7
        with invalid(hip_module):
            H.closed_map_clearance_segments(S, world, 4.04)                             # one step beyond
        assert K.segments(S, world, 4.04) is None
        for R in (Rz90, LS.offset(np.eye(4), 0.0, 0.3)[:3, :3]):
            pose = np.eye(4)
            pose[:3, :3], pose[:3, 3] = R, t
            with np.errstate(invalid="ignore"):
                local = np.ascontiguousarray((world - t) @ R)
            same_segments(H, K, np.zeros_like(local), local, 0.5, pose)
            same_segments(H, K, np.zeros_like(local), local, 0.0, pose)
    # the longest segment is the configuration's
    K, _ = cleared(H, G, unknown_is_obstacle=0, max_segment=3.0)
    assert same_segments(H, K, S, world, 0.5)[3][KN.SKIPPED] > 7


# ---- lifetime ----------------------------------------------------------------------------------------------------------------------
def test_what_drops_the_field(hip_module):
    reg = hip_module
    poses, clouds, scan, truth = LS.wall()
    v = CS.GHOST["voxel"]
    H = context(reg, poses, clouds, keep=range(5), voxel=v, cloud_mask=CS.MASK)
    zero = reg.ClearanceInfo().as_dict()
    assert H.closed_map_clearance_info() == zero
    with not_ready(reg):
        H.closed_map_clearance_build()                                                # no map
    H.closed_map_build(2, poses[:5])
    with not_ready(reg):
        H.closed_map_clearance_build()                                                # no grid
    H.closed_map_free_configure(**WALL)
    lo, hi = FN.auto_box(poses, v, (0.0, 0.0, 0.0), 12.0)
    H.closed_map_free_build(lo, hi)
    cfg = dict(max_distance=4.0, unknown_is_obstacle=0)
    H.closed_map_clearance_configure(**cfg)

    def reads():
        return (H.closed_map_clearance_field, lambda: H.closed_map_clearance_points(scan),
                lambda: H.closed_map_clearance_segments(scan, scan + 1.0, 0.5))

    def gone(grid=True):
        assert H.closed_map_clearance_info() == zero
        for call in reads():
            with not_ready(reg):
                call()
        if grid:
            H.closed_map_clearance_columns(0.5, 2.9)                                  # (computed from the grid: no field needed)
        return True

    assert gone()
    info = H.closed_map_clearance_build()
    field = H.closed_map_clearance_field().tobytes()
    drops = [(H.closed_map_free_add_keyframes, True), (lambda: H.closed_map_free_add_scan(scan[:50], truth), True),
             (H.closed_map_carve, True), (lambda: H.closed_map_carve_configure(max_range=11.0), True),
             (lambda: H.closed_map_clearance_configure(**cfg), True), (lambda: H.closed_map_free_reset(lo, hi), True),
             (lambda: H.closed_map_free_configure(**WALL), False)]
    for k, (drop, grid) in enumerate(drops):
        drop()
        assert gone(grid), k
        H.closed_map_free_build(lo, hi)                                               # back to the keyframes' grid
        assert H.closed_map_clearance_build() == info and H.closed_map_clearance_field().tobytes() == field, k
    # an extend: the new keyframe's voxels are obstacles of the next build, which equals a fresh context's
    assert H.place_add_scan(TF.TV.DUMMY, poses[5], 5) == 5
    H.place_set_keyframe_clouds(5, *clouds[5])
    H.closed_map_extend(2, poses[5:6])
    assert gone()
    H.closed_map_free_add_keyframes()
    after = H.closed_map_clearance_build()
    F, V = built(reg, poses, clouds, CS.MASK, v)
    F.closed_map_free_configure(**WALL)
    F.closed_map_free_build(lo, hi)
    F.closed_map_clearance_configure(**cfg)
    assert F.closed_map_clearance_build() == after and F.closed_map_clearance_field().tobytes() == H.closed_map_clearance_field().tobytes()
    G = FN.FreeNP(V, **WALL)
    G.reset(lo, hi)
    G.add_keyframes(poses, clouds, CS.MASK)
    K = KN.ClearNP(G, **cfg)
    assert K.build()
    same_field(H, K, after)
    # a build of the map, a load and an odometry reset drop it with the grid; the configuration persists
    blob = H.closed_map_save()
    H.closed_map_load(blob)
    assert gone(grid=False)
    F.closed_map_build(2, poses)
    assert F.closed_map_clearance_info() == zero
    F.closed_map_free_build(lo, hi)
    assert F.closed_map_clearance_build() == after
    F.odometry_reset(None, TS.TC.odom_cfg(reg))
    assert F.closed_map_clearance_info() == zero
    for k in range(len(poses)):
        assert F.place_add_scan(TS.DUMMY, np.eye(4), k) == k
        F.place_set_keyframe_clouds(k, *clouds[k])
    F.closed_map_build(2, poses)
    F.closed_map_free_build(lo, hi)
    assert F.closed_map_clearance_build() == after                                   # max_distance 4, unknown not an obstacle: still there
    H.close(); F.close()


def test_refusals_leave_the_field(wall, hip_module):
    reg = hip_module
    H, V, G, poses, clouds, scan, truth = wall
    K, info = cleared(H, G, unknown_is_obstacle=0)
    field = H.closed_map_clearance_field().tobytes()

    def untouched():
        return H.closed_map_clearance_field().tobytes() == field and H.closed_map_clearance_info() == info

    for bad in (dict(max_distance=0.0), dict(max_distance=-1.0), dict(max_distance=float("inf")), dict(max_distance=float("nan")),
                dict(max_segment=0.0), dict(max_segment=float("inf")), dict(max_segment=float("nan")), dict(max_bytes=1),
                dict(max_bytes=-1), dict(unknown_is_obstacle=2), dict(unknown_is_obstacle=-1)):
        with invalid(reg):
            H.closed_map_clearance_configure(**bad)
    with pytest.raises(KeyError):
        H.closed_map_clearance_configure(radius=1.0)
    assert untouched()
    # refused queries write nothing
    n = len(scan)
    flat = np.ascontiguousarray(scan).ctypes.data_as(C.POINTER(C.c_double))
    state, d2 = np.full(n, 9, np.uint8), np.full(n, 9, np.uint16)
    sp, dp = state.ctypes.data_as(C.POINTER(C.c_uint8)), d2.ctypes.data_as(C.POINTER(C.c_uint16))
    L = H.L
    assert L.tloam_closed_map_clearance_points(H.h, None, n, None, sp, dp, None, None) == -1
    assert L.tloam_closed_map_clearance_points(H.h, flat, 0, None, sp, dp, None, None) == -1
    assert L.tloam_closed_map_clearance_points(H.h, flat, n, None, None, dp, None, None) == -1
    assert L.tloam_closed_map_clearance_points(H.h, flat, n, None, sp, None, None, None) == -1
    assert L.tloam_closed_map_clearance_segments(H.h, None, flat, n, None, 0.5, sp, dp, None, None) == -1
    assert L.tloam_closed_map_clearance_segments(H.h, flat, None, n, None, 0.5, sp, dp, None, None) == -1
    assert L.tloam_closed_map_clearance_segments(H.h, flat, flat, 0, None, 0.5, sp, dp, None, None) == -1
    assert L.tloam_closed_map_clearance_segments(H.h, flat, flat, n, None, 0.5, None, dp, None, None) == -1
    assert L.tloam_closed_map_clearance_segments(H.h, flat, flat, n, None, 0.5, sp, None, None, None) == -1
    for radius in (-0.5, float("nan"), float("inf"), 4.04, 1e200):
        assert L.tloam_closed_map_clearance_segments(H.h, flat, flat, n, None, radius, sp, dp, None, None) == -1
    for bad_pose in (2.0 * np.eye(4), np.full((4, 4), np.nan), np.diag([1.0, 1.0, -1.0, 1.0])):
        with invalid(reg):
            H.closed_map_clearance_points(scan, bad_pose)
        with invalid(reg):
            H.closed_map_clearance_segments(scan, scan, 0.5, bad_pose)
    with pytest.raises(ValueError):
        H.closed_map_clearance_segments(scan, scan[:-1], 0.5)
    assert (state == 9).all() and (d2 == 9).all() and untouched()
    # the optional outputs may be left out
    assert L.tloam_closed_map_clearance_segments(H.h, flat, flat, n, None, 0.5, sp, dp, None, None) == 0 and (state == KN.SKIPPED).all()
    # the columns: the free columns' refusals and capacity convention
    for z_lo, z_hi, min_free in ((2.0, 1.0, 1), (np.nan, 1.0, 1), (0.0, np.inf, 1), (0.0, 1.0, 0)):
        with invalid(reg):
            H.closed_map_clearance_columns(z_lo, z_hi, min_free)
    nx, ny = C.c_size_t(0), C.c_size_t(0)
    col = np.full(76 * 56, 9, np.uint16)
    up = col.ctypes.data_as(C.POINTER(C.c_uint16))
    assert L.tloam_closed_map_clearance_columns(H.h, 0.5, 2.9, 1, None, up, 76 * 56 - 1, C.byref(nx), C.byref(ny)) == -1
    assert (nx.value, ny.value) == (76, 56) and (col == 9).all()
    assert L.tloam_closed_map_clearance_columns(H.h, 0.5, 2.9, 1, None, None, 76 * 56, C.byref(nx), C.byref(ny)) == -1
    assert L.tloam_closed_map_clearance_columns(H.h, 0.5, 2.9, 1, None, up, 76 * 56, C.byref(nx), C.byref(ny)) == 0
    assert col.tobytes() == H.closed_map_clearance_columns(0.5, 2.9)[1].tobytes() == K.columns(0.5, 2.9)[1].tobytes()
    # a range beyond the field
    cells = 76 * 56 * 56
    one = np.zeros(4, np.uint16)
    op = one.ctypes.data_as(C.POINTER(C.c_uint16))
    assert L.tloam_closed_map_read_clearance(H.h, cells, 1, op) == -1 and L.tloam_closed_map_read_clearance(H.h, cells, 0, op) == 0
    assert L.tloam_closed_map_read_clearance(H.h, cells - 1, 1, op) == 0 and one[0] == K.d2.ravel()[-1]
    assert L.tloam_closed_map_read_clearance(H.h, 5, 3, op) == 0 and one[:3].tobytes() == K.d2.ravel()[5:8].tobytes()
    assert L.tloam_closed_map_read_clearance(H.h, 0, 1, None) == -1 and untouched()
    # a build that is refused: R = 0 cannot be configured (max_distance > 0 gives R >= 1); R = 129 and over max_bytes.  A
    # configure drops the field, so what is left untouched is that there is none
    zero = reg.ClearanceInfo().as_dict()
    for cfg in (dict(max_distance=64.1), dict(max_distance=1e9), dict(max_bytes=4 * cells - 1)):
        H.closed_map_clearance_configure(unknown_is_obstacle=0, **cfg)
        with invalid(reg):
            H.closed_map_clearance_build()
        assert H.closed_map_clearance_info() == zero
        if "max_distance" in cfg:
            with invalid(reg):
                H.closed_map_clearance_columns(0.5, 2.9)
    # the column call's two layers are held to max_bytes too: 4 bytes a column
    H.closed_map_clearance_configure(unknown_is_obstacle=0, max_bytes=4 * 76 * 56 - 1)
    with invalid(reg):
        H.closed_map_clearance_columns(0.5, 2.9)
    H.closed_map_clearance_configure(unknown_is_obstacle=0, max_bytes=4 * 76 * 56)
    assert H.closed_map_clearance_columns(0.5, 2.9)[1].tobytes() == K.columns(0.5, 2.9)[1].tobytes()
    H.closed_map_clearance_configure(unknown_is_obstacle=0, max_distance=64.0, max_bytes=4 * cells)
    assert H.closed_map_clearance_build()["radius_cells"] == 128
    H.closed_map_clearance_configure(unknown_is_obstacle=0)
    assert H.closed_map_clearance_build() == info and untouched()
    # nranks > 1: every call is refused
    X = reg.HipRegistration()
    X.comm_init_callback(0, 2, lambda dev, count, stream: 0)
    for call in (X.closed_map_clearance_configure, X.closed_map_clearance_info, X.closed_map_clearance_build,
                 lambda: X.closed_map_clearance_points(scan), lambda: X.closed_map_clearance_segments(scan, scan, 0.5)):
        with invalid(reg):
            call()
    assert X.L.tloam_closed_map_read_clearance(X.h, 0, 0, None) == -1
    assert X.L.tloam_closed_map_clearance_columns(X.h, 0.0, 1.0, 1, None, up, 0, C.byref(nx), C.byref(ny)) == -1
    X.close()


def test_clearance_changes_nothing_else(hip_module):
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
    prior = LS.offset(pose, 0.1, 0.01)

    def everything(X):
        rows = X.closed_map_read()
        found = X.closed_map_localise(scan, prior)
        through, hits = X.closed_map_diff_counts()
        return (bits(rows[0]) + rows[1].tobytes(), X.closed_map_misses().tobytes(), TS.surfel_bytes(X), X.closed_map_free_words().tobytes(),
                X.closed_map_free_info(), through.tobytes() + hits.tobytes(), bits(found[0]), {**found[1], "prepared": 0},
                log_bytes(X.closed_map_localise_log()), {**X.closed_map_diff_info(), "prepared": 0, "launches": 0},
                X.closed_map_save(), X.closed_map_save(clouds=True))

    before = everything(H)
    M = H.closed_map_misses()
    for wrap in (0, 1):
        K, _ = cleared(H, G, misses=M, unknown_is_obstacle=wrap)
        same_queries(H, K, misses=M, n=500)
        assert everything(H) == before
    # the other stages that do not change what the field was built from leave it: a surfel pass, a diff, a localise
    field, info = H.closed_map_clearance_field().tobytes(), H.closed_map_clearance_info()
    H.closed_map_surfels(); H.closed_map_diff(scan, pose)
    assert everything(H) == before and H.closed_map_clearance_field().tobytes() == field and H.closed_map_clearance_info() == info
    H.close()
