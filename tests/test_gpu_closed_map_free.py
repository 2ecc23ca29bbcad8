"""-m gpu: the free space of the closed map (tl_free.hip, tl_api_free.hip) against its numpy restatement
(tests/closed_map_free_np.py), bit for bit: the grid's words, the states, ids, cell lists, columns and every counter.  Keyframes
are hand-made as in tests/test_gpu_closed_map_carve.py and built under the caller's poses (pose_source 2)."""
import ctypes as C
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
import test_gpu_closed_map_carve as TV  # noqa: E402
import test_gpu_closed_map_localise as TL  # noqa: E402
import test_gpu_closed_map_surfel as TS  # noqa: E402
from tloam_amd import map_io  # noqa: E402

pytestmark = pytest.mark.gpu

bits, invalid, not_ready, built, context, log_bytes = TL.bits, TL.invalid, TL.not_ready, TV.built, TV.context, TL.log_bytes
WALL = dict(max_range=12.0, end_margin=1.0)
Rz90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
UNCOUNTED = ("launches",)


def same_grid(H, G, info=None):
    """the device's words and info are the restatement's"""
    want = G.info()
    got = H.closed_map_free_info()
    if info is not None:
        assert info == got
    assert {k: v for k, v in got.items() if k not in UNCOUNTED} == want
    words = H.closed_map_free_words()
    assert words.dtype == np.uint64 and words.tobytes() == G.words.tobytes()
    if len(words) >= 3:
        assert H.closed_map_free_words(1, 2).tobytes() == G.words[1:3].tobytes()
    return got


def probes(G, rng, misses=None, n=4000):
    """points that meet every state: the map's centroids, the free cells' centres, points all over the box and beyond it, and the
    ones no cell holds"""
    lo = G.o + G.v * 4.0 * G.blo
    hi = lo + G.v * 4.0 * G.nb
    cen = G.free_cells(misses=misses)
    return np.concatenate([G.V.centroids()[:2000], cen[:: max(len(cen) // 500, 1)], rng.uniform(lo - 3.0, hi + 3.0, (n, 3)),
                           [[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [G.o[0] + G.v * 2.0 ** 20, 0.0, 0.0],
                            [0.0, G.o[1] - G.v * (2.0 ** 20 + 1.0), 0.0]]])


def same_reads(H, G, misses=None, seed=1, bands=((0.5, 2.9, 1), (-1.0, 0.7, 2), (-1e6, 1e6, 3), (50.0, 60.0, 1))):
    """occupancy, the cell list (whole and boxed) and the columns are the restatement's"""
    pts = probes(G, np.random.default_rng(seed), misses)
    state, ids, counts = H.closed_map_occupancy(pts, want_ids=True)
    ws, wi, wc = G.occupancy(pts, misses=misses)
    assert state.dtype == np.uint8 and ids.dtype == np.int32
    assert state.tobytes() == ws.tobytes() and ids.tobytes() == wi.tobytes() and counts.tobytes() == wc.tobytes()
    assert (counts > 0).sum() >= 3 and H.closed_map_occupancy(pts)[1] is None
    # ... and in the sensor frame of a pose
    pose = LS.offset(np.eye(4), 0.7, 0.4)
    pose[:3, 3] += G.o + G.v * 4.0 * (G.blo + 0.5 * G.nb)
    local = np.ascontiguousarray((pts[:-5] - pose[:3, 3]) @ pose[:3, :3])
    state, ids, counts = H.closed_map_occupancy(local, pose, want_ids=True)
    ws, wi, wc = G.occupancy(local, pose, misses=misses)
    assert state.tobytes() == ws.tobytes() and ids.tobytes() == wi.tobytes() and counts.tobytes() == wc.tobytes()
    cen = H.closed_map_free_cells()
    want = G.free_cells(misses=misses)
    assert bits(cen) == bits(want)
    if len(want):
        lo, hi = np.quantile(want, 0.25, axis=0), np.quantile(want, 0.8, axis=0)
        part = G.free_cells(lo, hi, misses=misses)
        assert bits(H.closed_map_free_cells(lo, hi)) == bits(part) and (len(want) < 50 or 0 < len(part) < len(want))
        assert bits(H.closed_map_free_cells(want[0], want[0])) == bits(want[:1])      # the box is inclusive
    for z_lo, z_hi, min_free in bands:
        col = H.closed_map_free_columns(z_lo, z_hi, min_free)
        assert col.dtype == np.uint8 and col.shape == (4 * G.nb[1], 4 * G.nb[0])
        assert col.tobytes() == G.columns(z_lo, z_hi, min_free, misses=misses).tobytes()
    return want


def free_built(H, V, poses, clouds, mask=CS.MASK, lo=None, hi=None, **cfg):
    """the grid configured, reset and filled from the keyframes on the device and in the restatement -> (G, info)"""
    H.closed_map_free_configure(**cfg)
    G = FN.FreeNP(V, **cfg)
    assert G.reset(lo, hi, poses=poses)
    G.add_keyframes(poses, clouds, cfg.get("ray_mask") or mask)
    info = H.closed_map_free_build(lo, hi)
    print(f"{cfg} box {lo} {hi}: {info}")
    assert info["launches"] == 2
    same_grid(H, G, info)
    return G, info


# ---- the scenes, built once --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wall(hip_module):
    poses, clouds, scan, truth = LS.wall()
    H, V = built(hip_module, poses, clouds, CS.MASK, CS.GHOST["voxel"])
    yield H, V, poses, clouds, scan, truth
    H.close()


# ---- 1: the scenes -----------------------------------------------------------------------------------------------------------
def test_the_wall(wall, hip_module, tmp_path):
    reg = hip_module
    H, V, poses, clouds, _, _ = wall
    G, info = free_built(H, V, poses, clouds, **WALL)
    assert (info["rays"], info["skipped_rays"], info["cells_marked"], info["cells_outside"]) == (5757, 0, 98767, 0)
    assert (info["free_cells"], info["n_bricks"], info["keyframes"], info["scans"]) == (875, (19, 14, 14), 6, 0)
    pts = np.array([(6, 2, 1.5), (6, 3.9, 1.5), (6, 0, 1.5), (6, 5.2, 1.5), (6, 4.7, 1.5), (6, 5.7, 1.5), (6, 7, 1.5), (6, -3, 1.5),
                    (6, 2, 4.5), (6, 2, -0.5)], np.float64)
    F, X, U = reg.OCCUPANCY_FREE, reg.OCCUPANCY_OCCUPIED, reg.OCCUPANCY_UNKNOWN
    state, ids, counts = H.closed_map_occupancy(pts, want_ids=True)
    assert list(state) == [F, F, F, X, U, U, U, U, U, U] and list(counts) == [0, 6, 3, 1] and ids[3] >= 0 and (np.delete(ids, 3) == -1).all()
    assert len(same_reads(H, G)) == 875
    col = H.closed_map_free_columns(0.5, 2.9)
    x0, y0 = -info["lo_cells"][0], -info["lo_cells"][1]
    assert (col[y0 + 10, x0:x0 + 25] == X).all() and not (col[y0 + 11:] == F).any() and not (col[:y0] == F).any()
    # the PCD export of the free cells
    path = str(tmp_path / "free.pcd")
    assert map_io.write_free_pcd(path, H) == 875 and bits(map_io.read_pcd(path)) == bits(G.free_cells())
    # a second add over the same keyframes finds nothing new to walk: the grid holds them all
    again = H.closed_map_free_add_keyframes()
    assert (again["rays"], again["cells_marked"], again["free_cells"], again["keyframes"]) == (0, 0, 875, 6)
    assert H.closed_map_free_words().tobytes() == G.words.tobytes()


def test_the_ghost_gate(hip_module):
    reg = hip_module
    poses, clouds, _, _, _ = DS.ghost_gate()
    H, V = built(reg, poses, clouds, CS.MASK, DS.VOXEL)
    H.closed_map_carve_configure(max_range=DS.MAX_RANGE)
    H.closed_map_carve()
    M, _ = CN.carve(V, poses, clouds, CS.MASK, max_range=DS.MAX_RANGE)
    assert H.closed_map_misses().tobytes() == M.tobytes()
    box = DS.box_voxels(V)
    C = V.centroids()[box]
    G, info = free_built(H, V, poses, clouds, max_range=DS.MAX_RANGE)
    assert (info["rays"], info["cells_marked"], info["free_cells"]) == (5821, 99423, 875) and len(box) == 8
    state, ids, _ = H.closed_map_occupancy(C, want_ids=True)
    assert (state == reg.OCCUPANCY_OCCUPIED).all() and np.array_equal(ids, box)
    same_reads(H, G)
    G, _ = free_built(H, V, poses, clouds, max_range=DS.MAX_RANGE, carve_gate=1)
    state, ids, _ = H.closed_map_occupancy(C, want_ids=True)
    assert (state == reg.OCCUPANCY_FREE).all() and (ids == -1).all()
    assert len(same_reads(H, G, misses=M)) == 875
    # another rule of the gate, and min_count
    G, _ = free_built(H, V, poses, clouds, max_range=DS.MAX_RANGE, carve_gate=1, min_miss=125, miss_ratio=0.5)
    assert 0 < (H.closed_map_occupancy(C)[0] == reg.OCCUPANCY_FREE).sum() < 8
    same_reads(H, G, misses=M)
    G, _ = free_built(H, V, poses, clouds, max_range=DS.MAX_RANGE, min_count=9)
    assert 0 < (G.occupancy(V.centroids())[0] != reg.OCCUPANCY_OCCUPIED).sum() < len(V.keys)
    same_reads(H, G)
    # the gate on a map that is not carved: the adds run, the reads are refused
    H.closed_map_carve_configure(max_range=11.0)
    H.closed_map_free_configure(max_range=DS.MAX_RANGE, carve_gate=1)
    H.closed_map_free_build()
    for call in (lambda: H.closed_map_occupancy(C), H.closed_map_free_cells, lambda: H.closed_map_free_columns(0.0, 1.0)):
        with not_ready(reg):
            call()
    H.close()


def test_the_static_pass_and_two_contexts(hip_module):
    poses, clouds = CS.static_pass()
    cfg = dict(max_range=CS.STATIC["max_range"])
    H, V = built(hip_module, poses, clouds, CS.MASK, CS.STATIC["voxel"])
    G, info = free_built(H, V, poses, clouds, **cfg)
    assert (info["rays"], info["skipped_rays"], info["cells_marked"], info["cells_outside"]) == (152074, 15702, 2870271, 0)
    assert (info["free_cells"], info["n_bricks"]) == (16575, (29, 22, 22))
    assert len(same_reads(H, G, bands=((0.0, 2.0, 1), (-3.0, 6.0, 4)))) == 16575 - 3263
    words = H.closed_map_free_words().tobytes()
    assert H.closed_map_free_build() == info and H.closed_map_free_words().tobytes() == words      # again: the same bytes
    other, _ = built(hip_module, poses, clouds, CS.MASK, CS.STATIC["voxel"], reserve_voxels=64)
    other.closed_map_free_configure(**cfg)
    assert other.closed_map_free_build() == info and other.closed_map_free_words().tobytes() == words
    assert bits(other.closed_map_free_cells()) == bits(H.closed_map_free_cells())
    # a ray mask of its own: no cloud of the source side holds a point here, so no ray is walked
    H.closed_map_free_configure(ray_mask=0x01, **cfg)
    assert (H.closed_map_free_build()["rays"], H.closed_map_free_info()["free_cells"]) == (0, 0)
    H.close(); other.close()


@pytest.mark.parametrize("turn", ["quarter", "general"])
def test_the_wall_turned(hip_module, turn):
    poses, clouds, _, _ = LS.wall()
    T = np.eye(4)
    if turn == "quarter":
        T[:3, :3], T[:3, 3] = Rz90, [1.5, -2.25, 0.5]
    else:
        T = LS.offset(T, 3.0, 0.7)
    poses = np.array([T @ np.asarray(P) for P in poses])
    H, V = built(hip_module, poses, clouds, CS.MASK, CS.GHOST["voxel"])
    G, info = free_built(H, V, poses, clouds, **WALL)
    assert info["rays"] == 5757 and info["skipped_rays"] == 0 and info["cells_outside"] == 0 and info["free_cells"] > 500
    same_reads(H, G)
    H.close()


# ---- 2: a scan's rays --------------------------------------------------------------------------------------------------------
def scan_and_compare(H, G, scan, pose):
    info = H.closed_map_free_add_scan(scan, pose)
    G.add_scan(scan, pose)
    assert info["launches"] == 2
    return same_grid(H, G, info)


def fresh(H, V, poses=None, lo=None, hi=None, **cfg):
    H.closed_map_free_configure(**cfg)
    G = FN.FreeNP(V, **cfg)
    assert G.reset(lo, hi, poses=poses)
    info = H.closed_map_free_reset(lo, hi)
    assert info["launches"] == 1 and info["free_cells"] == 0
    same_grid(H, G, info)
    return G


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_add_scan_block_boundaries(wall, n):
    """every ray of a scan leaves the one origin: they all cross the same first bricks"""
    H, V, poses, _, scan, truth = wall
    G = fresh(H, V, poses, **WALL)
    info = scan_and_compare(H, G, scan[np.arange(100, 100 + n) % len(scan)], LS.offset(truth, 0.1, 0.01))
    assert info["rays"] == n and info["scans"] == 1 and info["cells_marked"] > 0
    if n == 1025:
        info = scan_and_compare(H, G, scan[:700], truth)      # a second scan adds to the first
        assert info["scans"] == 2
        same_reads(H, G)


def hand_made_world(t):
    return np.array([
        [np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [-np.inf, np.nan, 0.0],           # 0-2: not finite
        [2.0 ** 19 + 5.0, 0.0, 0.0], [0.0, -(2.0 ** 19) - 5.0, 1.0],               # 3-4: beyond the grid at v = 0.5
        t,                                                                         # 5: at the sensor: L == 0
        t + [0.0, 30.0, 0.0],                                                      # 6: beyond max_range = 12
        t + [0.125, 0.0625, -0.125],                                               # 7: inside the sensor's cell: 0 steps
        t + [0.75, 0.0, 0.0], t + [0.0, -1.0, 0.0], t + [0.5, 0.5, 0.5],            # 8-10: L <= end_margin = 1: marks nothing
        t + [4.0, 0.0, 0.0], t + [0.0, 4.75, 0.0], t + [0.0, 0.0, -1.5],            # 11-13: axis-parallel, d == 0 on two axes
        t + [-3.0, 0.0, 0.0], t + [0.0, -11.0, 0.0], t + [0.0, 0.0, 7.0],           # 14-16: ... the long ones
        t + [2.0, 2.0, 0.0], t + [-1.5, 1.5, 0.0], t + [0.0, 2.5, 2.5],            # 17-19: tMax ties on two axes
        t + [2.0, 2.0, 2.0], t + [-1.0, 1.0, -1.0], t + [1.5, 4.5, 1.5],           # 20-22: ... and on three (22: not a diagonal)
        t + [6.0, 6.0, 6.0], t + [-5.0, -5.0, 5.0],                                # 23-24: long diagonals: a brick change at nearly every step
        t + [0.5, 4.75, 0.0], t + [-0.5, 4.75, 0.5],                                # 25-26: onto the wall
    ])


@pytest.mark.parametrize("t", [(6.25, 0.25, 1.25), (6.0, 0.0, 2.0), (-1.75, -3.25, -0.75)])
def test_hand_made_rays(wall, t):
    """t: a dyadic cell centre (the diagonals tie from the first step), a brick corner (the axis-parallel rays run along brick
    edges), a cell centre at negative cells"""
    H, V, poses, _, _, _ = wall
    t = np.array(t)
    for R in (np.eye(3), Rz90):
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3] = R, t
        world = hand_made_world(t)
        with np.errstate(invalid="ignore"):
            scan = np.ascontiguousarray((world - t) @ R)
        assert np.array_equal(CN.transform(pose, scan)[5:], world[5:])            # the pose gives the world points back exactly
        G = fresh(H, V, poses, **WALL)
        info = scan_and_compare(H, G, scan, pose)
        assert info["skipped_rays"] == 7 and info["cells_marked"] > 50
        if t[0] == 6.25:
            walk = CN.Walk(np.tile(t / 0.5, (5, 1)), world[20:25] / 0.5)
            assert ((walk.tmax == walk.tmax.min(axis=1, keepdims=True)).sum(axis=1)[[0, 1, 3, 4]] == 3).all()
        # one ray at a time: 7 - 10 mark nothing
        for k in (7, 8, 9, 10):
            G1 = fresh(H, V, poses, **WALL)
            assert scan_and_compare(H, G1, scan[k:k + 1], pose)["cells_marked"] == 0
        # a box the long rays leave
        G2 = fresh(H, V, lo=(8, -4, 0), hi=(19, 7, 7), **WALL)
        info = scan_and_compare(H, G2, scan, pose)
        assert info["cells_outside"] > 0
    # a turned pose that rounds
    G = fresh(H, V, poses, **WALL)
    scan_and_compare(H, G, scan, LS.offset(pose, 0.05, 0.3))
    same_reads(H, G)


# ---- 3: negative coordinates and caller-given boxes ----------------------------------------------------------------------------
def test_negative_cells(hip_module):
    """a map origin that puts every cell at negative indices: the floor of >> 2 and & 3"""
    poses, clouds, _, _ = LS.wall()
    origin = (100.0, 80.0, 40.0)
    H, V = built(hip_module, poses, clouds, CS.MASK, CS.GHOST["voxel"], origin)
    G, info = free_built(H, V, poses, clouds, **WALL)
    assert (V.i < 0).all() and max(info["lo_cells"][a] + 4 * info["n_bricks"][a] for a in range(3)) < 0
    assert (info["cells_marked"], info["free_cells"]) == (98767, 875)              # the wall's figures: the grid only shifted
    same_reads(H, G, bands=((0.5, 2.9, 1), (-1e6, 1e6, 3)))
    H.close()


def test_caller_given_boxes(wall):
    H, V, poses, clouds, _, _ = wall
    whole, _ = free_built(H, V, poses, clouds, **WALL)
    # lo not a multiple of 4, the box straddling 0 on y
    G, info = free_built(H, V, poses, clouds, lo=(-3, -7, 1), hi=(17, 9, 3), **WALL)
    assert info["lo_cells"] == (-4, -8, 0) and info["n_bricks"] == (6, 5, 1) and info["bytes"] == 8 * 30
    assert info["cells_outside"] > 0 and info["cells_marked"] + info["cells_outside"] == 98767
    assert len(H.closed_map_free_words()) == 30                                    # a word count that is exact
    same_reads(H, G)
    # what the small box holds is what the whole grid holds there
    cen = G.free_cells()
    big ={tuple(c) for c in whole.free_cells().tolist()}
    assert {tuple(c) for c in cen.tolist()} <= big and 0 < len(cen) < len(big)
    # one single brick, at negative cells and at the sensor
    for lo, hi in (((-4, -4, 0), (-1, -1, 3)), ((12, 0, 0), (12, 0, 0)), ((13, 1, 3), (14, 2, 3))):
        G, info = free_built(H, V, poses, clouds, lo=lo, hi=hi, **WALL)
        assert info["n_bricks"] == (1, 1, 1) and info["bytes"] == 8 and len(H.closed_map_free_words()) == 1
        same_reads(H, G, bands=((0.5, 2.9, 1),))
    assert info["free_cells"] > 0
    # a box no ray reaches
    G, info = free_built(H, V, poses, clouds, lo=(200, 200, 200), hi=(203, 207, 211), **WALL)
    assert (info["cells_marked"], info["cells_outside"], info["free_cells"], info["n_bricks"]) == (0, 98767, 0, (1, 2, 3))


# ---- 4: lifecycle ------------------------------------------------------------------------------------------------------------
def test_an_extend_then_add_keyframes(hip_module):
    reg = hip_module
    poses, clouds, _, _ = LS.wall()
    v = CS.GHOST["voxel"]
    A = context(reg, poses, clouds, keep=range(5), voxel=v, cloud_mask=CS.MASK)
    A.closed_map_build(2, poses[:5])
    A.closed_map_free_configure(**WALL)
    lo, hi = FN.auto_box(poses, v, (0.0, 0.0, 0.0), 12.0)                          # a box that holds all six
    first = A.closed_map_free_build(lo, hi)
    words5 = A.closed_map_free_words().tobytes()
    assert A.place_add_scan(TV.DUMMY, poses[5], 5) == 5
    A.place_set_keyframe_clouds(5, *clouds[5])
    A.closed_map_extend(2, poses[5:6])
    assert A.closed_map_free_info() == first and A.closed_map_free_words().tobytes() == words5   # an extend leaves the grid alone
    info = A.closed_map_free_add_keyframes()
    V = CN.build_map(poses, clouds, CS.MASK, v)
    G = FN.FreeNP(V, **WALL)
    G.reset(lo, hi)
    G.add_keyframes(poses[:5], clouds[:5], CS.MASK)
    G.add_keyframes(poses, clouds, CS.MASK)
    same_grid(A, G, info)
    assert info["keyframes"] == 6 and info["rays"] == len(CN.concatenation(clouds[5], CS.MASK))
    same_reads(A, G)                                                               # occupancy sees the extended map
    B, _ = built(reg, poses, clouds, CS.MASK, v)
    B.closed_map_free_configure(**WALL)
    whole = B.closed_map_free_build(lo, hi)
    assert B.closed_map_free_words().tobytes() == A.closed_map_free_words().tobytes()
    assert (whole["free_cells"], whole["bricks_nonzero"], whole["keyframes"]) == (info["free_cells"], info["bricks_nonzero"], 6)
    assert bits(B.closed_map_free_cells()) == bits(A.closed_map_free_cells())
    A.close(); B.close()


def test_free_space_changes_nothing_else_and_a_detached_map(hip_module):
    reg = hip_module
    poses, clouds, scan, pose, _ = DS.ghost_gate()
    H, T = TL.surfeled(reg, poses, clouds, CS.MASK, DS.VOXEL)
    V = CN.build_map(poses, clouds, CS.MASK, DS.VOXEL)
    cfg = dict(max_range=DS.MAX_RANGE)
    H.closed_map_carve_configure(**cfg)
    H.closed_map_carve()
    H.closed_map_diff_configure(**cfg)
    H.closed_map_diff(scan, pose)
    prior = LS.offset(pose, 0.1, 0.01)

    def everything(X):
        rows = X.closed_map_read()
        found = X.closed_map_localise(scan, prior)
        through, hits = X.closed_map_diff_counts()
        return (bits(rows[0]) + rows[1].tobytes(), X.closed_map_misses().tobytes(), TS.surfel_bytes(X), through.tobytes() + hits.tobytes(),
                bits(found[0]), {**found[1], "prepared": 0}, log_bytes(X.closed_map_localise_log()),
                {**X.closed_map_diff_info(), "prepared": 0, "launches": 0},
                X.closed_map_save(), X.closed_map_save(clouds=True))

    before = everything(H)
    G, _ = free_built(H, V, poses, clouds, carve_gate=1, **cfg)
    assert everything(H) == before
    M = H.closed_map_misses()
    scan_and_compare(H, G, scan, pose)
    same_reads(H, G, misses=M)
    H.closed_map_free_reset((0, 0, 0), (40, 20, 8))
    H.closed_map_free_add_keyframes()
    assert everything(H) == before
    # the other stages leave the grid: a carve, a surfel pass, a diff, a localise (inside everything)
    words, info = H.closed_map_free_words().tobytes(), H.closed_map_free_info()
    H.closed_map_carve(); H.closed_map_surfels(); H.closed_map_diff(scan, pose)
    assert everything(H) == before and H.closed_map_free_words().tobytes() == words and H.closed_map_free_info() == info
    # the detached map: saved without clouds, loaded into a fresh context
    D = reg.HipRegistration()
    D.closed_map_load(before[8])
    assert D.closed_map_free_info()["bytes"] == 0                                  # the snapshot holds no grid
    with not_ready(reg):
        D.closed_map_free_add_scan(scan, pose)                                     # no grid yet
    D.closed_map_free_configure(**cfg)
    G = fresh(D, V, poses, **cfg)
    with not_ready(reg):
        D.closed_map_free_add_keyframes()                                          # detached: no clouds to walk
    same_grid(D, G)
    info = scan_and_compare(D, G, scan, pose)
    assert info["scans"] == 1 and info["keyframes"] == 0 and info["free_cells"] > 100
    same_reads(D, G)
    assert D.closed_map_save() == before[8]
    # a load replaces the map: the grid goes
    H.closed_map_load(before[9])
    assert H.closed_map_free_info()["bytes"] == 0
    with not_ready(reg):
        H.closed_map_free_words()
    H.close(); D.close()


def test_refusals_and_lifecycle(hip_module):
    reg = hip_module
    poses, clouds, scan, truth = LS.wall()
    v = CS.GHOST["voxel"]
    H = context(reg, poses, clouds, voxel=v, cloud_mask=CS.MASK)
    zero = reg.FreeInfo().as_dict()
    assert H.closed_map_free_info() == zero
    with not_ready(reg):
        H.closed_map_free_reset()                                                  # no map
    H.closed_map_build(2, poses)
    for call in (H.closed_map_free_add_keyframes, lambda: H.closed_map_free_add_scan(scan, truth), H.closed_map_free_words,
                 lambda: H.closed_map_occupancy(scan), H.closed_map_free_cells, lambda: H.closed_map_free_columns(0.0, 1.0)):
        with not_ready(reg):
            call()                                                                 # no grid
    assert H.closed_map_free_info() == zero
    H.closed_map_free_configure(**WALL)
    info = H.closed_map_free_build()
    words = H.closed_map_free_words().tobytes()

    def untouched():
        return H.closed_map_free_words().tobytes() == words and H.closed_map_free_info() == info

    # refused resets leave the previous grid
    for lo, hi in (((1, 0, 0), (0, 0, 0)), ((0, 0, 5), (3, 3, 4)), ((-2 ** 20, 0, 0), (0, 0, 0)), ((0, 0, 0), (0, 2 ** 20, 0)),
                   ((-2 ** 40, 0, 0), (0, 0, 0)), ((-(2 ** 20 - 1),) * 3, (2 ** 20 - 1,) * 3)):       # the last: 2^60 bytes
        with invalid(reg):
            H.closed_map_free_reset(lo, hi)
    with pytest.raises(ValueError):
        H.closed_map_free_reset(lo_cells=(0, 0, 0))
    lp = C.POINTER(C.c_int64)
    three = np.zeros(3, np.int64)
    assert H.L.tloam_closed_map_free_reset(H.h, three.ctypes.data_as(lp), None) == -1
    assert H.L.tloam_closed_map_free_reset(H.h, None, three.ctypes.data_as(lp)) == -1
    assert untouched()
    # refused adds and reads change nothing
    flat = np.ascontiguousarray(scan).ctypes.data_as(C.POINTER(C.c_double))
    colp = np.ascontiguousarray(truth.T).reshape(-1).ctypes.data_as(C.POINTER(C.c_double))
    state = np.full(len(scan), 9, np.uint8)
    sp = state.ctypes.data_as(C.POINTER(C.c_uint8))
    assert H.L.tloam_closed_map_free_add_scan(H.h, None, len(scan), colp, None) == -1
    assert H.L.tloam_closed_map_free_add_scan(H.h, flat, len(scan), None, None) == -1
    assert H.L.tloam_closed_map_free_add_scan(H.h, flat, 0, colp, None) == -1
    assert H.L.tloam_closed_map_occupancy(H.h, None, len(scan), None, sp, None, None) == -1
    assert H.L.tloam_closed_map_occupancy(H.h, flat, len(scan), None, None, None, None) == -1
    assert H.L.tloam_closed_map_occupancy(H.h, flat, 0, None, sp, None, None) == -1
    shifted = truth.copy()
    shifted[0, 3] = np.inf
    for bad_pose in (2.0 * np.eye(4), np.full((4, 4), np.nan), np.diag([1.0, 1.0, -1.0, 1.0]), shifted):
        with invalid(reg):
            H.closed_map_free_add_scan(scan, bad_pose)
        with invalid(reg):
            H.closed_map_occupancy(scan, bad_pose)
    with invalid(reg):
        H.closed_map_free_add_scan(np.zeros((0, 3)), truth)
    for z_lo, z_hi, min_free in ((2.0, 1.0, 1), (np.nan, 1.0, 1), (0.0, np.inf, 1), (0.0, 1.0, 0), (0.0, 1.0, -3)):
        with invalid(reg):
            H.closed_map_free_columns(z_lo, z_hi, min_free)
    assert (state == 9).all() and untouched()
    # a short capacity writes nothing and reports the size, for the cells and the columns
    n = C.c_size_t(0)
    cen = np.full((875, 3), -7.0)
    cp = cen.ctypes.data_as(C.POINTER(C.c_double))
    assert H.L.tloam_closed_map_read_free(H.h, None, None, 874, C.byref(n), cp) == -1 and n.value == 875 and (cen == -7.0).all()
    assert H.L.tloam_closed_map_read_free(H.h, None, None, 875, C.byref(n), cp) == 0 and n.value == 875
    assert bits(cen) == bits(H.closed_map_free_cells())
    box = np.array([5.0, 0.0, 1.0, 7.0, 3.0, 2.0])
    cen[:] = -7.0
    rc = H.L.tloam_closed_map_read_free(H.h, box[:3].ctypes.data_as(C.POINTER(C.c_double)), box[3:].ctypes.data_as(C.POINTER(C.c_double)),
                                        875, C.byref(n), cp)
    m = n.value
    assert rc == 0 and 0 < m < 875 and bits(cen[:m]) == bits(H.closed_map_free_cells(box[:3], box[3:])) and (cen[m:] == -7.0).all()
    assert H.L.tloam_closed_map_read_free(H.h, box[:3].ctypes.data_as(C.POINTER(C.c_double)), None, 875, C.byref(n), cp) == -1
    with pytest.raises(ValueError):
        H.closed_map_free_cells(lo=(0.0, 0.0, 0.0))
    nx, ny = C.c_size_t(0), C.c_size_t(0)
    col = np.full(76 * 56, 9, np.uint8)
    up = col.ctypes.data_as(C.POINTER(C.c_uint8))
    assert H.L.tloam_closed_map_free_columns(H.h, 0.5, 2.9, 1, up, 76 * 56 - 1, C.byref(nx), C.byref(ny)) == -1
    assert (nx.value, ny.value) == (76, 56) and (col == 9).all()
    assert H.L.tloam_closed_map_free_columns(H.h, 0.5, 2.9, 1, up, 76 * 56, C.byref(nx), C.byref(ny)) == 0
    assert col.tobytes() == H.closed_map_free_columns(0.5, 2.9).tobytes() and untouched()
    # a word range beyond the grid
    nw = 19 * 14 * 14
    with invalid(reg):
        H.closed_map_free_words(nw, 1)
    assert len(H.closed_map_free_words(nw, 0)) == 0 and len(H.closed_map_free_words(nw - 1)) == 1
    # a refused configuration leaves the old one, and the grid
    for bad in (dict(max_range=0.0), dict(max_range=float("inf")), dict(max_range=float("nan")), dict(end_margin=-1.0),
                dict(end_margin=float("inf")), dict(end_margin=float("nan")), dict(ray_mask=-1), dict(ray_mask=0x100), dict(max_bytes=7),
                dict(max_bytes=-1), dict(min_count=0), dict(min_miss=-1), dict(miss_ratio=float("nan")), dict(carve_gate=2),
                dict(carve_gate=-1)):
        with invalid(reg):
            H.closed_map_free_configure(**bad)
    with pytest.raises(KeyError):
        H.closed_map_free_configure(radius=1.0)
    assert untouched() and H.closed_map_free_build() == info and untouched()       # (still max_range 12)
    # a reset over max_bytes is refused; one that just fits is not
    H.closed_map_free_configure(max_bytes=8 * nw - 1, **WALL)                      # (a configure drops the grid)
    assert H.closed_map_free_info() == zero
    with invalid(reg):
        H.closed_map_free_reset()
    assert H.closed_map_free_info() == zero
    assert H.closed_map_free_reset((0, 0, 0), (3, 3, 3))["bytes"] == 8
    H.closed_map_free_configure(max_bytes=8 * nw, **WALL)
    assert H.closed_map_free_build() == info and untouched()
    # a build drops the grid; the configuration persists across a reset of the odometry
    H.closed_map_build(2, poses)
    assert H.closed_map_free_info() == zero
    with not_ready(reg):
        H.closed_map_free_add_keyframes()
    assert H.closed_map_free_build() == info
    H.odometry_reset(None, TS.TC.odom_cfg(reg))
    assert H.closed_map_free_info() == zero
    for k in range(len(poses)):
        assert H.place_add_scan(TS.DUMMY, np.eye(4), k) == k
        H.place_set_keyframe_clouds(k, *clouds[k])
    H.closed_map_build(2, poses)
    assert H.closed_map_free_build() == info and untouched()                       # max_range 12 and max_bytes are still there
    # a map without keyframes: the auto box is the cell 0
    E = reg.HipRegistration()
    E.place_configure(enabled=1, exclude_recent=8)
    E.loop_configure(enabled=1)
    assert E.closed_map_build(0)["n_voxels"] == 0
    empty = E.closed_map_free_build()
    assert (empty["lo_cells"], empty["n_bricks"], empty["rays"], empty["free_cells"]) == ((0, 0, 0), (1, 1, 1), 0, 0)
    got = E.closed_map_free_add_scan(scan[:300], truth)
    assert got["rays"] == 300 and got["cells_marked"] + got["cells_outside"] > 0
    assert (E.closed_map_occupancy(scan[:300], truth)[0] == reg.OCCUPANCY_UNKNOWN).all() and len(E.closed_map_free_cells()) == got["free_cells"]
    E.close(); H.close()
    # nranks > 1: every call is refused
    H = reg.HipRegistration()
    H.comm_init_callback(0, 2, lambda dev, count, stream: 0)
    for call in (H.closed_map_free_configure, H.closed_map_free_info, H.closed_map_free_reset, H.closed_map_free_add_keyframes,
                 lambda: H.closed_map_free_add_scan(scan, truth), lambda: H.closed_map_free_words(0, 0),
                 lambda: H.closed_map_occupancy(scan), H.closed_map_free_cells):
        with invalid(reg):
            call()
    n = C.c_size_t(0)
    assert H.L.tloam_closed_map_free_columns(H.h, 0.0, 1.0, 1, None, 0, C.byref(n), C.byref(n)) == -1
    H.close()
