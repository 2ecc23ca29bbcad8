"""-m gpu: the ray-cast of the closed map (tl_raycast.hip, tl_api_raycast.hip) against its numpy restatement
(tests/closed_map_raycast_np.py): status, range, id and every counter bit for bit.  Keyframes are hand-made as in
tests/test_gpu_closed_map_surfel.py; the scenes are tests/raycast_scenes.py's, tests/diff_scenes.py's and
tests/localise_scenes.py's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_carve_np as CN  # noqa: E402
import closed_map_raycast_np as RN  # noqa: E402
import diff_scenes as DS  # noqa: E402
import localise_scenes as LS  # noqa: E402
import raycast_scenes as RS  # noqa: E402
import test_gpu_closed_map_diff as TD  # noqa: E402
import test_gpu_closed_map_localise as TL  # noqa: E402
import test_gpu_closed_map_surfel as TS  # noqa: E402
from tloam_amd import raycast as RC  # noqa: E402

pytestmark = pytest.mark.gpu

bits, invalid, not_ready, surfeled, context, log_bytes = TL.bits, TL.invalid, TL.not_ready, TL.surfeled, TL.context, TL.log_bytes
surfeled_with_map, counts_bytes = TD.surfeled_with_map, TD.counts_bytes
Rz90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
SAME = dict(prepared=0, launches=0)


def check_cast(H, T, V, ends, pose, cfg=None, misses=None):
    """one cast on the device (configured for `cfg` by the caller) and in the restatement -> (info, the restatement's result)"""
    status, ranges, ids, info = H.closed_map_raycast(ends, pose, want_ids=True)
    want = RN.cast(T, V, ends, pose, cfg, misses)
    print(f"n {len(ends)} {cfg}: {info}")
    assert status.dtype == np.uint8 and status.tobytes() == want["status"].tobytes()
    assert ranges.dtype == np.float64 and ranges.tobytes() == want["ranges"].tobytes()
    assert ids.dtype == np.int32 and ids.tobytes() == want["ids"].tobytes()
    assert {k: info[k] for k in want["info"]} == want["info"]
    assert H.closed_map_raycast_info() == info and info["launches"] == 1 + info["prepared"]
    return info, want


# ---- the scenes, built once --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wall(hip_module):
    poses, clouds, _, _ = LS.wall()
    H, T, V = surfeled_with_map(hip_module, poses, clouds, CS.MASK, DS.VOXEL)
    yield H, T, V
    H.close()


@pytest.fixture(scope="module")
def static(hip_module):
    poses, clouds = CS.static_pass()
    _, truth = LS.static_scan(poses)
    H, T, V = surfeled_with_map(hip_module, poses, clouds, CS.MASK, CS.STATIC["voxel"])
    yield H, T, V, RC.lidar_pattern(16, 180, -0.3, 0.3, 30.0), truth
    H.close()


# ---- 1: the wall, the ghost gate, the static pass, the block boundaries --------------------------------------------------------
@pytest.mark.parametrize("k", range(3))
def test_the_wall(wall, k):
    H, T, V = wall
    ends, pose = RS.pattern(), DS.pose_at(DS.SENSORS[k])
    t, on, off = RS.wall_ranges(DS.SENSORS[k])
    for planes in (0, 1, 2):
        for radius_cells in (0.5, 0.75, 1.0):
            cfg = dict(planes=planes, radius_cells=radius_cells)
            H.closed_map_raycast_configure(**cfg)
            info, want = check_cast(H, T, V, ends, pose, cfg)
            hit = want["status"] >= RN.HIT_CENTROID
            assert not (off & hit).any() and (radius_cells < 1.0 or hit[on].all())
            assert (info["hits_centroid"] == 0) == (planes == 2) and (info["hits_plane"] == 0) == (planes == 0)
    if k == 0:
        assert (info["steps"], info["tested"]) == (83737, 617)   # planes 2, radius_cells 1.0


def test_the_ghost_gate(hip_module):
    poses, clouds, _, pose, _ = DS.ghost_gate()
    H, T, V = surfeled_with_map(hip_module, poses, clouds, CS.MASK, DS.VOXEL)
    H.closed_map_carve_configure(max_range=DS.MAX_RANGE)
    H.closed_map_carve()
    M, _ = CN.carve(V, poses, clouds, CS.MASK, max_range=DS.MAX_RANGE)
    assert H.closed_map_misses().tobytes() == M.tobytes()
    box = DS.box_voxels(V)
    aim = V.centroids()[box] - pose[:3, 3]
    r = np.linalg.norm(aim, axis=1)
    ends = np.concatenate([aim * ((r + 6.0) / r)[:, None], RS.pattern()])
    for planes in (0, 1):
        H.closed_map_raycast_configure(planes=planes)
        off = check_cast(H, T, V, ends, pose, dict(planes=planes))[1]
        H.closed_map_raycast_configure(planes=planes, carve_gate=1)
        on = check_cast(H, T, V, ends, pose, dict(planes=planes, carve_gate=1), misses=M)[1]
        assert np.isin(off["ids"][:8], box).all() and not np.isin(on["ids"], box).any() and (on["ids"][:8] >= 0).all()
    # another rule of the gate, and min_count beside it
    cfg = dict(carve_gate=1, min_miss=125, miss_ratio=0.5, min_count=9)
    H.closed_map_raycast_configure(**cfg)
    some = check_cast(H, T, V, ends, pose, cfg, misses=M)[1]
    assert not np.isin(some["ids"], box).any()                   # (the box's voxels hold 8 points each)
    cfg = dict(carve_gate=1, min_miss=125, miss_ratio=0.5)
    H.closed_map_raycast_configure(**cfg)
    some = check_cast(H, T, V, ends, pose, cfg, misses=M)[1]
    assert 0 < np.isin(some["ids"][:8], box).sum() < 8
    H.close()


def test_the_static_pass(static):
    H, T, V, ends, truth = static
    for cfg in (dict(), dict(planes=2), dict(planes=0, radius_cells=1.0, min_count=3)):
        H.closed_map_raycast_configure(**cfg)
        info, _ = check_cast(H, T, V, ends, truth, cfg)
        assert info["hits_plane"] + info["hits_centroid"] > 1000 and info["skipped"] == 0
        check_cast(H, T, V, ends, LS.offset(truth, 0.3, 0.02), cfg)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_block_boundaries(static, n):
    H, T, V, ends, truth = static
    H.closed_map_raycast_configure()
    info, _ = check_cast(H, T, V, ends[700:700 + n], LS.offset(truth, 0.1, 0.01))
    assert info["rays"] == n


# ---- 2: the hand-made rays, the adversarial grid, the map without voxels -----------------------------------------------------------
HAND_ORIGIN = (0.0, -0.25, 0.0)        # the wall y = 5 in the middle of its cells [4.75, 5.25)
OUTSIDE = np.array([6.25, 0.0, 1.25])  # a dyadic cell centre of that grid, 5 m in front of the wall
INSIDE = np.array([6.25, 5.125, 1.25])  # inside a wall voxel, behind its plane; its centroid is near (6.2, 5.0, 1.2)


def hand_made_rays(t, inside):
    """world ends of rays from the sensor at t that hold every special case of the contract"""
    if inside:
        return np.array([
            t + [-0.03125, -0.1875, -0.03125],   # 0: inside one occupied cell, across its plane: the end cell is the only cell
            t + [0.0, 0.0625, 0.0],              # 1: inside that cell, away from the plane (tp < 0)
            t + [0.0, 3.0, 0.0],                 # 2: out of the voxel, its centroid behind the sensor
            t + [3.0, 0.0, 0.0], t + [0.0, 0.0, 1.5], t + [-2.0, 0.0, -0.5],   # 3-5: parallel to the plane (den == 0)
            t + [0.0, -2.0, 0.0],                # 6: out through the plane
        ])
    return np.array([
        [np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [-np.inf, np.nan, 0.0],            # 0-2: not finite
        [2.0 ** 19 + 5.0, 0.0, 0.0], [0.0, -(2.0 ** 19) - 5.0, 1.0],                # 3-4: beyond the grid at v = 0.5
        t,                                                                          # 5: zero length
        t + [0.0, 30.0, 0.0],                                                       # 6: longer than max_range = 12
        t + [0.125, 0.0625, -0.125],                                                # 7: inside the sensor's (empty) cell
        t + [0.0, 4.875, 0.0],                                                      # 8: ends in the wall's cell short of the plane
        t + [0.0, 5.0078125, 0.0],                                                  # 9: ... and just past it
        t + [4.0, 0.0, 0.0], t + [0.0, 5.5, 0.0], t + [0.0, 0.0, -1.0], t + [-3.0, 0.0, 0.0],   # 10-13: axis-parallel
        t + [2.0, 2.0, 0.0], t + [-1.5, 1.5, 0.0], t + [0.0, 2.5, 2.5],             # 14-16: tMax ties on two axes
        t + [5.5, 5.5, 0.0],                                                        # 17: ... all the way into the wall
        t + [2.0, 2.0, 2.0], t + [-1.0, 1.0, -1.0], t + [1.5, 4.5, 1.5],            # 18-20: ties on three (20: not a diagonal)
        t + [5.5, 5.5, 1.375],                                                      # 21: a general ray onto the wall
    ])


def sensor_frame(world, R, t):
    with np.errstate(invalid="ignore"):
        return np.ascontiguousarray((world - t) @ R)


def test_the_hand_made_rays(hip_module):
    reg = hip_module
    poses, clouds, _, _ = LS.wall()
    H, T, V = surfeled_with_map(reg, poses, clouds, CS.MASK, DS.VOXEL, HAND_ORIGIN)
    o = np.asarray(HAND_ORIGIN)
    for planes in (1, 2, 0):
        cfg = dict(planes=planes, max_range=12.0)
        H.closed_map_raycast_configure(**cfg)
        for R in (np.eye(3), Rz90, LS.rotation([0.2, -0.3, 0.9], 0.4)):
            for t, inside in ((OUTSIDE, False), (INSIDE, True)):
                pose = np.eye(4)
                pose[:3, :3], pose[:3, 3] = R, t
                world = hand_made_rays(t, inside)
                info, want = check_cast(H, T, V, sensor_frame(world, R, t), pose, cfg)
                s = list(want["status"])
                if abs(R).sum() != 3.0:
                    continue                                                    # a rotation that rounds: bit for bit, no more
                E = CN.transform(pose, sensor_frame(world, R, t))
                if inside:
                    assert np.array_equal(E, world)                             # the pose gives the world points back exactly
                    assert CN.Walk((t - o) / DS.VOXEL, (E[:2] - o) / DS.VOXEL).n.tolist() == [0, 0]
                    assert T.find(np.floor((t - o) / DS.VOXEL).astype(np.int64)[None])[0] >= 0   # the sensor's cell is a voxel
                    assert s[0] == (reg.RAYCAST_HIT_PLANE if planes else reg.RAYCAST_HIT_CENTROID) and s[1] == s[2] == reg.RAYCAST_MISS
                    # den == 0: the centroid test under planes 1, passed through under planes 2
                    assert s[3:6] == [reg.RAYCAST_MISS if planes == 2 else reg.RAYCAST_HIT_CENTROID] * 3
                    assert s[6] == (reg.RAYCAST_HIT_PLANE if planes else reg.RAYCAST_HIT_CENTROID)
                    assert want["ranges"][0] > 0.0 and info["skipped"] == 0
                else:
                    assert np.array_equal(E[5:], world[5:])
                    walk = CN.Walk(np.tile((t - o) / DS.VOXEL, (len(E) - 7, 1)), (E[7:] - o) / DS.VOXEL)
                    tie = (walk.tmax == walk.tmax.min(axis=1, keepdims=True)).sum(axis=1)
                    assert walk.n[0] == 0 and (tie[7:11] == 2).all() and (tie[11:13] == 3).all()   # (the ties are there from the first step)
                    assert ((walk.step[3:7] != 0).sum(axis=1) == 1).all()                          # d == 0 on two axes
                    assert s[:7] == [reg.RAYCAST_SKIPPED] * 7 and info["skipped"] == 7 and s[7] == s[8] == reg.RAYCAST_MISS
                    front = reg.RAYCAST_HIT_PLANE if planes else reg.RAYCAST_HIT_CENTROID
                    assert s[9] == s[11] == s[17] == s[21] == front
                    assert [s[k] for k in (10, 12, 13, 14, 15, 16, 18, 19, 20)] == [reg.RAYCAST_MISS] * 9
                    if planes:
                        assert abs(want["ranges"][9] - 5.0) < 1e-9 and abs(want["ranges"][11] - 5.0) < 1e-9
    # the grid's limit by itself: within max_range, beyond the grid
    cfg = dict(max_range=1e7)
    H.closed_map_raycast_configure(**cfg)
    pose = DS.pose_at(OUTSIDE)
    info, want = check_cast(H, T, V, hand_made_rays(OUTSIDE, False)[3:5] - OUTSIDE, pose, cfg)
    assert info["skipped"] == 2
    H.close()


@pytest.mark.parametrize("voxel,origin", [(1.0, (1.0, -2.0, 0.5)), (0.3, (-0.37, 12.5, 0.11))])
def test_the_adversarial_grid(hip_module, voxel, origin):
    """section 22's map: negative cells, a non-zero origin and q = 2^24, the localiser's gate opened to every solved voxel; the
    rays run from the middle of the map to its own centroids, past them, and between them"""
    poses, clouds = TS.adversarial_plus(voxel, origin)
    H, T, V = surfeled_with_map(hip_module, poses, clouds, 0xFF, voxel, origin, min_points=3, min_planarity=-1.0)
    assert (T.c < 0.0).any() and T.eligible.sum() >= 15
    pose = LS.offset(np.eye(4), 0.05 * voxel, 1e-4)
    pose[:3, 3] += np.median(T.c, axis=0)
    world = np.concatenate([T.c, 0.5 * (T.c[:-1] + T.c[1:]), T.c + 0.3 * voxel, 2.0 * T.c - pose[:3, 3]])
    ends = (world - pose[:3, 3]) @ pose[:3, :3]
    for cfg in (dict(max_range=1e4), dict(max_range=1e4, planes=0, radius_cells=2.0), dict(max_range=1e4, planes=2, min_count=2)):
        H.closed_map_raycast_configure(**cfg)
        info, _ = check_cast(H, T, V, ends, pose, cfg)
        assert info["tested"] > 0 and info["hits_centroid"] + info["hits_plane"] > 0
    H.close()


def test_a_map_without_voxels(hip_module):
    """a built map's slot table is there when the map holds nothing: every probe finds a free slot"""
    reg = hip_module
    H = reg.HipRegistration()
    H.place_configure(enabled=1, exclude_recent=8)
    H.loop_configure(enabled=1)
    assert H.closed_map_build(0)["n_voxels"] == 0          # no keyframes: an empty map, built
    H.closed_map_surfels()
    status, ranges, ids, info = H.closed_map_raycast(RS.pattern()[:300], DS.pose_at(DS.SENSORS[0]), want_ids=True)
    assert (status == reg.RAYCAST_MISS).all() and (ranges == -1.0).all() and (ids == -1).all()
    assert (info["missed"], info["tested"], info["skipped"], info["hits_centroid"], info["hits_plane"]) == (300, 0, 0, 0, 0)
    assert info["steps"] > 300
    H.close()


# ---- 3: determinism, the shared records, non-interference, the detached map --------------------------------------------------------
def test_calls_and_contexts_give_the_same_bytes(static, hip_module):
    H, T, V, ends, truth = static
    H.closed_map_raycast_configure()
    pose = LS.offset(truth, 0.3, 0.02)
    a = H.closed_map_raycast(ends, pose, want_ids=True)
    b = H.closed_map_raycast(ends, pose, want_ids=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and {**a[3], **SAME} == {**b[3], **SAME}
    c = H.closed_map_raycast(ends, pose)                      # want_ids=False: no ids, the same status and ranges
    assert c[2] is None and c[0].tobytes() == a[0].tobytes() and c[1].tobytes() == a[1].tobytes() and c[3] == b[3]
    poses, clouds = CS.static_pass()
    other, _ = surfeled(hip_module, poses, clouds, CS.MASK, CS.STATIC["voxel"], reserve_voxels=64)
    d = other.closed_map_raycast(ends, pose, want_ids=True)
    assert d[3]["prepared"] == 1 and d[3]["launches"] == 2 and {**d[3], **SAME} == {**a[3], **SAME}
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], d[:3]))
    other.close()


def test_the_records_are_shared_with_the_localiser_and_the_diff(hip_module):
    poses, clouds, scan, truth = LS.wall()
    H, T, V = surfeled_with_map(hip_module, poses, clouds, CS.MASK, DS.VOXEL)
    ends, pose = RS.pattern(), DS.pose_at(DS.SENSORS[0])
    first = H.closed_map_raycast(ends, pose)[3]
    assert (first["prepared"], first["launches"]) == (1, 2)
    assert H.closed_map_localise(scan, truth)[1]["prepared"] == 0 and H.closed_map_diff(scan, truth)[2]["prepared"] == 0
    again = H.closed_map_raycast(ends, pose)[3]
    assert (again["prepared"], again["launches"]) == (0, 1) and {**again, **SAME} == {**first, **SAME}
    # the localiser's gate makes the records stale for all three; whichever runs first rebuilds them
    H.closed_map_localise_configure(min_planarity=0.5)
    assert H.closed_map_raycast(ends, pose)[3]["prepared"] == 1 and H.closed_map_localise(scan, truth)[1]["prepared"] == 0
    H.closed_map_localise_configure(min_planarity=0.05)
    assert H.closed_map_diff(scan, truth)[2]["prepared"] == 1
    last = check_cast(H, T, V, ends, pose)[0]
    assert last == again
    H.close()


def test_a_cast_changes_nothing_else_and_a_detached_map_casts_alike(hip_module):
    reg = hip_module
    poses, clouds, scan, pose, _ = DS.ghost_gate()
    H, T, V = surfeled_with_map(reg, poses, clouds, CS.MASK, DS.VOXEL)
    H.closed_map_carve_configure(max_range=DS.MAX_RANGE)
    H.closed_map_carve()
    prior = LS.offset(pose, 0.1, 0.01)
    H.closed_map_diff_configure(max_range=DS.MAX_RANGE)
    H.closed_map_diff(scan, pose)
    ends = RS.pattern()

    def everything(X):
        rows = X.closed_map_read()
        found = X.closed_map_localise(scan, prior)
        return (bits(rows[0]) + rows[1].tobytes(), X.closed_map_misses().tobytes(), TS.surfel_bytes(X), counts_bytes(X),
                X.closed_map_diff_info(), bits(found[0]), {**found[1], "prepared": 0}, log_bytes(X.closed_map_localise_log()),
                X.closed_map_save(), X.closed_map_save(clouds=True))

    before = everything(H)
    H.closed_map_raycast_configure(carve_gate=1)
    mine = H.closed_map_raycast(ends, pose, want_ids=True)
    H.closed_map_raycast(ends[:100], prior)
    assert everything(H) == before
    mine = H.closed_map_raycast(ends, pose, want_ids=True)
    # the detached map: saved without clouds, loaded into a fresh context, cast there
    F = reg.HipRegistration()
    F.closed_map_load(before[8])
    assert F.closed_map_raycast_info()["rays"] == 0
    F.closed_map_raycast_configure(carve_gate=1)
    theirs = F.closed_map_raycast(ends, pose, want_ids=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(mine[:3], theirs[:3])) and {**theirs[3], **SAME} == {**mine[3], **SAME}
    assert F.closed_map_save() == before[8]
    # a load replaces the map: the last info goes
    H.closed_map_load(before[9])
    assert H.closed_map_raycast_info() == {k: 0 for k in mine[3]}
    H.close(); F.close()


# ---- 4: refusals and lifecycle -------------------------------------------------------------------------------------------------
def test_refusals_and_lifecycle(hip_module):
    reg = hip_module
    poses, clouds, _, _ = LS.wall()
    ends, pose = RS.pattern()[1260:1760], DS.pose_at(DS.SENSORS[1])   # rings 7 to 9: level rays
    H = context(reg, poses, clouds, voxel=DS.VOXEL, cloud_mask=CS.MASK)
    with not_ready(reg):
        H.closed_map_raycast(ends, pose)                             # no map
    H.closed_map_build(2, poses)
    with not_ready(reg):
        H.closed_map_raycast(ends, pose)                             # no surfels
    H.closed_map_surfels()
    status, ranges, ids, info = H.closed_map_raycast(ends, pose, want_ids=True)
    assert info["prepared"] == 1 and info["launches"] == 2 and info["rays"] == 500

    n = len(ends)
    st, rg, ix = np.full(n, 77, np.uint8), np.full(n, -7.0), np.full(n, -7, np.int32)
    flat, col = np.ascontiguousarray(ends), np.ascontiguousarray(pose.T).reshape(-1)
    dp = C.POINTER(C.c_double)
    fp, cp, sp, rp, ip = (flat.ctypes.data_as(dp), col.ctypes.data_as(dp), st.ctypes.data_as(C.POINTER(C.c_uint8)),
                          rg.ctypes.data_as(dp), ix.ctypes.data_as(C.POINTER(C.c_int32)))

    def untouched():
        return (st == 77).all() and (rg == -7.0).all() and (ix == -7).all() and H.closed_map_raycast_info() == info

    call = H.L.tloam_closed_map_raycast
    assert call(H.h, None, n, cp, sp, rp, ip, None) == -1
    assert call(H.h, fp, n, None, sp, rp, ip, None) == -1
    assert call(H.h, fp, n, cp, None, rp, ip, None) == -1
    assert call(H.h, fp, n, cp, sp, None, ip, None) == -1
    assert call(H.h, fp, 0, cp, sp, rp, ip, None) == -1              # n == 0
    assert untouched()
    for bad_pose in (2.0 * np.eye(4), np.full((4, 4), np.nan), np.diag([1.0, 1.0, -1.0, 1.0])):
        bad = np.ascontiguousarray(bad_pose.T).reshape(-1)
        assert call(H.h, fp, n, bad.ctypes.data_as(dp), sp, rp, ip, None) == -1
    shifted = pose.copy()
    shifted[0, 3] = np.inf
    with invalid(reg):
        H.closed_map_raycast(ends, shifted)
    assert untouched()
    for bad in (dict(max_range=0.0), dict(max_range=float("inf")), dict(max_range=float("nan")), dict(radius_cells=0.0),
                dict(radius_cells=2.5), dict(radius_cells=float("nan")), dict(radius_cells=float("inf")), dict(planes=3),
                dict(planes=-1), dict(min_count=0), dict(min_miss=-1), dict(miss_ratio=float("nan")), dict(carve_gate=2),
                dict(carve_gate=-1)):
        with invalid(reg):
            H.closed_map_raycast_configure(**bad)
    with pytest.raises(KeyError):
        H.closed_map_raycast_configure(end_margin=1.0)
    assert untouched()                                              # the old configuration stays, and the info with it
    # ids NULL: status and ranges alone, and the ids' buffer is not written
    assert call(H.h, fp, n, cp, sp, rp, None, None) == 0
    assert st.tobytes() == status.tobytes() and rg.tobytes() == ranges.tobytes() and (ix == -7).all()
    assert H.closed_map_raycast_info() == {**info, "prepared": 0, "launches": 1}
    assert call(H.h, fp, n, cp, sp, rp, ip, None) == 0 and ix.tobytes() == ids.tobytes()
    info = H.closed_map_raycast_info()
    st[:], rg[:], ix[:] = 77, -7.0, -7
    # the surfels dropped: refused
    H.closed_map_surfel_configure(min_points=6)
    assert call(H.h, fp, n, cp, sp, rp, ip, None) == -6 and untouched()
    H.closed_map_surfel_configure()
    H.closed_map_surfels()
    # the gate on a map that is not carved
    H.closed_map_raycast_configure(carve_gate=1)                     # (a configure clears the info)
    assert H.closed_map_raycast_info()["rays"] == 0
    assert call(H.h, fp, n, cp, sp, rp, ip, None) == -6 and (st == 77).all() and (rg == -7.0).all() and (ix == -7).all()
    H.closed_map_carve_configure(max_range=DS.MAX_RANGE)
    H.closed_map_carve()
    got = H.closed_map_raycast(ends, pose, want_ids=True)
    assert got[0].tobytes() == status.tobytes() and got[2].tobytes() == ids.tobytes()   # the wall's voxels are not seen through
    # what empties the map clears the info; the configuration persists across a reset
    H.closed_map_raycast_configure(max_range=11.5, radius_cells=1.5, planes=0)
    H.closed_map_raycast(ends, pose)
    H.closed_map_build(2, poses)
    assert H.closed_map_raycast_info()["rays"] == 0
    H.odometry_reset(None, TS.TC.odom_cfg(reg))
    for k in range(len(poses)):
        assert H.place_add_scan(TS.DUMMY, np.eye(4), k) == k
        H.place_set_keyframe_clouds(k, *clouds[k])
    H.closed_map_build(2, poses)
    H.closed_map_surfels()
    T, V = LS.target(poses, clouds, CS.MASK, DS.VOXEL)[4], CN.build_map(poses, clouds, CS.MASK, DS.VOXEL)
    info, _ = check_cast(H, T, V, ends, pose, dict(max_range=11.5, radius_cells=1.5, planes=0))
    assert info["hits_plane"] == 0 and info["hits_centroid"] > 0
    H.close()
    # nranks > 1: every ray-cast call is refused
    H = reg.HipRegistration()
    H.comm_init_callback(0, 2, lambda dev, count, stream: 0)
    for refused in (H.closed_map_raycast_configure, lambda: H.closed_map_raycast(ends, pose), H.closed_map_raycast_info):
        with invalid(reg):
            refused()
    H.close()
