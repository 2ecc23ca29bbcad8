"""-m gpu: a scan diffed against the closed map (tl_diff.hip, tl_api_diff.hip) against its numpy
restatement (tests/closed_map_diff_np.py): labels, ids, through, hits and every counter bit for bit.  Keyframes are hand-made as
in tests/test_gpu_closed_map_surfel.py; the scenes are tests/diff_scenes.py's."""
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
import test_gpu_closed_map_localise as TL  # noqa: E402
import test_gpu_closed_map_surfel as TS  # noqa: E402

pytestmark = pytest.mark.gpu

bits, invalid, not_ready, surfeled, context, log_bytes = TL.bits, TL.invalid, TL.not_ready, TL.surfeled, TL.context, TL.log_bytes
RANGE = dict(max_range=DS.MAX_RANGE)
Rz90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def surfeled_with_map(reg, poses, clouds, mask, voxel, origin=(0.0, 0.0, 0.0), **kw):
    """TL.surfeled, and the restated map beside the restated target"""
    H, T = surfeled(reg, poses, clouds, mask, voxel, origin, **kw)
    return H, T, CN.build_map(poses, clouds, mask, voxel, origin)


def counts_bytes(H):
    through, hits = H.closed_map_diff_counts()
    return through.tobytes() + hits.tobytes()


def check_diff(H, T, V, pts, pose, cfg=None, misses=None, accumulate=False, state=None):
    """one diff on the device (configured for `cfg` by the caller) and in the restatement -> (info, the restatement's result)"""
    labels, ids, info = H.closed_map_diff(pts, pose, accumulate=accumulate, want_ids=True)
    want = DN.diff(T, V, pts, pose, cfg, misses, state)
    print(f"n {len(pts)} {cfg}: {info}")
    assert labels.dtype == np.uint8 and labels.tobytes() == want["labels"].tobytes()
    assert ids.dtype == np.int32 and ids.tobytes() == want["ids"].tobytes()
    through, hits = H.closed_map_diff_counts()
    assert through.tobytes() == want["through"].tobytes() and hits.tobytes() == want["hits"].tobytes()
    assert {k: info[k] for k in want["info"]} == want["info"]
    assert H.closed_map_diff_info() == info
    assert info["cleared"] == (0 if accumulate else 1) and info["launches"] == 3 + info["cleared"] + info["prepared"]
    if len(through) >= 3:
        part = H.closed_map_diff_counts(1, 2)
        assert part[0].tobytes() == want["through"][1:3].tobytes() and part[1].tobytes() == want["hits"][1:3].tobytes()
    return info, want


def check_gone(H, V, want, **read):
    cen, cnt, through, hits = H.closed_map_read_gone(**read)
    ids = DN.read_gone(V, want["through"], want["hits"], **read)
    assert bits(cen) == bits(V.centroids()[ids]) and cnt.tobytes() == V.N[ids].tobytes()
    assert through.tobytes() == want["through"][ids].tobytes() and hits.tobytes() == want["hits"][ids].tobytes()
    return ids


# ---- the scenes, built once --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gone(hip_module):
    poses, clouds, _, _ = DS.gone()
    H, T, V = surfeled_with_map(hip_module, poses, clouds, CS.MASK, DS.VOXEL)
    H.closed_map_diff_configure(**RANGE)
    yield H, T, V, (poses, clouds)
    H.close()


@pytest.fixture(scope="module")
def static(hip_module):
    poses, clouds = CS.static_pass()
    scan, truth = LS.static_scan(poses)
    H, T, V = surfeled_with_map(hip_module, poses, clouds, CS.MASK, CS.STATIC["voxel"])
    yield H, T, V, scan, truth
    H.close()


# ---- 1: the three scenes, the corner, the static pass ------------------------------------------------------------------------
def test_the_gone_scene_and_read_gone(gone, hip_module):
    H, T, V, _ = gone
    box = DS.box_voxels(V)
    for sensor in DS.SENSORS:
        _, _, scan, pose = DS.gone(sensor)
        info, want = check_diff(H, T, V, scan, pose, RANGE)
        assert np.array_equal(check_gone(H, V, want), box) and len(box) == 27          # the wrapper's defaults: exactly the box
        assert np.array_equal(check_gone(H, V, want, lo=DS.BOX_LO, hi=DS.BOX_HI), box)
        assert len(check_gone(H, V, want, lo=(0.0, 4.0, 0.0), hi=(12.0, 6.0, 4.0))) == 0
        assert len(check_gone(H, V, want, min_through=10, gone_ratio=0.0)) < 27
        assert len(check_gone(H, V, want, min_through=0, gone_ratio=-1.0)) == len(V.keys)   # every voxel: hits > 0 or through > 0
    # a short capacity returns the count needed and writes nothing, in any of the four columns
    import ctypes as C
    n = C.c_size_t(0)
    cen, cnt, thr, hit = np.full((27, 3), -7.0), np.full(27, -7, np.int64), np.full(27, -7, np.int64), np.full(27, -7, np.int64)
    lp = C.POINTER(C.c_int64)
    args = (cen.ctypes.data_as(C.POINTER(C.c_double)), cnt.ctypes.data_as(lp), thr.ctypes.data_as(lp), hit.ctypes.data_as(lp))
    rc = H.L.tloam_closed_map_read_gone(H.h, None, None, 3, 1.0, 5, C.byref(n), *args)
    assert rc == -1 and n.value == 27 and (cen == -7.0).all() and (cnt == -7).all() and (thr == -7).all() and (hit == -7).all()
    # ... and a capacity that holds them fills exactly the first n of each
    rc = H.L.tloam_closed_map_read_gone(H.h, None, None, 10, 0.0, 27, C.byref(n), *args)
    m = n.value
    ids = DN.read_gone(V, want["through"], want["hits"], min_through=10, gone_ratio=0.0)
    assert rc == 0 and 0 < m == len(ids) < 27 and thr[:m].tobytes() == want["through"][ids].tobytes()
    assert hit[:m].tobytes() == want["hits"][ids].tobytes() and cnt[:m].tobytes() == V.N[ids].tobytes()
    assert (cen[m:] == -7.0).all() and (cnt[m:] == -7).all() and (thr[m:] == -7).all() and (hit[m:] == -7).all()
    with pytest.raises(ValueError):
        H.closed_map_read_gone(lo=(0.0, 0.0, 0.0))


def test_the_appeared_scene(hip_module):
    poses, clouds, scan, pose, is_box = DS.appeared()
    H, T, V = surfeled_with_map(hip_module, poses, clouds, CS.MASK, DS.VOXEL)
    H.closed_map_diff_configure(**RANGE)
    info, want = check_diff(H, T, V, scan, pose, RANGE)
    labels = H.closed_map_diff(scan, pose)[0]
    assert (labels[is_box] == hip_module.DIFF_NEW).all() and (labels[~is_box] == hip_module.DIFF_SURFACE).all()
    assert len(check_gone(H, V, want)) == 0 and info["n_new"] == int(is_box.sum())
    assert H.closed_map_diff(scan, pose)[1] is None
    H.close()


def test_the_ghost_gate_scene(hip_module):
    reg = hip_module
    poses, clouds, scan, pose, is_box = DS.ghost_gate()
    H, T, V = surfeled_with_map(reg, poses, clouds, CS.MASK, DS.VOXEL)
    H.closed_map_carve_configure(**RANGE)
    H.closed_map_carve()
    M, _ = CN.carve(V, poses, clouds, CS.MASK, **RANGE)
    assert H.closed_map_misses().tobytes() == M.tobytes()
    H.closed_map_diff_configure(**RANGE)
    off = check_diff(H, T, V, scan, pose, RANGE)[1]
    H.closed_map_diff_configure(carve_gate=1, **RANGE)
    on = check_diff(H, T, V, scan, pose, dict(RANGE, carve_gate=1), misses=M)[1]
    assert (off["labels"][is_box] == reg.DIFF_OCCUPIED).all() and (on["labels"][is_box] == reg.DIFF_NEW).all()
    assert (off["labels"][~is_box] == reg.DIFF_SURFACE).all() and (on["labels"][~is_box] == reg.DIFF_SURFACE).all()
    # another rule of the gate
    H.closed_map_diff_configure(carve_gate=1, min_miss=125, miss_ratio=0.5, **RANGE)
    some = check_diff(H, T, V, scan, pose, dict(RANGE, carve_gate=1, min_miss=125, miss_ratio=0.5), misses=M)[1]
    assert 0 < (some["labels"][is_box] == reg.DIFF_NEW).sum() < is_box.sum()
    H.close()


def test_the_corner(hip_module):
    poses, clouds, scan, truth = LS.corner()
    H, T, V = surfeled_with_map(hip_module, poses, clouds, CS.MASK, LS.CORNER["voxel"])
    info, _ = check_diff(H, T, V, scan, truth)
    assert info["n_surface"] == len(scan)
    info, _ = check_diff(H, T, V, scan, LS.offset(truth, *LS.CORNER_START))
    assert 0 < info["n_surface"] < len(scan)
    H.close()


def test_the_static_pass(static):
    H, T, V, scan, truth = static
    H.closed_map_diff_configure(max_range=20.0)
    info, want = check_diff(H, T, V, scan, truth, dict(max_range=20.0))
    assert (info["skipped_rays"], info["steps"], info["tested"], info["through"], info["voxels_through"], info["voxels_hit"]) == \
           (2076, 384950, 27726, 2507, 877, 3022)
    assert len(check_gone(H, V, want)) == 266
    check_diff(H, T, V, scan, LS.offset(truth, 0.3, 0.02), dict(max_range=20.0))
    H.closed_map_diff_configure()
    info, want = check_diff(H, T, V, scan, truth)
    assert (info["skipped_rays"], info["steps"]) == (484, 511632) and len(check_gone(H, V, want)) == 291


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_block_boundaries(static, n):
    H, T, V, scan, truth = static
    H.closed_map_diff_configure()
    info, _ = check_diff(H, T, V, scan[5000:5000 + n], LS.offset(truth, 0.1, 0.01))
    assert info["n_points"] == info["rays"] == n


# ---- 2: the hand-made scan and the adversarial grid --------------------------------------------------------------------------
def hand_made_scan(R, t):
    """points in the sensor frame of the pose (R, t) -- R a signed permutation, t dyadic, so that every world point comes back
    exactly -- that hold every special case of the contract; world: what the points are in the map"""
    world = np.array([
        [np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [-np.inf, np.nan, 0.0],           # 0-2: not finite
        [2.0 ** 19 + 5.0, 0.0, 0.0], [0.0, -(2.0 ** 19) - 5.0, 1.0],               # 3-4: beyond the grid at v = 0.5
        t,                                                                         # 5: at the sensor: L == 0
        t + [0.0, 30.0, 0.0],                                                      # 6: beyond max_range = 12
        t + [0.125, 0.0625, -0.125],                                               # 7: inside the sensor's cell: 0 steps
        t + [4.0, 0.0, 0.0], t + [0.0, 4.75, 0.0], t + [0.0, 0.0, -1.0],            # 8-10: axis-parallel, d == 0 on two axes
        t + [-3.0, 0.0, 0.0],
        t + [2.0, 2.0, 0.0], t + [-1.5, 1.5, 0.0], t + [0.0, 2.5, 2.5],            # 12-14: tMax ties on two axes
        t + [2.0, 2.0, 2.0], t + [-1.0, 1.0, -1.0], t + [1.5, 4.5, 1.5],           # 15-17: ... and on three (17: not a diagonal)
        t + [0.5, 4.75, 0.0], t + [-0.5, 4.75, 0.5],                                # 18-19: onto the wall
    ])
    with np.errstate(invalid="ignore"):
        return np.ascontiguousarray((world - t) @ R), world


def test_the_hand_made_scan(gone, hip_module):
    H, T, V, _ = gone
    t = np.array([6.25, 0.25, 1.25])   # a cell centre at v = 0.5
    for R in (np.eye(3), Rz90):
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3] = R, t
        scan, world = hand_made_scan(R, t)
        E = CN.transform(pose, scan)
        assert np.array_equal(E[5:], world[5:])                     # the pose gives the world points back exactly
        walk = CN.Walk(np.tile(t / DS.VOXEL, (len(E) - 7, 1)), E[7:] / DS.VOXEL)
        tie = (walk.tmax == walk.tmax.min(axis=1, keepdims=True)).sum(axis=1)
        assert walk.n[0] == 0 and (tie[5:8] == 2).all() and (tie[8:10] == 3).all()   # (the ties are there from the first step)
        assert ((walk.step[1:5] != 0).sum(axis=1) == 1).all()                        # d == 0 on two axes
        info, want = check_diff(H, T, V, scan, pose, RANGE)
        assert list(want["labels"][:5]) == [hip_module.DIFF_INVALID] * 5 and want["labels"][5] != hip_module.DIFF_INVALID
        assert info["n_invalid"] == 5 and info["skipped_rays"] == 7 and (want["labels"][18:] == hip_module.DIFF_SURFACE).all()
    # a turned pose that rounds: the same scan under a general rotation
    pose = LS.offset(pose, 0.05, 0.3)
    check_diff(H, T, V, scan, pose, RANGE)
    check_diff(H, T, V, np.concatenate([scan, DS.gone()[2]]), pose, RANGE)


@pytest.mark.parametrize("voxel,origin", [(1.0, (1.0, -2.0, 0.5)), (0.3, (-0.37, 12.5, 0.11))])
def test_the_adversarial_grid(hip_module, voxel, origin):
    """section 22's map: negative cells, a non-zero origin and q = 2^24, the localiser's gate opened to every solved voxel; the
    scan is the map's own centroids, and points between them, under a small pose offset"""
    poses, clouds = TS.adversarial_plus(voxel, origin)
    H, T, V = surfeled_with_map(hip_module, poses, clouds, 0xFF, voxel, origin, min_points=3, min_planarity=-1.0)
    assert (T.c < 0.0).any() and T.eligible.sum() >= 15
    pose = LS.offset(np.eye(4), 0.05 * voxel, 1e-4)
    pose[:3, 3] += np.median(T.c, axis=0)
    world = np.concatenate([T.c, 0.5 * (T.c[:-1] + T.c[1:]), T.c + 0.3 * voxel])
    scan = (world - pose[:3, 3]) @ pose[:3, :3]
    cfg = dict(max_range=1e4, end_margin=0.2 * voxel, radius=0.5 * voxel, near=0.4 * voxel, plane_tol=0.02 * voxel)
    H.closed_map_diff_configure(**cfg)
    info, want = check_diff(H, T, V, scan, pose, cfg)
    assert info["n_surface"] > 0 and info["n_occupied"] > 0 and info["voxels_hit"] > 0 and info["tested"] > 0
    check_gone(H, V, want, min_through=1, gone_ratio=0.0)
    H.close()


# ---- 3: accumulation, determinism, non-interference, the detached map ----------------------------------------------------------
def test_accumulate(gone, hip_module):
    H, T, V, _ = gone
    H.closed_map_diff_configure(**RANGE)   # (drops the counts)
    with not_ready(hip_module):
        H.closed_map_diff_counts()
    scans = [DS.gone(s)[2:] for s in DS.SENSORS]
    state = None
    for k, (scan, pose) in enumerate(scans):   # accumulating into nothing starts from zero
        info, state = check_diff(H, T, V, scan, pose, RANGE, accumulate=True, state=state)
        assert info["scans"] == k + 1
    singles = [DN.diff(T, V, scan, pose, RANGE) for scan, pose in scans]
    assert np.array_equal(state["through"], sum(s["through"] for s in singles))
    assert np.array_equal(state["hits"], sum(s["hits"] for s in singles)) and info["scans"] == 3
    info, one = check_diff(H, T, V, *scans[1], RANGE)            # without the flag: the single result again
    assert info["scans"] == 1 and np.array_equal(one["through"], singles[1]["through"])


def test_calls_and_contexts_give_the_same_bytes(static, hip_module):
    H, T, V, scan, truth = static
    H.closed_map_diff_configure()
    pose = LS.offset(truth, 0.3, 0.02)
    a = H.closed_map_diff(scan, pose, want_ids=True)
    ca = counts_bytes(H)
    b = H.closed_map_diff(scan, pose, want_ids=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and {**a[2], "prepared": 0} == {**b[2], "prepared": 0}
    assert counts_bytes(H) == ca
    poses, clouds = CS.static_pass()
    other, _ = surfeled(hip_module, poses, clouds, CS.MASK, CS.STATIC["voxel"], reserve_voxels=64)
    c = other.closed_map_diff(scan, pose, want_ids=True)
    assert c[2]["prepared"] == 1 and {**c[2], "prepared": 0, "launches": 0} == {**a[2], "prepared": 0, "launches": 0}
    assert c[0].tobytes() == a[0].tobytes() and c[1].tobytes() == a[1].tobytes() and counts_bytes(other) == ca
    other.close()


def test_a_diff_changes_nothing_else_and_a_detached_map_diffs_alike(hip_module):
    reg = hip_module
    poses, clouds, scan, pose, _ = DS.ghost_gate()
    H, T, V = surfeled_with_map(reg, poses, clouds, CS.MASK, DS.VOXEL)
    H.closed_map_carve_configure(**RANGE)
    H.closed_map_carve()
    prior = LS.offset(pose, 0.1, 0.01)

    def everything(X):
        rows = X.closed_map_read()
        found = X.closed_map_localise(scan, prior)
        return (bits(rows[0]) + rows[1].tobytes(), X.closed_map_misses().tobytes(), TS.surfel_bytes(X), bits(found[0]),
                {**found[1], "prepared": 0}, log_bytes(X.closed_map_localise_log()), X.closed_map_save(), X.closed_map_save(clouds=True))

    before = everything(H)
    H.closed_map_diff_configure(carve_gate=1, **RANGE)
    mine = H.closed_map_diff(scan, pose, want_ids=True)
    H.closed_map_diff(scan, prior, accumulate=True)
    assert everything(H) == before
    # a carve pass or a surfel pass leaves the counts
    counts = counts_bytes(H)
    H.closed_map_carve()
    H.closed_map_surfels()
    assert counts_bytes(H) == counts and H.closed_map_diff_info()["scans"] == 2
    # the detached map: saved without clouds, loaded into a fresh context, diffed there
    mine = H.closed_map_diff(scan, pose, want_ids=True)
    counts = counts_bytes(H)
    F = reg.HipRegistration()
    F.closed_map_load(before[6])
    with not_ready(reg):
        F.closed_map_diff_counts()                                  # the snapshot holds no counts
    with not_ready(reg):
        F.closed_map_carve()                                        # detached
    F.closed_map_diff_configure(carve_gate=1, **RANGE)
    theirs = F.closed_map_diff(scan, pose, want_ids=True)
    assert theirs[0].tobytes() == mine[0].tobytes() and theirs[1].tobytes() == mine[1].tobytes() and counts_bytes(F) == counts
    assert {**theirs[2], "prepared": 0, "launches": 0} == {**mine[2], "prepared": 0, "launches": 0}
    assert F.closed_map_save() == before[6]
    # a load replaces the map: the counts go
    H.closed_map_load(before[7])
    with not_ready(reg):
        H.closed_map_diff_counts()
    assert H.closed_map_diff_info()["scans"] == 0
    H.close(); F.close()


def test_a_map_without_voxels(hip_module):
    """a built map's slot table is there when the map holds nothing: every probe of either kernel finds a free slot"""
    reg = hip_module
    H = reg.HipRegistration()
    H.place_configure(enabled=1, exclude_recent=8)
    H.loop_configure(enabled=1)
    assert H.closed_map_build(0)["n_voxels"] == 0          # no keyframes: an empty map, built
    H.closed_map_surfels()
    scan, pose = DS.gone()[2:]
    labels, ids, info = H.closed_map_diff(scan[:300], pose, want_ids=True)
    assert (labels == reg.DIFF_NEW).all() and (ids == -1).all() and info["n_new"] == 300 and info["steps"] > 0
    assert (info["tested"], info["through"], info["voxels_through"], info["voxels_hit"], info["skipped_rays"]) == (0, 0, 0, 0, 0)
    assert len(H.closed_map_diff_counts()[0]) == 0 and len(H.closed_map_read_gone()[0]) == 0
    H.close()


# ---- 4: refusals and lifecycle -------------------------------------------------------------------------------------------------
def test_refusals_and_lifecycle(hip_module):
    reg = hip_module
    poses, clouds, scan, pose = DS.gone()
    H = context(reg, poses, clouds, voxel=DS.VOXEL, cloud_mask=CS.MASK)
    with not_ready(reg):
        H.closed_map_diff(scan, pose)                               # no map
    H.closed_map_build(2, poses)
    with not_ready(reg):
        H.closed_map_diff(scan, pose)                               # no surfels
    for call in (H.closed_map_diff_counts, H.closed_map_read_gone):
        with not_ready(reg):
            call()                                                  # no counts
    H.closed_map_surfels()
    H.closed_map_diff_configure(**RANGE)
    labels, ids, info = H.closed_map_diff(scan, pose, want_ids=True)
    assert info["prepared"] == 1 and info["launches"] == 5 and info["scans"] == 1
    counts, cfg_info = counts_bytes(H), H.closed_map_diff_info()

    def untouched():
        return counts_bytes(H) == counts and H.closed_map_diff_info() == cfg_info

    import ctypes as C
    flat, col = np.ascontiguousarray(scan).ctypes.data_as(C.POINTER(C.c_double)), np.ascontiguousarray(pose.T).reshape(-1)
    colp = col.ctypes.data_as(C.POINTER(C.c_double))
    assert H.L.tloam_closed_map_diff(H.h, flat, len(scan), colp, 2, None, None, None) == -1       # unknown flags
    assert H.L.tloam_closed_map_diff(H.h, flat, len(scan), colp, -1, None, None, None) == -1
    assert H.L.tloam_closed_map_diff(H.h, None, len(scan), colp, 0, None, None, None) == -1
    assert H.L.tloam_closed_map_diff(H.h, flat, len(scan), None, 0, None, None, None) == -1
    assert untouched()
    assert H.L.tloam_closed_map_diff(H.h, flat, len(scan), colp, 0, None, None, None) == 0         # labels and ids may be NULL
    assert counts_bytes(H) == counts and H.closed_map_diff_info() == {**cfg_info, "prepared": 0, "launches": 4}
    cfg_info = H.closed_map_diff_info()
    for bad_pose in (2.0 * np.eye(4), np.full((4, 4), np.nan), np.diag([1.0, 1.0, -1.0, 1.0])):
        with invalid(reg):
            H.closed_map_diff(scan, bad_pose)
    shifted = pose.copy()
    shifted[0, 3] = np.inf
    with invalid(reg):
        H.closed_map_diff(scan, shifted)
    with invalid(reg):
        H.closed_map_diff(np.zeros((0, 3)), pose)                   # n == 0
    assert untouched()
    for bad in (dict(max_range=0.0), dict(max_range=float("inf")), dict(max_range=float("nan")), dict(end_margin=-1.0),
                dict(end_margin=float("inf")), dict(radius=0.0), dict(radius=float("nan")), dict(plane_tol=-1e-9),
                dict(plane_tol=float("inf")), dict(plane_tol=float("nan")), dict(near=-1.0), dict(near=float("inf")),
                dict(near=float("nan")), dict(min_miss=-1), dict(miss_ratio=float("nan")), dict(carve_gate=2), dict(carve_gate=-1)):
        with invalid(reg):
            H.closed_map_diff_configure(**bad)
    with pytest.raises(KeyError):
        H.closed_map_diff_configure(ray_mask=1)
    assert untouched()                                             # the old configuration stays, and the counts with it
    again = H.closed_map_diff(scan, pose, want_ids=True)
    assert again[0].tobytes() == labels.tobytes() and again[1].tobytes() == ids.tobytes() and counts_bytes(H) == counts
    assert again[2] == {**info, "prepared": 0, "launches": 4}
    # the surfels dropped under the counts: refused, and the counts stay
    H.closed_map_surfel_configure(min_points=6)
    with not_ready(reg):
        H.closed_map_diff(scan, pose)
    assert untouched()
    H.closed_map_surfel_configure()
    H.closed_map_surfels()
    assert H.closed_map_diff(scan, pose, want_ids=True)[1].tobytes() == ids.tobytes() and counts_bytes(H) == counts
    # the gate on a map that is not carved
    H.closed_map_diff_configure(carve_gate=1, **RANGE)             # (a configure drops the counts)
    with not_ready(reg):
        H.closed_map_diff_counts()
    with not_ready(reg):
        H.closed_map_diff(scan, pose)
    H.closed_map_diff_configure(**RANGE)
    H.closed_map_diff(scan, pose)
    H.closed_map_diff_configure(carve_gate=1, **RANGE)
    H.closed_map_carve_configure(**RANGE)
    H.closed_map_carve()
    assert H.closed_map_diff(scan, pose)[0].tobytes() == labels.tobytes()   # the wall's voxels are not seen through
    counts, cfg_info = counts_bytes(H), H.closed_map_diff_info()
    H.closed_map_carve_configure(max_range=11.0)                    # drops the carve's counts: the gate has nothing to read
    with not_ready(reg):
        H.closed_map_diff(scan, pose)
    assert untouched()                                             # the refusal leaves the diff's counts
    H.closed_map_carve()
    assert H.closed_map_diff(scan, pose)[0].tobytes() == labels.tobytes()
    # the localiser's gate rebuilds the records, for either stage
    H.closed_map_localise_configure(min_planarity=0.5)
    assert H.closed_map_diff(scan, pose)[2]["prepared"] == 1 and H.closed_map_localise(scan, pose)[1]["prepared"] == 0
    H.closed_map_localise_configure()
    assert H.closed_map_localise(scan, pose)[1]["prepared"] == 1 and H.closed_map_diff(scan, pose)[2]["prepared"] == 0
    # what empties the map drops the counts; the configuration persists across a reset
    H.closed_map_diff_configure(max_range=7.0, near=0.125)
    H.closed_map_diff(scan, pose)
    H.closed_map_build(2, poses)
    with not_ready(reg):
        H.closed_map_diff_counts()
    assert H.closed_map_diff_info()["scans"] == 0
    H.odometry_reset(None, TS.TC.odom_cfg(reg))
    for k in range(len(poses)):
        assert H.place_add_scan(TS.DUMMY, np.eye(4), k) == k
        H.place_set_keyframe_clouds(k, *clouds[k])
    H.closed_map_build(2, poses)
    H.closed_map_surfels()
    T, V = LS.target(poses, clouds, CS.MASK, DS.VOXEL)[4], CN.build_map(poses, clouds, CS.MASK, DS.VOXEL)
    check_diff(H, T, V, scan, pose, dict(max_range=7.0, near=0.125))
    H.close()
    # nranks > 1: every diff call is refused
    H = reg.HipRegistration()
    H.comm_init_callback(0, 2, lambda dev, count, stream: 0)
    for call in (H.closed_map_diff_configure, lambda: H.closed_map_diff(scan, pose), H.closed_map_diff_info,
                 lambda: H.closed_map_diff_counts(0, 0), H.closed_map_read_gone):
        with invalid(reg):
            call()
    H.close()
