"""-m gpu: the surfels of the closed map (tl_surfel.hip, tl_api_surfel.hip) against their numpy restatement
(tests/closed_map_surfel_np.py), bit for bit: the thirteen sums, the normals, the variances, every counter and the box reads.
Keyframes are hand-made as in tests/test_gpu_closed_map_carve.py and built under the caller's poses (pose_source 2)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_carve_np as CN  # noqa: E402
import closed_map_surfel_np as SN  # noqa: E402
import test_gpu_closed_map as TC  # noqa: E402
import test_gpu_closed_map_carve as TV  # noqa: E402
from tloam_amd import map_io, synth_hdl64 as G  # noqa: E402

pytestmark = pytest.mark.gpu

bits, invalid, not_ready = TC.bits, TC.invalid, TC.not_ready
context, built, DUMMY = TV.context, TV.built, TV.DUMMY
READS = (dict(), dict(lo=[-30.0, -30.0, -5.0], hi=[30.0, 30.0, 5.0], min_count=2, max_sigma=0.05, min_planarity=0.2),
         dict(min_planarity=0.0), dict(max_sigma=0.0, min_planarity=-1.0))


def surfel_bytes(H):
    n, e, c = H.closed_map_read_surfels()
    return H.closed_map_moments().tobytes() + bits(n) + bits(e) + c.tobytes()


def surfels_and_compare(H, V, poses, clouds, mask, min_points=5, reads=READS):
    """one pass on the device and in the restatement: the counters, the sums, the surfels, the box reads -> (info, S, normals, evals)"""
    H.closed_map_surfel_configure(min_points=min_points)
    info = H.closed_map_surfels()
    S, normals, evals, want = SN.surfels(V, poses, clouds, mask, min_points)
    print(f"mask {mask:#04x} min_points {min_points}: {info}")
    assert H.closed_map_surfel_info() == info
    assert {k: v for k, v in info.items() if k not in ("launches", "reserved0")} == want
    assert H.closed_map_moments().tobytes() == S.tobytes()
    n, e, c = H.closed_map_read_surfels()
    assert c.tobytes() == S[:, 0].tobytes() and bits(n) == bits(normals) and bits(e) == bits(evals)
    if len(S) >= 3:
        n, e, c = H.closed_map_read_surfels(1, 2)
        assert c.tobytes() == S[1:3, 0].tobytes() and bits(n) == bits(normals[1:3]) and bits(e) == bits(evals[1:3])
        assert H.closed_map_moments(1, 2).tobytes() == S[1:3].tobytes()
    C = V.centroids()
    for read in reads:
        ids = SN.read_box(V, S, evals, min_points=min_points, **read)
        cen, n, e, c = H.closed_map_read_surfels_box(**read)
        assert bits(cen) == bits(C[ids]) and bits(n) == bits(normals[ids]) and bits(e) == bits(evals[ids]), read
        assert c.tobytes() == S[ids, 0].tobytes(), read
    return info, S, normals, evals


# ---- 1: the ghost scene ----------------------------------------------------------------------------------------------------
def test_the_ghost_scene(hip_module, tmp_path):
    poses, clouds, wall, box = CS.ghost_scene()
    v = CS.GHOST["voxel"]
    H, V = built(hip_module, poses, clouds, CS.MASK, v)
    info, S, normals, evals = surfels_and_compare(H, V, poses, clouds, CS.MASK, min_points=5)
    assert info["orphan_points"] == 0 and H.closed_map_moments()[:, 0].tobytes() == H.closed_map_read()[1].tobytes()   # Ns == N
    cen, nrm, ev, cnt = H.closed_map_read_surfels_box(min_planarity=0.05)
    cells = {tuple(c) for c in np.floor(wall / v).astype(np.int64).tolist()}
    on_wall = np.array([tuple(c) in cells for c in np.floor(cen / v).astype(np.int64).tolist()])
    assert len(cells) == 175 and int(on_wall.sum()) == 144
    assert np.all(nrm[on_wall] == np.array([0.0, -1.0, 0.0])) and np.all(ev[on_wall, 0] == 0.0)
    path = str(tmp_path / "surfels.pcd")
    assert map_io.write_closed_map_surfel_pcd(path, H) == len(cnt)
    c2, n2, k2 = map_io.read_surfel_pcd(path)
    assert bits(c2) == bits(cen) and bits(n2) == bits(nrm) and k2.tobytes() == cnt.tobytes()
    H.close()


# ---- 2: the adversarial set ------------------------------------------------------------------------------------------------
def hand_made(v, origin, base, sensor):
    """-> (pose, points in the keyframe's frame): voxels of 1, 2 and 4 points, five collinear points, a thousand points in one
    voxel starting at lane 12 of a wave, and a point whose offset rounds to q = 2^24; `base` is the first voxel's cell"""
    rng = np.random.default_rng(8)
    o, b = np.asarray(origin, np.float64), np.asarray(base, np.float64)
    cell = lambda dx, frac: b + np.array([dx, 0.0, 0.0]) + np.asarray(frac, np.float64)  # noqa: E731
    g = [cell(0, [0.5, 0.5, 0.5])]
    g += [cell(2, [0.2, 0.3, 0.4]), cell(2, [0.7, 0.3, 0.5])]
    g += [cell(4, f) for f in ([0.1, 0.1, 0.1], [0.9, 0.1, 0.2], [0.1, 0.9, 0.3], [0.8, 0.8, 0.4])]
    g += [cell(6, 0.1 + t * np.array([0.1, 0.15, 0.2])) for t in range(5)]
    g += [cell(8, f) for f in rng.uniform(0.05, 0.95, (1000, 3))]
    g += [cell(10, [1.0 - 2.0 ** -30, 0.5, 0.5])]
    t = o + v * (b + np.asarray(sensor, np.float64))
    return TV.yaw_pose(t, 0.0), (o + v * np.array(g)) - t


def adversarial_plus(v, origin):
    """tests/test_gpu_closed_map_carve.py's four keyframes, and the hand-made voxels twice: as a source cloud (keyframe 4) and
    as a target cloud (keyframe 5), far apart, so that every mask of the test selects them"""
    poses, clouds = TV.adversarial(v, origin)
    none = CS.NONE
    P4, h4 = hand_made(v, origin, (1000, 1000, 0), (5.0, -3.0, 0.5))
    P5, h5 = hand_made(v, origin, (-2000, 500, 3), (5.0, 4.0, -2.5))
    clouds = clouds + [[[h4, none, none, none], [none] * 4], [[none] * 4, [none, h5, none, none]]]
    return np.concatenate([poses, [P4, P5]]), clouds


@pytest.mark.parametrize("voxel,origin", [(1.0, (1.0, -2.0, 0.5)), (0.3, (-0.37, 12.5, 0.11))])
def test_the_adversarial_set(hip_module, voxel, origin):
    poses, clouds = adversarial_plus(voxel, origin)
    launches = set()
    for mask in (0xF0, 0x0F, 0x21):
        H, V = built(hip_module, poses, clouds, mask, voxel, origin)
        info, S, normals, evals = surfels_and_compare(H, V, poses, clouds, mask)
        launches.add(info["launches"])
        assert info["orphan_points"] == 0 and np.array_equal(S[:, 0], V.N)
        for base in ([1000, 1000, 0], [-2000, 500, 3])[(0 if mask & 0x01 else 1):(2 if mask & 0x20 else 1)]:
            ids = [int(np.flatnonzero((V.i == np.array(base) + [dx, 0, 0]).all(axis=1))[0]) for dx in (0, 2, 4, 6, 8, 10)]
            assert S[ids, 0].tolist() == [1, 2, 4, 5, 1000, 1]
            assert not normals[ids[:3]].any() and not evals[ids[:3]].any() and not normals[ids[5]].any()       # unsolved
            assert abs(np.linalg.norm(normals[ids[3]]) - 1.0) < 1e-12 and evals[ids[3], 2] > 0.0              # the line: solved ...
            kept = SN.read_box(V, S, evals)
            assert ids[3] not in kept and ids[4] in kept                                                      # ... and gated out
            assert S[ids[5], 1] == 65536                                                                      # q = 2^24
        # the gate's parts one at a time on the same surfels, and another min_points
        surfels_and_compare(H, V, poses, clouds, mask, min_points=3, reads=READS[:1])
        H.close()
    assert len(launches) == 1


# ---- 3: overflow keyframes and orphans -------------------------------------------------------------------------------------
def test_overflow_keyframes_and_orphans(hip_module):
    rng = np.random.default_rng(12)
    v = 0.5
    a = rng.uniform(-4.0, 4.0, (700, 3))
    far = rng.uniform(-4.0, 4.0, (300, 3))
    poses = np.array([TV.yaw_pose([1.0, 2.0, 0.5], 0.3), TV.yaw_pose([1.5, 2.0, 0.5], 0.3), TV.yaw_pose([300.0, -80.0, 1.0], -1.0),
                      TV.yaw_pose([5.0e6, 0.0, 0.0], 0.0)])
    # keyframe 3 stands ten million voxels from what it sees (beside keyframe 2's surfaces): its w_x is clamped to 2^30
    seen_from_afar = (np.array([300.0, -80.0, 1.0]) + rng.uniform(-3.0, 3.0, (50, 3))) - poses[3][:3, 3]
    # keyframe 1 sees keyframe 0's surfaces and has one point beyond the grid: an overflow keyframe of the build and of the pass
    beyond = np.concatenate([a[:400] - [0.5, 0.0, 0.0], [[v * 2.0 ** 21, 0.0, 0.0]], a[400:] - [0.5, 0.0, 0.0]])
    clouds = [CS.slot0(a), CS.slot0(beyond), CS.slot0(far), CS.slot0(seen_from_afar)]
    H, V = built(hip_module, poses, clouds, CS.MASK, v)
    assert H.closed_map_info()["overflow_keyframes"] == 1
    info, S, _, _ = surfels_and_compare(H, V, poses, clouds, CS.MASK)
    assert info["orphan_points"] == 0 and info["n_points"] == 1050 and np.array_equal(S[:, 0], V.N)
    assert S[:, 10].max() >= 1 << 30
    third = H.closed_map_moments()[len(V.keys) - 1].tobytes()
    # keyframe 0's cloud re-attached, moved: its points are orphans or fall into other voxels; keyframe 1 loses its far point and
    # now adds; keyframe 2's voxels keep their sums
    now = [CS.slot0(a + [0.0, 30.0, 0.0]), CS.slot0(np.delete(beyond, 400, axis=0)), clouds[2], clouds[3]]
    H.place_set_keyframe_clouds(0, *now[0])
    H.place_set_keyframe_clouds(1, *now[1])
    info2, S2, _, _ = surfels_and_compare(H, V, poses, now, CS.MASK)
    assert info2["orphan_points"] > 0 and info2["n_points"] + info2["orphan_points"] == 1750
    from_third = np.flatnonzero(np.linalg.norm(V.centroids() - poses[2][:3, 3], axis=1) < 20.0)
    assert len(from_third) > 0 and np.array_equal(S2[from_third], S[from_third]) and not np.array_equal(S2, S)
    assert H.closed_map_moments()[len(V.keys) - 1].tobytes() == third
    cen, cnt = H.closed_map_read()
    assert cnt.tobytes() == V.N.tobytes() and bits(cen) == bits(V.centroids())      # the map is the build's still
    H.close()


# ---- 4: the same bits ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def static():
    return CS.static_pass()


def test_forms_passes_and_contexts_give_the_same_bits(hip_module, static, monkeypatch):
    poses, clouds = static
    v = CS.STATIC["voxel"]
    H, V = built(hip_module, poses, clouds, CS.MASK, v)
    info, S, _, _ = surfels_and_compare(H, V, poses, clouds, CS.MASK, reads=READS[:2])
    assert info["n_points"] > 100000 and info["solved_voxels"] > 1000 and np.array_equal(S[:, 0], V.N)
    want = surfel_bytes(H)
    assert H.closed_map_surfels() == info and surfel_bytes(H) == want              # a pass replaces the sums: it does not add
    monkeypatch.setenv("TLOAM_SURFEL_NO_RUNS", "1")                                 # plain atomics, read per pass
    assert H.closed_map_surfels() == info and surfel_bytes(H) == want
    monkeypatch.delenv("TLOAM_SURFEL_NO_RUNS")
    assert H.closed_map_surfels() == info and surfel_bytes(H) == want
    box = H.closed_map_read_surfels_box()
    H.close()
    other, _ = built(hip_module, poses, clouds, CS.MASK, v, reserve_voxels=64)        # the rows grown inside the build
    assert other.closed_map_surfels() == info and surfel_bytes(other) == want
    for x, y in zip(other.closed_map_read_surfels_box(), box):
        assert x.tobytes() == y.tobytes()
    # launches: another size and two other masks
    for mask in (0x20, 0xFF):
        other.closed_map_configure(voxel=v, cloud_mask=mask)
        other.closed_map_build(2, poses)
        i = other.closed_map_surfels()
        assert i["launches"] == info["launches"] and i["n_points"] == (0 if mask == 0x20 else info["n_points"])
    other.close()
    half, Vh = built(hip_module, poses[:4], clouds[:4], CS.MASK, v)
    ih, _, _, _ = surfels_and_compare(half, Vh, poses[:4], clouds[:4], CS.MASK, reads=READS[:1])
    assert ih["launches"] == info["launches"] and ih["n_points"] < info["n_points"]
    half.close()


# ---- 5: undisturbed --------------------------------------------------------------------------------------------------------
def test_odometry_the_closed_map_and_the_carve_are_undisturbed(hip_module):
    reg = hip_module
    seq = G.sequence(7, seed=3)[0]
    seen = []

    def surfels_between_frames(f, H):
        if f in (2, 4, 6):
            H.closed_map_build(0)
            seen.append(H.closed_map_surfels())
            H.closed_map_moments()
            H.closed_map_read_surfels()
            H.closed_map_read_surfels_box()

    def closed_map_bytes(H):
        cen, cnt = H.closed_map_read()
        bc, bn = H.closed_map_read_box([-50.0] * 3, [50.0] * 3, 2)
        carved = H.closed_map_read_carved()
        return (bits(cen) + cnt.tobytes() + bits(bc) + bn.tobytes() + bits(H.closed_map_poses()) + H.closed_map_misses().tobytes() +
                bits(carved[0]) + carved[1].tobytes() + carved[2].tobytes() + repr(H.closed_map_carve_info()).encode())

    Hoff, off = TC.odom_run(reg, seq)
    Hon, on = TC.odom_run(reg, seq, hook=surfels_between_frames)
    assert len(seen) == 3 and seen[-1]["n_points"] > 0 and seen[-1]["solved_voxels"] > 0
    for f, (a, b) in enumerate(zip(on, off)):
        assert bits(a["pose"]) == bits(b["pose"]) and bits(a["reg"]) == bits(b["reg"]), f
        sa, sb = a["stats"], b["stats"]
        for key in sb:
            if key != "match":
                assert sa[key] == sb[key], (f, key)
        for key, val in sb["match"].items():
            if key != "host_wait_us":
                assert np.asarray(sa["match"][key]).tobytes() == np.asarray(val).tobytes(), (f, key)
        assert a["map_info"] == b["map_info"] and bits(a["map"]) == bits(b["map"]) and a["vinfo"] == b["vinfo"], f
        for x, y in zip(a["vmap"], b["vmap"]):
            assert x.tobytes() == y.tobytes(), f
    assert bits(Hon.graph_poses()) == bits(Hoff.graph_poses())
    for H in (Hon, Hoff):
        H.closed_map_build(1)
        H.closed_map_carve_configure(max_range=30.0)
        H.closed_map_carve()
    before = closed_map_bytes(Hon)
    info = Hon.closed_map_surfels()
    Hon.closed_map_read_surfels_box()
    assert closed_map_bytes(Hon) == before == closed_map_bytes(Hoff)
    # and a carve leaves the surfels as they were
    want = surfel_bytes(Hon)
    Hon.closed_map_carve()
    Hon.closed_map_read_carved()
    Hon.closed_map_carve_configure(max_range=20.0)
    assert surfel_bytes(Hon) == want and Hon.closed_map_surfel_info() == info
    Hon.close(); Hoff.close()


# ---- 6: lifecycle ----------------------------------------------------------------------------------------------------------
def test_lifecycle(hip_module):
    reg = hip_module
    poses, clouds, _, _ = CS.ghost_scene()
    v = CS.GHOST["voxel"]

    def no_surfels(H):
        for read in (lambda: H.closed_map_moments(0, 0), lambda: H.closed_map_read_surfels(0, 0), lambda: H.closed_map_read_surfels_box()):
            with not_ready(reg):
                read()
        assert H.closed_map_surfel_info()["n_keyframes"] == 0 and H.closed_map_surfel_info()["launches"] == 0

    def refill(H):
        if H.place_info()["n_keyframes"] == 0:
            for k in range(6):
                assert H.place_add_scan(DUMMY, np.eye(4), k) == k
                H.place_set_keyframe_clouds(k, *clouds[k])

    H = context(reg, poses, clouds, keep=range(4), voxel=v, cloud_mask=CS.MASK)
    no_surfels(H)
    with not_ready(reg):
        H.closed_map_surfels()                    # before a build
    H.closed_map_build(2, poses[:4])
    no_surfels(H)
    info = H.closed_map_surfels()
    V = CN.build_map(poses[:4], clouds[:4], CS.MASK, v)
    S, normals, evals, want = SN.surfels(V, poses[:4], clouds[:4], CS.MASK)
    have = surfel_bytes(H)
    assert have == S.tobytes() + bits(normals) + bits(evals) + S[:, 0].tobytes() and info["n_keyframes"] == 4
    nv = len(S)
    for read in (H.closed_map_moments, H.closed_map_read_surfels):
        with invalid(reg):
            read(0, nv + 1)
        with invalid(reg):
            read(nv + 1, 0)
        read(nv, 0)
    # a refused configuration or build leaves the surfels readable and equal
    for bad in (2, 0, -1):
        with invalid(reg):
            H.closed_map_surfel_configure(min_points=bad)
    with invalid(reg):
        H.closed_map_build(2, poses[:3])
    assert surfel_bytes(H) == have and H.closed_map_surfel_info() == info
    # keyframes added after the build add nothing
    for k in (4, 5):
        assert H.place_add_scan(DUMMY, np.eye(4), k) == k
        H.place_set_keyframe_clouds(k, *clouds[k])
    assert H.closed_map_surfels() == info and surfel_bytes(H) == have
    # a carve and its configuration leave the surfels; a surfel configuration drops the surfels alone
    H.closed_map_carve_configure(max_range=12.0)
    H.closed_map_carve()
    misses = H.closed_map_misses().tobytes()
    assert surfel_bytes(H) == have
    H.closed_map_surfel_configure(min_points=3)
    no_surfels(H)
    assert H.closed_map_misses().tobytes() == misses and len(H.closed_map_read()[1]) == nv
    assert H.closed_map_surfels()["solved_voxels"] == int((S[:, 0] >= 3).sum()) >= info["solved_voxels"]
    # a rebuild drops the surfels, and so does everything that empties the closed map
    H.closed_map_build(2, poses)
    no_surfels(H)
    assert H.closed_map_surfels()["n_keyframes"] == 6
    for drop in (lambda: H.closed_map_configure(voxel=v, cloud_mask=CS.MASK), lambda: H.place_configure(enabled=1, exclude_recent=8),
                 lambda: H.loop_configure(enabled=1), lambda: H.odometry_reset(None, TC.odom_cfg(reg))):
        refill(H)
        H.closed_map_build(2, poses)
        H.closed_map_surfels()
        H.closed_map_moments()
        drop()
        no_surfels(H)
        with not_ready(reg):
            H.closed_map_surfels()
    # the configuration persisted across the reset (min_points 3)
    refill(H)
    H.closed_map_build(2, poses)
    V = CN.build_map(poses, clouds, CS.MASK, v)
    assert H.closed_map_surfels()["solved_voxels"] == SN.surfels(V, poses, clouds, CS.MASK, 3)[3]["solved_voxels"] \
        > SN.surfels(V, poses, clouds, CS.MASK, 5)[3]["solved_voxels"]
    H.close()
    # nranks > 1: every surfel call is refused
    H = reg.HipRegistration()
    H.comm_init_callback(0, 2, lambda dev, count, stream: 0)
    for call in (H.closed_map_surfel_configure, H.closed_map_surfels, H.closed_map_surfel_info, lambda: H.closed_map_moments(0, 0),
                 lambda: H.closed_map_read_surfels(0, 0), H.closed_map_read_surfels_box):
        with invalid(reg):
            call()
    H.close()


# ---- 7: the three box reads are one selection ------------------------------------------------------------------------------
def test_the_three_box_reads_are_one_selection(hip_module):
    """closed_map_read_box, _read_carved with a min_miss no voxel reaches and _read_surfels_box with its gate open run one
    device body: the same voxels in the same order.  The ghost scene at 0.25 m is 762 voxels -- three blocks, the last of 250 --
    and the box keeps voxels of every block, so the ticket order, the look-back chain and the last block's total all take part."""
    import ctypes as C
    poses, clouds, _, _ = CS.ghost_scene()
    H, V = built(hip_module, poses, clouds, CS.MASK, 0.25)
    H.closed_map_carve_configure(max_range=CS.GHOST["max_range"])
    H.closed_map_carve()
    H.closed_map_surfel_configure(min_points=3)
    H.closed_map_surfels()
    cen, cnt = H.closed_map_read()
    _, ev, ns = H.closed_map_read_surfels()
    M = H.closed_map_misses()
    nv = len(cnt)
    assert 512 < nv < 1024 and nv % 256 != 0
    solved = (ns >= 3) & (ev[:, 2] > 0.0)
    lo, hi, mc = np.array([1.0, 2.2, 0.9]), np.array([9.0, 5.2, 3.1]), 2
    never, inf = 1 << 62, float("inf")
    for box in (False, True):
        keep = cnt >= mc
        if box:
            keep &= np.all((cen >= lo) & (cen <= hi), axis=1)
        where = dict(lo=lo, hi=hi) if box else dict()
        ids, ids_s = np.flatnonzero(keep), np.flatnonzero(keep & solved)
        blocks = {int(i) // 256 for i in ids_s}
        assert blocks == {0, 1, 2} and 0 < len(ids_s) < len(ids) < nv, box
        carved = H.closed_map_read_carved(min_count=mc, min_miss=never, **where)
        assert bits(carved[0]) == bits(cen[ids]) and carved[1].tobytes() == cnt[ids].tobytes(), box
        assert carved[2].tobytes() == M[ids].tobytes(), box
        if box:
            plain = H.closed_map_read_box(lo, hi, mc)
            assert bits(plain[0]) == bits(carved[0]) and plain[1].tobytes() == carved[1].tobytes()
        surf = H.closed_map_read_surfels_box(min_count=mc, max_sigma=inf, min_planarity=-inf, **where)
        assert bits(surf[0]) == bits(cen[ids_s]) and surf[3].tobytes() == ns[ids_s].tobytes(), box
        assert bits(surf[0]) == bits(carved[0][solved[ids]]), box      # the carved read's voxels, the unsolved ones left out
    # a capacity one short: INVALID, *n the size, nothing copied (the box is the last pass's: ids, ids_s)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    out = np.full((len(ids), 3), 7.0)
    n = C.c_size_t(0)
    calls = ((ids, lambda cap: H.L.tloam_closed_map_read_box(H.h, dp(lo), dp(hi), mc, cap, C.byref(n), dp(out), None)),
             (ids, lambda cap: H.L.tloam_closed_map_read_carved(H.h, dp(lo), dp(hi), mc, never, 1.0, cap, C.byref(n), dp(out), None,
                                                                None)),
             (ids_s, lambda cap: H.L.tloam_closed_map_read_surfels_box(H.h, dp(lo), dp(hi), mc, inf, -inf, cap, C.byref(n), dp(out),
                                                                       None, None, None)))
    for want, call in calls:
        out[:] = 7.0
        assert call(len(want) - 1) == -1 and n.value == len(want) and np.all(out == 7.0)
        assert call(len(want)) == 0 and n.value == len(want) and bits(out[:len(want)]) == bits(cen[want])
    H.close()
