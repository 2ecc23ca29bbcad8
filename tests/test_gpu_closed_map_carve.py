"""-m gpu: the carve of the closed map (tl_carve.hip, tl_api_carve.hip) against its numpy restatement
(tests/closed_map_carve_np.py), bit for bit: M, every counter, and read_carved's voxels.  Keyframes are hand-made through
place_add_scan + place_set_keyframe_clouds and built under the caller's poses (pose_source 2)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_carve_np as CN  # noqa: E402
import test_gpu_closed_map as TC  # noqa: E402
from tloam_amd import map_io, synth_hdl64 as G  # noqa: E402

pytestmark = pytest.mark.gpu

bits, invalid, not_ready = TC.bits, TC.invalid, TC.not_ready
DUMMY = np.random.default_rng(5).uniform(-20.0, 20.0, (200, 3))   # the scan a hand-made keyframe is described by
READS = (dict(), dict(lo=[-30.0, -30.0, -5.0], hi=[30.0, 30.0, 5.0], min_count=2, min_miss=1, miss_ratio=0.5),
         dict(min_miss=1, miss_ratio=0.0))


def context(reg, poses, clouds, keep=None, **closed_map_cfg):
    H = reg.HipRegistration()
    H.place_configure(enabled=1, exclude_recent=8)
    H.loop_configure(enabled=1)
    for k in (range(len(poses)) if keep is None else keep):
        assert H.place_add_scan(DUMMY, np.eye(4), k) == k
        H.place_set_keyframe_clouds(k, *clouds[k])
    H.closed_map_configure(**closed_map_cfg)
    return H


def carve_and_compare(H, V, poses, clouds, build_mask, ray_mask=0, reads=READS, **cfg):
    """one carve on the device and in the restatement: the counters, M, and read_carved's voxels -> (info, M)"""
    H.closed_map_carve_configure(ray_mask=ray_mask, **cfg)
    info = H.closed_map_carve()
    M, want = CN.carve(V, poses, clouds, ray_mask or build_mask, **cfg)
    print(f"ray_mask {ray_mask:#04x} {cfg}: {info}")
    assert H.closed_map_carve_info() == info
    assert {k: v for k, v in info.items() if k not in ("launches", "reserved0")} == want
    assert H.closed_map_misses().tobytes() == M.tobytes()
    assert H.closed_map_misses(1, 2).tobytes() == M[1:3].tobytes()
    C = V.centroids()
    for read in reads:
        ids = CN.read_carved(V, M, **read)
        cen, cnt, mis = H.closed_map_read_carved(**read)
        assert bits(cen) == bits(C[ids]) and cnt.tobytes() == V.N[ids].tobytes() and mis.tobytes() == M[ids].tobytes(), read
    return info, M


def built(reg, poses, clouds, mask, voxel=1.0, origin=(0.0, 0.0, 0.0), **kw):
    """a context with the closed map built, and the restated map, checked to be the same map"""
    H = context(reg, poses, clouds, voxel=voxel, origin=origin, cloud_mask=mask, **kw)
    H.closed_map_build(2, poses)
    V = CN.build_map(poses, clouds, mask, voxel, origin)
    cen, cnt = H.closed_map_read()
    assert cnt.tobytes() == V.N.tobytes() and bits(cen) == bits(V.centroids())
    return H, V


# ---- 1: the ghost scene ----------------------------------------------------------------------------------------------------
def test_the_ghost_scene(hip_module, tmp_path):
    poses, clouds, wall, box = CS.ghost_scene()
    v = CS.GHOST["voxel"]
    H, V = built(hip_module, poses, clouds, CS.MASK, v)
    info, M = carve_and_compare(H, V, poses, clouds, CS.MASK, max_range=CS.GHOST["max_range"])
    cen, cnt, mis = H.closed_map_read_carved()
    kept = {tuple(c) for c in np.floor(cen / v).astype(np.int64).tolist()}
    assert not kept & {tuple(c) for c in np.floor(box / v).astype(np.int64).tolist()}      # the ghost is gone ...
    assert {tuple(c) for c in np.floor(wall / v).astype(np.int64).tolist()} == kept         # ... and the wall is whole
    assert len(H.closed_map_read()[1]) == len(V.keys) > len(cnt)                          # _read still returns everything
    path = str(tmp_path / "carved.pcd")
    assert map_io.write_carved_closed_map_pcd(path, H) == len(cnt)
    c2, n2 = map_io.read_voxel_pcd(path)
    assert bits(c2) == bits(cen) and n2.tobytes() == cnt.tobytes()
    H.close()


# ---- 2: the adversarial set ------------------------------------------------------------------------------------------------
MAX_RANGE = 20.0


def yaw_pose(t, yaw):
    P = np.eye(4)
    P[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    P[:3, 3] = t
    return P


def unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1)[:, None]


def adversarial(v, origin):
    """four keyframes -> (poses, clouds); every cloud slot is used by some keyframe, with empty slots between"""
    rng = np.random.default_rng(33)
    o = np.asarray(origin, np.float64)
    rand = lambda n, r=15.0: unit(rng, n) * rng.uniform(0.2, r, (n, 1))  # noqa: E731
    none = CS.NONE
    # keyframe 0: a sensor on a cell corner; rays along the six axis directions, through cell corners and edges (whole
    # multiples of v), and random ones.  Clouds of 255, 1, 2 | 256, 257 and 300 points
    axes = np.concatenate([s * m * v * np.eye(3) for s in (1.0, -1.0) for m in (1, 4, 7)])
    i3 = np.array([[a, b, c] for a in (-3, 0, 2, 5) for b in (-4, 0, 3) for c in (-2, 0, 1)], np.float64) * v
    k0_src = [np.concatenate([axes, i3, rand(255 - len(axes) - len(i3))]), none, rand(1), rand(2)]
    k0_tgt = [rand(256), none, rand(257), rand(300)]
    P0 = yaw_pose(o + v * np.array([2.0, 3.0, 1.0]), 0.0)
    # keyframe 1: all-negative coordinates under a rotation; rays inside one cell, L = 0, L just below and above max_range,
    # NaN and inf points
    d = unit(rng, 8)
    special = np.concatenate([np.zeros((2, 3)), 0.01 * v * d, MAX_RANGE * (1.0 - 1e-12) * d, MAX_RANGE * (1.0 + 1e-12) * d,
                              [[np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [-np.inf, 0.0, np.nan]]])
    k1_src = [none, np.concatenate([special, rand(100)]), none, rand(40, 3.0)]
    k1_tgt = [none, rand(300), none, none]
    P1 = yaw_pose([-63.3, -47.1, -22.2], 2.8)
    # keyframe 2, far from the others: three returns make a voxel, a thousand rays pass through it
    through = np.tile(np.array([[10.3, 0.0, 0.0]]) * v, (1000, 1))
    k2_src = [np.array([[5.1, 0.1, 0.1]] * 3) * v, none, none, none]
    k2_tgt = [none, none, through, none]
    P2 = yaw_pose(o + v * np.array([400.5, 400.5, 0.5]), 0.0)
    # keyframe 3: so close to the grid's edge that rays along +x end beyond it (it adds nothing to the map: an overflow
    # keyframe of the build), the others stay inside
    k3_src = [none, none, rand(64, 10.0 * v), none]
    k3_tgt = [np.array([[5.0, 0.0, 0.0], [-5.0, 0.3, 0.2], [0.5, 4.0, 0.0]]) * v, none, none, none]
    P3 = yaw_pose(o + v * np.array([float(1 << 20) - 2.5, 0.5, 0.5]), 0.0)
    return np.array([P0, P1, P2, P3]), [[k0_src, k0_tgt], [k1_src, k1_tgt], [k2_src, k2_tgt], [k3_src, k3_tgt]]


@pytest.mark.parametrize("voxel,origin", [(1.0, (0.0, 0.0, 0.0)), (0.25, (1.0, -2.0, 0.5))])
def test_the_adversarial_set(hip_module, voxel, origin):
    poses, clouds = adversarial(voxel, origin)
    H, V = built(hip_module, poses, clouds, 0xFF, voxel, origin)
    assert H.closed_map_info()["overflow_keyframes"] == 1
    one = dict(reads=READS[:1])
    info, M = carve_and_compare(H, V, poses, clouds, 0xFF, max_range=MAX_RANGE)
    assert info["skipped_rays"] >= 2 + 8 + 3 + 1 and info["n_rays"] == sum(len(c) for kf in clouds for side in kf for c in side)
    through = int(np.flatnonzero((V.i == np.floor((poses[2][:3, 3] + voxel * np.array([5.1, 0.1, 0.1]) - origin) / voxel)).all(axis=1))[0])
    assert M[through] == 1000 and V.N[through] == 3
    launches = {info["launches"]}
    for cfg in (dict(radius=float("inf")), dict(radius=0.05), dict(end_margin=100.0), dict(end_margin=0.0, radius=0.4)):
        launches.add(carve_and_compare(H, V, poses, clouds, 0xFF, max_range=MAX_RANGE, **one, **cfg)[0]["launches"])
    assert H.closed_map_carve_info()["misses"] > 0
    H.closed_map_carve_configure(max_range=MAX_RANGE, end_margin=100.0)
    assert H.closed_map_carve()["misses"] == 0   # end_margin >= L for every ray
    rays = {}
    for mask in (0x0F, 0xF0, 0x04, 0x40):
        i, _ = carve_and_compare(H, V, poses, clouds, 0xFF, ray_mask=mask, max_range=MAX_RANGE, **one)
        rays[mask] = i["n_rays"]
        launches.add(i["launches"])
    assert rays[0x0F] + rays[0xF0] == info["n_rays"] and rays[0x40] == 257 + 1000 and len(launches) == 1
    H.close()
    # a build of the target side alone: ray_mask 0 is the build's mask, and any other mask still casts its rays
    H, V = built(hip_module, poses, clouds, 0xF0, voxel, origin)
    i, _ = carve_and_compare(H, V, poses, clouds, 0xF0, max_range=MAX_RANGE, **one)
    assert i["n_rays"] == rays[0xF0]
    i, _ = carve_and_compare(H, V, poses, clouds, 0xF0, ray_mask=0x0F, max_range=MAX_RANGE, **one)
    assert i["n_rays"] == rays[0x0F] and i["launches"] in launches
    H.close()


# ---- 3: the real pass, and the same bits -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def static():
    return CS.static_pass()


def test_the_real_pass_and_determinism(hip_module, static):
    poses, clouds = static
    v, cfg = CS.STATIC["voxel"], dict(max_range=CS.STATIC["max_range"])
    H, V = built(hip_module, poses, clouds, CS.MASK, v)
    info, M = carve_and_compare(H, V, poses, clouds, CS.MASK, **cfg)
    assert info["n_rays"] > 100000 and info["misses"] > 0 and info["tested"] > info["misses"]
    again = H.closed_map_carve()
    assert again == info and H.closed_map_misses().tobytes() == M.tobytes()      # a carve replaces the counts: it does not add
    # launches: another size and two other masks
    small = H.closed_map_carve_info()
    for mask in (0x20, 0xFF):
        H.closed_map_carve_configure(ray_mask=mask, **cfg)
        i = H.closed_map_carve()
        assert i["launches"] == info["launches"] and i["n_rays"] == (0 if mask == 0x20 else info["n_rays"])
    H.close()
    other, _ = built(hip_module, poses, clouds, CS.MASK, v, reserve_voxels=64)        # the rows grown inside the build
    other.closed_map_carve_configure(**cfg)
    assert other.closed_map_carve() == small and other.closed_map_misses().tobytes() == M.tobytes()
    for a, b in zip(other.closed_map_read_carved(), (V.centroids(), V.N, M)):
        assert a.tobytes() == b[CN.read_carved(V, M)].tobytes()
    other.close()
    half, Vh = built(hip_module, poses[:4], clouds[:4], CS.MASK, v)
    ih, _ = carve_and_compare(half, Vh, poses[:4], clouds[:4], CS.MASK, reads=READS[:1], **cfg)
    assert ih["launches"] == info["launches"] and ih["n_rays"] < info["n_rays"]
    half.close()


# ---- 4: lifecycle ----------------------------------------------------------------------------------------------------------
def test_lifecycle(hip_module):
    reg = hip_module
    poses, clouds, _, _ = CS.ghost_scene()
    v = CS.GHOST["voxel"]

    def no_counts(H):
        for read in (lambda: H.closed_map_misses(0, 0), lambda: H.closed_map_read_carved()):
            with not_ready(reg):
                read()
        assert H.closed_map_carve_info()["n_rays"] == 0

    H = context(reg, poses, clouds, keep=range(4), voxel=v, cloud_mask=CS.MASK)
    no_counts(H)
    with not_ready(reg):
        H.closed_map_carve()                      # before a build
    H.closed_map_build(2, poses[:4])
    no_counts(H)
    H.closed_map_carve_configure(max_range=12.0)
    info = H.closed_map_carve()
    M = H.closed_map_misses()
    V = CN.build_map(poses[:4], clouds[:4], CS.MASK, v)
    assert M.tobytes() == CN.carve(V, poses[:4], clouds[:4], CS.MASK, max_range=12.0)[0].tobytes()
    nv = len(M)
    with invalid(reg):
        H.closed_map_misses(0, nv + 1)
    with invalid(reg):
        H.closed_map_misses(nv + 1, 0)
    # a refused configuration leaves the counts readable and equal
    for over in (dict(max_range=0.0), dict(max_range=-1.0), dict(max_range=np.inf), dict(max_range=np.nan), dict(end_margin=-0.5),
                 dict(end_margin=np.inf), dict(end_margin=np.nan), dict(radius=0.0), dict(radius=-1.0), dict(radius=np.nan),
                 dict(ray_mask=0x100), dict(ray_mask=-1)):
        with invalid(reg):
            H.closed_map_carve_configure(**over)
    assert H.closed_map_misses().tobytes() == M.tobytes() and H.closed_map_carve_info() == info
    with invalid(reg):
        H.closed_map_build(2, poses[:3])         # a refused build leaves the closed map and its counts
    assert H.closed_map_misses().tobytes() == M.tobytes()
    # keyframes added after the build cast no rays
    for k in (4, 5):
        assert H.place_add_scan(DUMMY, np.eye(4), k) == k
        H.place_set_keyframe_clouds(k, *clouds[k])
    assert H.closed_map_carve() == info and H.closed_map_misses().tobytes() == M.tobytes()
    # a rebuild drops the counts, and so does everything that empties the closed map; a carve configuration drops the counts alone
    H.closed_map_build(2, poses)
    no_counts(H)
    assert H.closed_map_carve()["n_keyframes"] == 6
    H.closed_map_carve_configure(max_range=12.0, radius=np.inf)
    no_counts(H)
    assert H.closed_map_info()["n_keyframes"] == 6 and len(H.closed_map_read()[1]) > 0
    for drop in (lambda: H.closed_map_configure(voxel=v, cloud_mask=CS.MASK), lambda: H.place_configure(enabled=1, exclude_recent=8),
                 lambda: H.loop_configure(enabled=1), lambda: H.odometry_reset(None, TC.odom_cfg(reg))):
        if H.place_info()["n_keyframes"] == 0:
            for k in range(6):
                assert H.place_add_scan(DUMMY, np.eye(4), k) == k
                H.place_set_keyframe_clouds(k, *clouds[k])
        H.closed_map_build(2, poses)
        H.closed_map_carve()
        H.closed_map_misses()
        drop()
        no_counts(H)
        with not_ready(reg):
            H.closed_map_carve()
    # the configuration persisted across the reset (radius inf, max_range 12)
    for k in range(6):
        assert H.place_add_scan(DUMMY, np.eye(4), k) == k
        H.place_set_keyframe_clouds(k, *clouds[k])
    H.closed_map_build(2, poses)
    V = CN.build_map(poses, clouds, CS.MASK, v)
    Mw, want = CN.carve(V, poses, clouds, CS.MASK, max_range=12.0, radius=np.inf)
    got = H.closed_map_carve()
    assert got["misses"] == want["misses"] and H.closed_map_misses().tobytes() == Mw.tobytes()
    assert want["misses"] != CN.carve(V, poses, clouds, CS.MASK, max_range=12.0)[1]["misses"]
    H.close()
    # nranks > 1: every carve call is refused
    H = reg.HipRegistration()
    H.comm_init_callback(0, 2, lambda dev, count, stream: 0)
    for call in (H.closed_map_carve_configure, H.closed_map_carve, H.closed_map_carve_info, lambda: H.closed_map_misses(0, 0),
                 H.closed_map_read_carved):
        with invalid(reg):
            call()
    H.close()


# ---- 5: undisturbed --------------------------------------------------------------------------------------------------------
def test_odometry_and_the_closed_map_are_undisturbed_by_carves(hip_module):
    reg = hip_module
    seq = G.sequence(7, seed=3)[0]
    seen = []

    def carves_between_frames(f, H):
        if f in (2, 4, 6):
            H.closed_map_build(0)
            H.closed_map_carve_configure(max_range=30.0)
            seen.append(H.closed_map_carve())
            H.closed_map_misses()
            H.closed_map_read_carved()

    def closed_map_bytes(H):
        H.closed_map_build(1)
        cen, cnt = H.closed_map_read()
        bc, bn = H.closed_map_read_box([-50.0] * 3, [50.0] * 3, 2)
        return bits(cen) + cnt.tobytes() + bits(bc) + bn.tobytes() + bits(H.closed_map_poses())

    Hoff, off = TC.odom_run(reg, seq)
    Hon, on = TC.odom_run(reg, seq, hook=carves_between_frames)
    assert len(seen) == 3 and seen[-1]["n_rays"] > 0 and seen[-1]["steps"] > 0
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
    ka, kb = Hon.place_read_keyframes(), Hoff.place_read_keyframes()
    for k in ka:
        assert np.asarray(ka[k]).tobytes() == np.asarray(kb[k]).tobytes(), k
    assert Hon.place_loops() == Hoff.place_loops()
    ca, cb = Hon.loop_constraints(), Hoff.loop_constraints()
    assert len(ca) == len(cb)
    for a, b in zip(ca, cb):
        for k in b:
            if k in ("coarse", "fine"):
                assert all(np.asarray(a[k][s]).tobytes() == np.asarray(b[k][s]).tobytes() for s in b[k] if s != "host_wait_us"), k
            else:
                assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    assert bits(Hon.graph_poses()) == bits(Hoff.graph_poses())
    before = closed_map_bytes(Hon)
    Hon.closed_map_carve()
    Hon.closed_map_read_carved()
    cen, cnt = Hon.closed_map_read()
    bc, bn = Hon.closed_map_read_box([-50.0] * 3, [50.0] * 3, 2)
    assert bits(cen) + cnt.tobytes() + bits(bc) + bn.tobytes() + bits(Hon.closed_map_poses()) == before == closed_map_bytes(Hoff)
    Hon.close(); Hoff.close()
