"""-m gpu: the odometry frame's global map and registered scan -- FrontEnd::spinOnce's /raw_cloud
(front_end.cpp:84-86) and updateSubmap's mapping branch (:269-274) on the device -- against the oracle's pc_transform /
pc_voxel_down_sample bit for bit, and against a mapping-off context (the odometry must not move by a bit).

Sequences and feature settings are those of tests/test_gpu_odometry_frame.py: the ray-cast street has nothing round, so the
PCA radius is widened to 0.5 m and cvr_submap lowered to 0.05 (sphere lists of ten points or more)."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from oracle import binding as ob  # noqa: E402
from tloam_amd import map_io, replay, synth_hdl64 as G  # noqa: E402

pytestmark = pytest.mark.gpu

FEATURE = dict(radius=0.5, cvr_submap=0.05)
N_FRAMES = 8


def odom_cfg(reg):
    return reg.default_odom_config(**{f"feature__{k}": v for k, v in FEATURE.items()})


def expected_span(T, raw, voxel=1.0):
    """global_map += raw.Transform(T).VoxelDownSample(voxel), non-finite returns left out"""
    xf = ob.pc_transform(T, raw[np.isfinite(raw).all(axis=1)])
    return ob.pc_voxel_down_sample(xf, voxel)


def run(reg, scans, mapping, init=None, map_over=None):
    H = reg.HipRegistration()
    if mapping:
        H.map_configure(reg.default_map_config(enabled=1, **(map_over or {})))
    H.odometry_reset(init, odom_cfg(reg))
    res = []
    for f, xyz in enumerate(scans):
        rc, T, st = H.odometry_frame(xyz)
        assert rc in (0, -7), (f, rc)
        r = {"pose": T, "stats": st, "reg": H.registered_scan(), "targets": [H.get_target(k) for k in range(4)]}
        if f:
            r["corr"] = [H.get_correspondences(k) for k in range(4)]
        if mapping:
            r["info"] = H.map_info()
            r["span"] = H.map_read(r["info"]["last_first"], r["info"]["last_count"])
        res.append(r)
    return H, res


@pytest.fixture(scope="module")
def seq3():
    return G.sequence(N_FRAMES, seed=3)[0]


@pytest.fixture(scope="module")
def both(hip_module, seq3):
    """the same sequence in a mapping-on and a mapping-off context"""
    Hon, on = run(hip_module, seq3, True)
    full = Hon.map_read()
    Hon.close()
    Hoff, off = run(hip_module, seq3, False)
    Hoff.close()
    return on, off, full


def test_map_contents_are_the_oracle_bit_for_bit(seq3, both):
    on, _, full = both
    assert on[0]["info"]["n_points"] == 0 and on[0]["info"]["n_frames"] == 0   # the first frame returns at :304
    spans, at = [], 0
    for f in range(1, N_FRAMES):
        info, span = on[f]["info"], on[f]["span"]
        want = expected_span(on[f]["pose"], seq3[f])
        assert info["last_first"] == at and info["last_count"] == len(want), f
        assert span.shape == want.shape and span.tobytes() == want.tobytes(), f
        at += len(want)
        assert info["n_points"] == at and info["n_frames"] == f and info["overflow_frames"] == 0, f
        spans.append(want)
    assert full.tobytes() == np.concatenate(spans).tobytes()
    assert np.isfinite(full).all()
    print("global map:", [len(s) for s in spans], "points per frame,", at, "in all")


def test_odometry_is_undisturbed_by_the_map(both):
    on, off, _ = both
    for f, (a, b) in enumerate(zip(on, off)):
        assert a["pose"].tobytes() == b["pose"].tobytes(), f
        for k in range(4):
            assert a["targets"][k].tobytes() == b["targets"][k].tobytes(), (f, k)
        sa, sb = a["stats"], b["stats"]
        for key in sb:
            if key not in ("match", "d2h_bytes"):
                assert sa[key] == sb[key], (f, key)
        for key, v in sb["match"].items():
            if key == "host_wait_us":   # (a time)
                continue
            assert np.asarray(sa["match"][key]).tobytes() == np.asarray(v).tobytes(), (f, key)
        if f == 0:
            assert sa["d2h_bytes"] == sb["d2h_bytes"]
            continue
        assert sa["host_syncs"] == 4 and sa["h2d_bytes"] == sb["h2d_bytes"], f
        assert sa["d2h_bytes"] == sb["d2h_bytes"] + 64, f   # the map stage's pinned segment
        for k in range(4):
            for key in ("idx", "a", "b", "d", "w", "cost"):
                assert a["corr"][k][key].tobytes() == b["corr"][k][key].tobytes(), (f, k, key)


def test_registered_scan_is_the_transformed_raw_scan(hip_module, seq3, both):
    on, off, _ = both
    for f in range(N_FRAMES):
        T = np.eye(4) if f == 0 else on[f]["pose"]
        want = ob.pc_transform(T, seq3[f])
        assert on[f]["reg"].tobytes() == want.tobytes(), f
        assert off[f]["reg"].tobytes() == want.tobytes(), f
    # under a non-identity init pose the first frame's lidar_odom_pose is still Identity (front_end.hpp:106)
    init = np.eye(4)
    c, s = np.cos(0.05), np.sin(0.05)
    init[:2, :2] = [[c, -s], [s, c]]
    init[:3, 3] = (0.4, -0.3, 0.1)
    reg = hip_module
    for mapping in (True, False):
        H = reg.HipRegistration()
        if mapping:
            H.map_configure(reg.default_map_config(enabled=1))
        with pytest.raises(reg.TloamHipError, match="TLOAM_E_NOT_READY"):   # before the reset
            H.registered_scan()
        H.odometry_reset(init, odom_cfg(reg))
        with pytest.raises(reg.TloamHipError, match="TLOAM_E_NOT_READY"):   # before the first frame
            H.registered_scan()
        n = ctypes.c_size_t(0)
        assert H.L.tloam_registered_scan(H.h, 0, ctypes.byref(n), None) == -6
        for f in range(3):
            rc, T, _ = H.odometry_frame(seq3[f])
            assert rc in (0, -7), f
            if f == 0:
                assert np.array_equal(T, init)
            want = ob.pc_transform(np.eye(4) if f == 0 else T, seq3[f])
            # too small a capacity: the size is written, nothing is copied
            assert H.L.tloam_registered_scan(H.h, 5, ctypes.byref(n), None) == -1 and n.value == len(seq3[f])
            assert H.registered_scan().tobytes() == want.tobytes(), (mapping, f)
        # another upload into the segmentation's input: the scan is gone unless the map stage transformed it
        H.segment(seq3[3], odom_cfg(reg).seg)
        if mapping:
            assert H.registered_scan().tobytes() == want.tobytes()
        else:
            with pytest.raises(reg.TloamHipError, match="TLOAM_E_NOT_READY"):
                H.registered_scan()
        H.close()


def test_map_growth_keeps_the_contents(hip_module, seq3):
    reg = hip_module
    small = reg.HipRegistration()
    small.map_configure(reg.default_map_config(enabled=1, voxel=0.25, reserve_points=3000))
    assert small.map_info()["capacity_points"] >= 3000
    big = reg.HipRegistration()
    big.map_configure(reg.default_map_config(enabled=1, voxel=0.25, reserve_points=1 << 23))
    caps = []
    for H in (small, big):
        H.odometry_reset(None, odom_cfg(reg))
    for f, xyz in enumerate(seq3):
        for H in (small, big):
            rc, _, st = H.odometry_frame(xyz)
            assert rc in (0, -7), f
        caps.append(small.map_info()["capacity_points"])
        a, b = small.map_info(), big.map_info()
        assert {k: v for k, v in a.items() if k != "capacity_points"} == {k: v for k, v in b.items() if k != "capacity_points"}
    grows = sum(1 for x, y in zip(caps, caps[1:]) if y > x)
    print("capacity after each frame:", caps)
    assert grows >= 2 and big.map_info()["capacity_points"] >= 1 << 23
    assert small.map_read().tobytes() == big.map_read().tobytes()
    small.close()
    big.close()


def test_skips_resets_ranges_and_overflow(hip_module, seq3, both):
    reg = hip_module
    on, off, full = both
    H = reg.HipRegistration()
    with pytest.raises(reg.TloamHipError, match="TLOAM_E_INVALID"):
        H.map_configure(reg.default_map_config(enabled=1, voxel=0.0))
    with pytest.raises(reg.TloamHipError, match="TLOAM_E_INVALID"):
        H.map_configure(reg.default_map_config(enabled=1, voxel=-1.0))
    with pytest.raises(reg.TloamHipError, match="TLOAM_E_INVALID"):
        H.map_configure(reg.default_map_config(enabled=1, reserve_points=-1))
    H.map_configure(reg.default_map_config(enabled=1))
    H.odometry_reset(None, odom_cfg(reg))
    for f in range(3):
        rc, T, _ = H.odometry_frame(seq3[f])
        assert rc in (0, -7)
    info = H.map_info()
    assert info == on[2]["info"]
    # a skipped frame appends nothing and changes nothing
    rng = np.random.default_rng(3)
    for bad in (np.zeros((0, 3)), rng.uniform(-5, 5, (5000, 3)).astype(np.float32).astype(np.float64)):
        rc, _, _ = H.odometry_frame(bad)
        assert rc == -2
        assert H.map_info() == info
    rc, T, _ = H.odometry_frame(seq3[3])
    assert rc in (0, -7) and T.tobytes() == on[3]["pose"].tobytes()
    assert H.map_info() == on[3]["info"]
    assert H.map_read().tobytes() == full[: on[3]["info"]["n_points"]].tobytes()
    # ranges
    n = H.map_info()["n_points"]
    out = np.zeros((4, 3))
    dp = reg._dp(out)
    assert H.L.tloam_map_read(H.h, n + 1, 0, dp) == -1
    assert H.L.tloam_map_read(H.h, n - 1, 2, dp) == -1
    assert H.L.tloam_map_read(H.h, 0, n + 1, dp) == -1
    assert H.L.tloam_map_read(H.h, n, 0, dp) == 0
    assert len(H.map_read(n)) == 0
    # a reset empties the map and keeps the configuration (the poses after it are not those of `on`: the segmentation node
    # is not reset, and seeds its first frame differently)
    cap = H.map_info()["capacity_points"]
    H.odometry_reset(None, odom_cfg(reg))
    assert H.map_info() == dict(n_points=0, n_frames=0, last_first=0, last_count=0, capacity_points=cap, overflow_frames=0)
    for f in range(2):
        rc, T, _ = H.odometry_frame(seq3[f])
        assert rc in (0, -7)
    want = expected_span(T, seq3[1])
    assert H.map_info() == dict(n_points=len(want), n_frames=1, last_first=0, last_count=len(want), capacity_points=cap,
                                overflow_frames=0)
    assert H.map_read().tobytes() == want.tobytes()
    # configure between frames: the map starts again, the odometry goes on
    H.map_configure(reg.default_map_config(enabled=1, voxel=2.0))
    assert H.map_info()["n_points"] == 0
    rc, T, _ = H.odometry_frame(seq3[2])
    assert rc in (0, -7)
    assert H.map_read().tobytes() == expected_span(T, seq3[2], 2.0).tobytes()
    H.close()
    # a voxel so small that the grid's 2^21 cells per axis do not cover a scan: nothing appended, the pose unaffected
    H = reg.HipRegistration()
    H.map_configure(reg.default_map_config(enabled=1, voxel=1e-5))
    H.odometry_reset(None, odom_cfg(reg))
    for f in range(3):
        rc, T, st = H.odometry_frame(seq3[f])
        assert rc in (0, -7) and T.tobytes() == off[f]["pose"].tobytes(), f
        assert st["host_syncs"] == off[f]["stats"]["host_syncs"], f
    info = H.map_info()
    assert info["overflow_frames"] == 2 and info["n_points"] == 0 and info["n_frames"] == 0
    H.close()


def test_non_finite_returns_stay_out_of_the_map(hip_module):
    """the segmentation drops non-finite returns (removeClosedPointCloud): the frame accepts such a scan, the map leaves them out"""
    reg = hip_module
    scans = G.sequence(3, seed=3, nan_inf=60)[0]
    assert all((~np.isfinite(s).all(axis=1)).sum() == 60 for s in scans)
    H = reg.HipRegistration()
    H.map_configure(reg.default_map_config(enabled=1))
    H.odometry_reset(None, odom_cfg(reg))
    for f, xyz in enumerate(scans):
        rc, T, _ = H.odometry_frame(xyz)
        assert rc in (0, -7), f
        if f:
            info = H.map_info()
            span = H.map_read(info["last_first"], info["last_count"])
            assert span.tobytes() == expected_span(T, xyz).tobytes(), f
        got = H.registered_scan()
        ok = np.isfinite(xyz).all(axis=1)
        want = ob.pc_transform(np.eye(4) if f == 0 else T, xyz)
        assert got[ok].tobytes() == want[ok].tobytes() and not np.isfinite(got[~ok]).all(axis=1).any(), f
    assert np.isfinite(H.map_read()).all()
    H.close()


def test_replay_builds_the_same_map(hip_module, seq3, both, tmp_path):
    on, _, full = both
    H = hip_module.HipRegistration()
    path = str(tmp_path / "map.pcd")
    poses, stats = replay.replay_device(H, seq3, odom_cfg=odom_cfg(hip_module),
                                        map_cfg=hip_module.default_map_config(enabled=1), out_map=path)
    H.close()
    assert stats["skipped"] == [] and stats["map"] == on[-1]["info"]
    for f, T in enumerate(poses):
        assert T.tobytes() == on[f]["pose"].tobytes(), f
    assert map_io.read_pcd(path).tobytes() == full.tobytes()


@pytest.mark.parametrize("voxel", (3.0, 8.0))
def test_crowded_voxels_are_the_oracle_bit_for_bit(hip_module, seq3, voxel):
    """coarse grids put thousands of returns into one voxel: members sorted in LDS (up to 8192), or picked out of the scan in
    index order (more)"""
    reg = hip_module
    H = reg.HipRegistration()
    H.map_configure(reg.default_map_config(enabled=1, voxel=voxel))
    H.odometry_reset(None, odom_cfg(reg))
    for f in range(3):
        rc, T, _ = H.odometry_frame(seq3[f])
        assert rc in (0, -7), f
        if f:
            info = H.map_info()
            span = H.map_read(info["last_first"], info["last_count"])
            assert span.tobytes() == expected_span(T, seq3[f], voxel).tobytes(), (voxel, f)
    H.close()
