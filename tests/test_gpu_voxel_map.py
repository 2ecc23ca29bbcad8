"""-m gpu: the merged voxel map of the odometry frame against its int64 restatement
(tests/voxel_map_np.py) bit for bit -- ids, counts, centroids after every frame --, and against a context without it (the
odometry, the append map and the registered scan must not move by a bit).

The restatement's input is the device's registered scan of each adding frame (tloam_registered_scan: proved equal to the
oracle's pc_transform in tests/test_gpu_mapping.py).  Sequence and feature settings are those of tests/test_gpu_mapping.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import voxel_map_np as V  # noqa: E402
from tloam_amd import map_io, synth_hdl64 as G  # noqa: E402

pytestmark = pytest.mark.gpu

FEATURE = dict(radius=0.5, cvr_submap=0.05)
N_FRAMES = 8


def odom_cfg(reg):
    return reg.default_odom_config(**{f"feature__{k}": v for k, v in FEATURE.items()})


def run(reg, scans, vmap=None, mapping=False, init=None):
    """a new context through the scans; per frame: pose, stats, registered scan, voxel map info / contents, append map info"""
    H = reg.HipRegistration()
    if mapping:
        H.map_configure(reg.default_map_config(enabled=1))
    if vmap is not None:
        H.voxel_map_configure(reg.default_voxel_map_config(enabled=1, **vmap))
    H.odometry_reset(init, odom_cfg(reg))
    res = []
    for f, xyz in enumerate(scans):
        rc, T, st = H.odometry_frame(xyz)
        assert rc in (0, -7), (f, rc)
        r = {"rc": rc, "pose": T, "stats": st, "reg": H.registered_scan()}
        if vmap is not None:
            r["vinfo"] = H.voxel_map_info()
            r["vmap"] = H.voxel_map_read()
        if mapping:
            r["info"] = H.map_info()
            r["span"] = H.map_read(r["info"]["last_first"], r["info"]["last_count"])
        res.append(r)
    return H, res


def restated(res, voxel=1.0, origin=(0.0, 0.0, 0.0)):
    """the restatement after every frame, fed with the registered scans of the adding frames"""
    M = V.VoxelMapNP(voxel, origin)
    out = []
    for f, r in enumerate(res):
        if f > 0 and r["rc"] in (0, -7):
            M.add_frame(r["reg"])
        out.append((M.info(), M.centroids(), M.N.copy()))
    return M, out


def same_contents(got, want_info, want_c, want_n):
    info = dict(got["vinfo"])
    cap = info.pop("capacity_voxels")
    w = dict(want_info)
    w.pop("capacity_voxels")
    assert info == w
    assert cap >= info["n_voxels"]
    c, n = got["vmap"]
    assert c.shape == want_c.shape and c.tobytes() == want_c.tobytes()
    assert n.tobytes() == want_n.tobytes()


@pytest.fixture(scope="module")
def seq3():
    return G.sequence(N_FRAMES, seed=3)[0]


@pytest.fixture(scope="module")
def runs(hip_module, seq3):
    """the same sequence: voxel map alone, voxel map + append map, append map alone, neither, and the voxel map alone again"""
    reg = hip_module
    out = {}
    for name, vmap, mapping in (("v", {}, False), ("vm", {}, True), ("m", None, True), ("off", None, False), ("v2", {}, False)):
        H, res = run(reg, seq3, vmap, mapping)
        H.close()
        out[name] = res
    return out


def test_contents_equal_the_restatement_after_every_frame(runs):
    res = runs["v"]
    M, want = restated(res)
    assert res[0]["vinfo"]["n_voxels"] == 0 and res[0]["vinfo"]["n_frames"] == 0   # the first frame adds nothing
    for f in range(N_FRAMES):
        same_contents(res[f], *want[f])
    assert M.n_frames == N_FRAMES - 1 and M.overflow_frames == 0
    print("voxel map:", [w[0]["last_new"] for w in want[1:]], "new voxels per frame,", len(M.keys), "in all,",
          int(M.N.sum()), "returns")


def test_odometry_append_map_and_scan_are_undisturbed(runs):
    for on, off, extra in ((runs["v"], runs["off"], 64), (runs["vm"], runs["m"], 64)):
        for f, (a, b) in enumerate(zip(on, off)):
            assert a["pose"].tobytes() == b["pose"].tobytes(), f
            assert a["reg"].tobytes() == b["reg"].tobytes(), f
            sa, sb = a["stats"], b["stats"]
            for key in sb:
                if key not in ("match", "d2h_bytes"):
                    assert sa[key] == sb[key], (f, key)
            for key, v in sb["match"].items():
                if key != "host_wait_us":   # (a time)
                    assert np.asarray(sa["match"][key]).tobytes() == np.asarray(v).tobytes(), (f, key)
            assert sa["d2h_bytes"] == sb["d2h_bytes"] + (extra if f else 0), f   # the stage's pinned segment
            if f:
                assert sa["host_syncs"] == 4, f
            if "info" in b:
                assert a["info"] == b["info"] and a["span"].tobytes() == b["span"].tobytes(), f


def test_runs_and_contexts_give_the_same_bits(runs):
    for other in ("v2", "vm"):   # a second context; the append map's transform as input instead of the stage's own
        for f, (a, b) in enumerate(zip(runs["v"], runs[other])):
            assert a["vinfo"] == b["vinfo"], (other, f)
            for x, y in zip(a["vmap"], b["vmap"]):
                assert x.tobytes() == y.tobytes(), (other, f)


def test_skipped_and_failing_frames_change_nothing(hip_module, seq3, runs):
    reg = hip_module
    ref = runs["v"]
    H = reg.HipRegistration()
    H.voxel_map_configure(reg.default_voxel_map_config(enabled=1))
    H.odometry_reset(None, odom_cfg(reg))
    for f in range(3):
        rc, _, _ = H.odometry_frame(seq3[f])
        assert rc in (0, -7)
    info = H.voxel_map_info()
    c0, n0 = H.voxel_map_read()
    box0 = H.voxel_map_read_box((-30, -30, -5), (30, 30, 5), 2)
    assert info == ref[2]["vinfo"]

    def unchanged():
        assert H.voxel_map_info() == info
        c, n = H.voxel_map_read()
        assert c.tobytes() == c0.tobytes() and n.tobytes() == n0.tobytes()
        b = H.voxel_map_read_box((-30, -30, -5), (30, 30, 5), 2)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(b, box0))

    rng = np.random.default_rng(3)
    for bad in (np.zeros((0, 3)), rng.uniform(-5, 5, (5000, 3)).astype(np.float32).astype(np.float64)):
        rc, _, _ = H.odometry_frame(bad)   # TLOAM_E_TOO_FEW_POINTS: skipped
        assert rc == -2
        unchanged()
    pose = np.zeros(16)
    assert H.L.tloam_odometry_frame(H.h, None, 1 << 29, reg._dp(pose), None) == -1   # refused: fails before any stage
    unchanged()
    rc, T, _ = H.odometry_frame(seq3[3])
    assert rc in (0, -7) and T.tobytes() == ref[3]["pose"].tobytes()
    assert H.voxel_map_info() == ref[3]["vinfo"]
    for x, y in zip(H.voxel_map_read(), ref[3]["vmap"]):
        assert x.tobytes() == y.tobytes()
    # a reset empties the map and keeps the configuration; configure empties it too
    H.odometry_reset(None, odom_cfg(reg))
    assert H.voxel_map_info()["n_voxels"] == 0 and H.voxel_map_info()["n_frames"] == 0
    for f in range(2):
        rc, T, _ = H.odometry_frame(seq3[f])
        assert rc in (0, -7)
    M = V.VoxelMapNP()
    M.add_frame(H.registered_scan())
    c, n = H.voxel_map_read()
    assert c.tobytes() == M.centroids().tobytes() and n.tobytes() == M.N.tobytes()
    H.voxel_map_configure(reg.default_voxel_map_config(enabled=1, voxel=0.5, origin=(0.25, -0.5, 1.0)))
    assert H.voxel_map_info()["n_voxels"] == 0
    rc, T, _ = H.odometry_frame(seq3[2])
    assert rc in (0, -7)
    M = V.VoxelMapNP(0.5, (0.25, -0.5, 1.0))
    M.add_frame(H.registered_scan())
    c, n = H.voxel_map_read()
    assert c.tobytes() == M.centroids().tobytes() and n.tobytes() == M.N.tobytes()
    # off: the device memory is released, the calls report an empty map
    H.voxel_map_configure(reg.default_voxel_map_config(enabled=0))
    assert H.voxel_map_info()["capacity_voxels"] == 0 and H.voxel_map_info()["n_voxels"] == 0
    H.close()


def test_growth_rehashes_and_keeps_ids(hip_module, seq3, runs):
    reg = hip_module
    H = reg.HipRegistration()
    H.voxel_map_configure(reg.default_voxel_map_config(enabled=1, reserve_voxels=64))
    assert H.voxel_map_info()["capacity_voxels"] == 64
    H.odometry_reset(None, odom_cfg(reg))
    caps = []
    for f, xyz in enumerate(seq3):
        rc, _, _ = H.odometry_frame(xyz)
        assert rc in (0, -7), f
        caps.append(H.voxel_map_info()["capacity_voxels"])
        a, b = H.voxel_map_info(), runs["v"][f]["vinfo"]
        assert {k: v for k, v in a.items() if k != "capacity_voxels"} == {k: v for k, v in b.items() if k != "capacity_voxels"}
        for x, y in zip(H.voxel_map_read(), runs["v"][f]["vmap"]):
            assert x.tobytes() == y.tobytes(), f
    grows = [f for f, (x, y) in enumerate(zip([64] + caps, caps)) if y > x]
    print("capacity after each frame:", caps)
    # (room for one new voxel per return: the first later frame grows past the scan, a later one rehashes a non-empty map)
    assert len(grows) >= 2 and grows[-1] >= 2
    H.close()


def test_read_box_equals_the_restatement(hip_module, seq3, runs, tmp_path):
    reg = hip_module
    res = runs["v"]
    M, _ = restated(res)
    H = reg.HipRegistration()
    H.voxel_map_configure(reg.default_voxel_map_config(enabled=1))
    H.odometry_reset(None, odom_cfg(reg))
    for xyz in seq3:
        rc, _, _ = H.odometry_frame(xyz)
        assert rc in (0, -7)
    cen, cnt = M.centroids(), M.N
    lo_all, hi_all = cen.min(axis=0), cen.max(axis=0)
    boxes = [(lo_all, hi_all), ((-10, -10, -3), (10, 10, 3)), ((0, -50, -50), (50, 0, 50)),
             (cen[5], cen[5]), ((1e6, 1e6, 1e6), (1e6 + 1, 1e6 + 1, 1e6 + 1)), ((5, 5, 5), (-5, -5, -5))]
    for lo, hi in boxes:
        for mc in (1, 2, 50):
            ids = M.box(lo, hi, mc)
            c, n = H.voxel_map_read_box(lo, hi, mc)
            assert c.tobytes() == cen[ids].tobytes() and n.tobytes() == cnt[ids].tobytes(), (lo, hi, mc)
    assert len(M.box(lo_all, hi_all, 1)) == len(cen) and len(M.box(*boxes[1], 2)) > 10
    # too small a capacity: the size is written, nothing is copied
    lo, hi = (np.asarray(boxes[1][0], np.float64), np.asarray(boxes[1][1], np.float64))
    want = len(M.box(lo, hi, 1))
    n = ctypes.c_size_t(0)
    out = np.full((4, 3), 7.0)
    cnt_out = np.full(4, 7, np.int64)
    assert H.L.tloam_voxel_map_read_box(H.h, reg._dp(lo), reg._dp(hi), 1, 3, ctypes.byref(n), reg._dp(out),
                                        reg._lp(cnt_out)) == -1
    assert n.value == want and (out == 7.0).all() and (cnt_out == 7).all()
    # whole reads: ranges, NULL outputs, and the PCD export
    nv = len(cen)
    assert H.L.tloam_voxel_map_read(H.h, nv + 1, 0, None, None) == -1
    assert H.L.tloam_voxel_map_read(H.h, nv - 1, 2, None, None) == -1
    assert H.L.tloam_voxel_map_read(H.h, nv, 0, None, None) == 0
    c_part, n_part = H.voxel_map_read(7, 20)
    assert c_part.tobytes() == cen[7:27].tobytes() and n_part.tobytes() == cnt[7:27].tobytes()
    only_n = np.zeros(nv, np.int64)
    assert H.L.tloam_voxel_map_read(H.h, 0, nv, None, reg._lp(only_n)) == 0 and only_n.tobytes() == cnt.tobytes()
    path = str(tmp_path / "vmap.pcd")
    c, n = H.voxel_map_read()
    map_io.write_voxel_pcd(path, c, n)
    c2, n2 = map_io.read_voxel_pcd(path)
    assert c2.tobytes() == cen.tobytes() and n2.tobytes() == cnt.tobytes()
    H.close()


def test_overflow_adds_nothing_and_leaves_the_pose(hip_module, seq3):
    """an init pose 2^20 + 1000 m out: every later frame's returns are beyond the grid"""
    reg = hip_module
    init = np.eye(4)
    init[:3, 3] = ((1 << 20) + 1000.0, 0.0, 0.0)
    Hon, on = run(reg, seq3[:4], {}, init=init)
    Hoff, off = run(reg, seq3[:4], None, init=init)
    Hon.close()
    Hoff.close()
    for f, (a, b) in enumerate(zip(on, off)):
        assert a["pose"].tobytes() == b["pose"].tobytes(), f
        assert a["stats"]["host_syncs"] == b["stats"]["host_syncs"], f
    info = on[-1]["vinfo"]
    assert info["overflow_frames"] == 3 and info["n_voxels"] == 0 and info["n_frames"] == 0 and info["n_points"] == 0
    # the same run with the origin moved out with it: every frame adds
    Hn, near = run(reg, seq3[:4], {"origin": ((1 << 20) + 1000.0, 0.0, 0.0)}, init=init)
    Hn.close()
    assert near[-1]["vinfo"]["overflow_frames"] == 0 and near[-1]["vinfo"]["n_frames"] == 3
    M, want = restated(near, 1.0, ((1 << 20) + 1000.0, 0.0, 0.0))
    same_contents(near[-1], *want[-1])


def test_invalid_configurations_are_refused(hip_module):
    reg = hip_module
    H = reg.HipRegistration()
    nan, inf = float("nan"), float("inf")
    for over in (dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=nan), dict(voxel=inf), dict(origin=(0.0, nan, 0.0)),
                 dict(origin=(inf, 0.0, 0.0)), dict(origin=(0.0, 0.0, -inf)), dict(reserve_voxels=-1)):
        with pytest.raises(reg.TloamHipError, match="TLOAM_E_INVALID"):
            H.voxel_map_configure(reg.default_voxel_map_config(enabled=1, **over))
        assert H.voxel_map_info()["capacity_voxels"] == 0
    n = ctypes.c_size_t(5)
    lo = np.zeros(3)
    assert H.L.tloam_voxel_map_read_box(H.h, None, reg._dp(lo), 1, 0, ctypes.byref(n), None, None) == -1
    assert H.L.tloam_voxel_map_read_box(H.h, reg._dp(lo), reg._dp(lo), 1, 0, None, None, None) == -1
    assert H.L.tloam_voxel_map_read(H.h, 0, 1, None, None) == -1   # an empty map has no voxel 0
    assert H.L.tloam_voxel_map_get_info(H.h, None) == -1
    H.close()


def test_voxel_count_is_below_the_append_map(runs):
    vinfo, info = runs["vm"][-1]["vinfo"], runs["vm"][-1]["info"]
    print(f"after {N_FRAMES} frames: voxel map {vinfo['n_voxels']} voxels ({vinfo['n_voxels'] * 40} B of rows) over "
          f"{vinfo['n_points']} returns; append map {info['n_points']} points ({info['n_points'] * 24} B)")
    assert 0 < vinfo["n_voxels"] < info["n_points"]
    assert vinfo["n_points"] == sum(int(np.isfinite(r["reg"]).all(axis=1).sum()) for r in runs["vm"][1:])
