"""-m gpu: the closed map (tl_cmap.hip, tl_api_cmap.hip) against the voxel map's numpy restatement
(tests/voxel_map_np.py, unchanged) fed each adding keyframe's transformed concatenation, keyframes ascending: one line per
keyframe, VoxelMapNP.add_frame(oracle.pc_transform(P_k, concatenation)).  The keyframes are those of section 17's out-and-back
pass (the recipe of tests/test_gpu_graph.py's `ob_context`, rebuilt here)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import graph_np as GN  # noqa: E402
import loop_np as LN  # noqa: E402
import voxel_map_np as VN  # noqa: E402
from oracle import binding as ob_oracle  # noqa: E402
from tloam_amd import synth_graph as SG  # noqa: E402
from tloam_amd import synth_hdl64 as G  # noqa: E402
from tloam_amd import synth_revisit as RV  # noqa: E402

pytestmark = pytest.mark.gpu

FEATURE = dict(radius=0.5, cvr_submap=0.05)
ODOM_PLACE = dict(kf_dist=2.0, exclude_recent=2)
THIN = dict(n_az=600, rings=np.arange(0, 64, 2))
N_OUT, EX, SEED = 16, 8, 1
DRIFT = np.array([0.02, 0.0, 0.0, 0.0, 0.0, 0.005])   # per keyframe step: 0.02 m along the heading, 0.005 rad of yaw
DRIFT_VOXEL = 0.5


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def invalid(reg):
    return pytest.raises(reg.TloamHipError, match="TLOAM_E_INVALID")


def not_ready(reg):
    return pytest.raises(reg.TloamHipError, match="TLOAM_E_NOT_READY")


def odom_cfg(reg):
    return reg.default_odom_config(**{f"feature__{k}": v for k, v in FEATURE.items()})


def kf_lists(H, reg, xyz):
    """a scan's keyframe clouds through the public stage calls (later-frame lists: selections, down-sampled edge / ground)"""
    cfg = odom_cfg(reg)
    S = H.segment(xyz, cfg.seg)
    assert S["status"] == 0
    ground, edge, general = xyz[S["ground"]], xyz[S["edge"]], xyz[S["general"]]
    ps, pm, ss, sm = H.extract_planar_sphere(general, cfg.feature)
    e_ds = H.voxel_down_sample(edge, cfg.edge_down_sample)
    g_ds = H.voxel_down_sample(ground, cfg.submap.ground_down_sample)
    sel = lambda idx: np.ascontiguousarray(general[idx])  # noqa: E731
    return [sel(ps), g_ds, e_ds, sel(ss)], [sel(pm), g_ds, e_ds, sel(sm)]


@pytest.fixture(scope="module")
def ob(hip_module):
    reg = hip_module
    thin, poses, leg = RV.out_and_back(N_OUT, seed=SEED, **THIN)
    full, _, _ = RV.out_and_back(N_OUT, seed=SEED)
    H = reg.HipRegistration()
    lists = [kf_lists(H, reg, xyz) for xyz in full]
    H.close()
    return thin, poses, leg, lists


def ob_context(reg, ob, keep=None):
    thin, poses, _, lists = ob
    H = reg.HipRegistration()
    H.place_configure(enabled=1, exclude_recent=EX)
    H.loop_configure(enabled=1)
    ks = range(len(poses)) if keep is None else keep
    for f, k in enumerate(ks):
        assert H.place_add_scan(thin[k], poses[k], 100 + k) == f
        H.place_set_keyframe_clouds(f, *lists[k])
    return H


@pytest.fixture(scope="module")
def ob_run(hip_module, ob):
    """the pass with its loops verified and its graph optimised"""
    H = ob_context(hip_module, ob)
    assert H.loop_verify_pending() > 0
    H.graph_optimize()
    yield H
    H.close()


def concatenation(clouds, mask):
    """a keyframe's selected clouds end to end in ascending slot order; clouds = [four source, four target]"""
    parts = [np.asarray(clouds[j // 4][j % 4], np.float64).reshape(-1, 3) for j in range(8) if (mask >> j) & 1]
    return np.concatenate(parts) if parts else np.zeros((0, 3))


def restate(poses, clouds, mask=0xF0, voxel=1.0, origin=(0.0, 0.0, 0.0)):
    """the contract -> (the restated map, info as the device reports it)"""
    V = VN.VoxelMapNP(voxel, origin)
    empty = 0
    for P, c in zip(poses, clouds):
        cat = concatenation(c, mask)
        if len(cat) == 0:
            empty += 1
            continue
        V.add_frame(ob_oracle.pc_transform(P, cat))
    info = dict(n_keyframes=len(poses), added_keyframes=len(poses) - empty - V.overflow_frames, empty_keyframes=empty,
                overflow_keyframes=V.overflow_frames, n_voxels=len(V.keys), n_points=int(V.N.sum()))
    return V, info


def same_as_restated(H, info, V, winfo):
    for k, v in winfo.items():
        assert info[k] == v, (k, info[k], v)
    assert H.closed_map_info() == info
    cen, cnt = H.closed_map_read()
    assert cnt.tobytes() == V.N.tobytes()
    assert bits(cen) == bits(V.centroids())


def rows(H):
    cen, cnt = H.closed_map_read()
    return bits(cen) + cnt.tobytes()


# ---- 1: parity, bit for bit ------------------------------------------------------------------------------------------------
PARITY = [  # (pose_source, voxel, origin, mask)
    (1, 1.0, (0.0, 0.0, 0.0), 0xF0),
    (1, 0.25, (0.0, 0.0, 0.0), 0xF0),
    (0, 0.25, (3.3, -1.7, 0.9), 0x0F),
    (0, 1.0, (0.0, 0.0, 0.0), 0xFF),
    (2, 1.0, (-0.37, 12.5, 0.11), 0x40),
    (2, 0.25, (0.0, 0.0, 0.0), 0xF0),
]


@pytest.mark.parametrize("source,voxel,origin,mask", PARITY)
def test_device_equals_the_restatement_bit_for_bit(ob, ob_run, source, voxel, origin, mask):
    _, _, _, lists = ob
    H = ob_run
    stored = H.place_read_keyframes()["poses"]
    H.closed_map_configure(voxel=voxel, origin=origin, cloud_mask=mask)
    if source == 0:
        want_poses, info = stored, H.closed_map_build(0)
    elif source == 1:
        want_poses, info = H.graph_poses(), H.closed_map_build()   # (the default source)
    else:
        want_poses = np.array([P @ GN.se3_exp(0.01 * np.array([k % 3, 1.0, 0.2, 0.1, -0.3, k % 5]))[0]
                               for k, P in enumerate(stored)])
        info = H.closed_map_build(2, want_poses)
    V, winfo = restate(want_poses, lists, mask, voxel, origin)
    print(f"source {source} voxel {voxel} origin {origin} mask {mask:#04x}: {info}")
    assert info["pose_source"] == source and info["n_keyframes"] == 2 * N_OUT and info["n_voxels"] > 1000
    assert info["empty_keyframes"] == 0 and info["overflow_keyframes"] == 0 and info["launches"] > 0
    same_as_restated(H, info, V, winfo)
    assert bits(H.closed_map_poses()) == bits(want_poses)
    assert bits(H.closed_map_poses(3, 2)) == bits(want_poses[3:5])
    assert bits(H.place_read_keyframes()["poses"]) == bits(stored)


def test_keyframes_added_after_the_optimise_take_the_last_correction(hip_module, ob):
    reg = hip_module
    thin, poses, _, lists = ob
    n, first = len(poses), len(poses) - 4
    H = ob_context(reg, ob, keep=range(first))
    assert H.loop_verify_pending() > 0
    H.graph_optimize()
    corrected = H.graph_poses()
    assert len(corrected) == first and np.max(np.abs(corrected - np.array(poses[:first]))) > 1e-6
    for k in range(first, n):
        assert H.place_add_scan(thin[k], poses[k], 100 + k) == k
        H.place_set_keyframe_clouds(k, *lists[k])
    info = H.closed_map_build(1)
    used = H.closed_map_poses()
    assert len(used) == n and bits(used[:first]) == bits(corrected)
    stored = H.place_read_keyframes()["poses"]
    for k in range(first, n):
        assert bits(used[k]) == bits(H.graph_correct_pose(-1, stored[k])), k
    V, winfo = restate(used, lists)
    same_as_restated(H, info, V, winfo)
    H.close()


# ---- 2: overflow and empties -----------------------------------------------------------------------------------------------
def test_overflow_and_empty_keyframes_and_refused_poses(hip_module, ob):
    reg = hip_module
    thin, poses, _, lists = ob
    H = ob_context(reg, ob)
    n = len(poses)
    # keyframe 9 has no target clouds, keyframe 20 only a cloud of non-finite points: 9 is empty, 20 adds no point
    none = [np.zeros((0, 3))] * 4
    H.place_set_keyframe_clouds(9, tgt=none)
    nan_cloud = np.full((5, 3), np.nan)
    nan_cloud[1] = [np.inf, 0.0, 0.0]
    H.place_set_keyframe_clouds(20, tgt=[nan_cloud, none[0], none[0], none[0]])
    clouds = [list(c) for c in lists]
    clouds[9] = [lists[9][0], none]
    clouds[20] = [lists[20][0], [nan_cloud, none[0], none[0], none[0]]]
    P = np.array(poses)
    far = P.copy()
    far[5, 0, 3] += float(1 << 20)           # keyframe 5 lies beyond 2^20 voxels of 1 m
    far[13, 1, 3] -= 1.5 * float(1 << 20)
    info = H.closed_map_build(2, far)
    V, winfo = restate(far, clouds)
    print("overflow:", info)
    assert (info["overflow_keyframes"], info["empty_keyframes"], info["added_keyframes"]) == (2, 1, n - 3)
    same_as_restated(H, info, V, winfo)
    others = [k for k in range(n) if k not in (5, 9, 13)]
    W, _ = restate(P[others], [clouds[k] for k in others])
    assert V.keys.tobytes() == W.keys.tobytes() and V.N.tobytes() == W.N.tobytes()   # the others are unaffected
    before = rows(H)
    bad = P.copy()
    bad[3, 1, 3] = np.nan
    with invalid(reg):
        H.closed_map_build(2, bad)
    bad = P.copy()
    bad[3, 0, 0] = 1.5                       # not a rotation
    with invalid(reg):
        H.closed_map_build(2, bad)
    bad = P.copy()
    bad[7, 3, 3] = np.inf
    with invalid(reg):
        H.closed_map_build(2, bad)
    with invalid(reg):
        H.closed_map_build(2, P[:-1])        # n_poses != K
    with invalid(reg):
        H.closed_map_build(3)
    with invalid(reg):
        H.closed_map_build(-1)
    with not_ready(reg):
        H.closed_map_build(1)                # no optimise yet
    assert rows(H) == before and H.closed_map_info() == info   # the previous closed map is still readable
    # every keyframe beyond the grid: an empty map, built
    H.closed_map_configure(voxel=1e-6)
    info = H.closed_map_build(0)
    assert (info["overflow_keyframes"], info["n_voxels"], info["n_points"]) == (n - 2, 0, 0)
    assert len(H.closed_map_read()[0]) == 0 and len(H.closed_map_read_box([-1e9] * 3, [1e9] * 3)[0]) == 0
    H.close()


# ---- 3: it closes the map --------------------------------------------------------------------------------------------------
def drift_case():
    """(thinned scans, true poses, drifted poses, the graph's i, j, Z, w): the true step composed with a fixed error per step;
    the loop edges are the true relative poses from every keyframe of the way back to the nearest one of the way out"""
    thin, poses, leg = RV.out_and_back(N_OUT, seed=SEED, **THIN)
    P = np.array(poses)
    n = len(P)
    err = GN.se3_exp(DRIFT)[0]
    D = [P[0]]
    for k in range(n - 1):
        D.append(D[k] @ LN.t_rel(P[k], P[k + 1]) @ err)
    D = np.array(D)
    out = np.flatnonzero(leg == 0)
    loops = [(int(out[np.argmin(np.linalg.norm(P[out, :3, 3] - P[q, :3, 3], axis=1))]), int(q)) for q in np.flatnonzero(leg == 1)]
    i = list(range(n - 1)) + [m for m, _ in loops]
    j = list(range(1, n)) + [q for _, q in loops]
    Z = [LN.t_rel(D[k], D[k + 1]) for k in range(n - 1)] + [LN.t_rel(P[m], P[q]) for m, q in loops]
    wo = [1.0 / 0.05 ** 2] * 3 + [1.0 / 0.005 ** 2] * 3   # the default sigmas (tloam_graph_default_config)
    wl = [1.0 / 0.05 ** 2] * 3 + [1.0 / 0.01 ** 2] * 3
    return thin, P, D, i, j, np.array(Z), np.array([wo] * (n - 1) + [wl] * len(loops))


def scan_clouds(thin):
    none = np.zeros((0, 3))
    return [[[none] * 4, [xyz, none, none, none]] for xyz in thin]


def test_it_closes_the_map(hip_module):
    """Voxels of 0.5 m from the same 608 121 points of the 32 thinned scans, each scan its keyframe's only cloud (restatement,
    on a CPU, the solve being tests/graph_np.py's direct one): 35 730 under the drifted poses, 26 193 under the solved
    ones, 25 624 under the true ones."""
    reg = hip_module
    thin, P, D, i, j, Z, w = drift_case()
    clouds = scan_clouds(thin)
    H = reg.HipRegistration()
    H.place_configure(enabled=1, exclude_recent=EX)
    H.loop_configure(enabled=1)
    for k, xyz in enumerate(thin):
        assert H.place_add_scan(xyz, D[k], k) == k
        H.place_set_keyframe_clouds(k, tgt=clouds[k][1])
    solved, ginfo = H.graph_solve(D, i, j, Z, w)
    assert ginfo["final_cost"] < ginfo["initial_cost"]
    H.closed_map_configure(voxel=DRIFT_VOXEL, cloud_mask=0x10)
    count = {}
    for name, poses in (("drifted", D), ("solved", solved), ("true", P)):
        info = H.closed_map_build(2, poses)
        V, winfo = restate(poses, clouds, 0x10, DRIFT_VOXEL)
        same_as_restated(H, info, V, winfo)
        count[name] = winfo["n_voxels"]
        assert winfo["n_points"] == 608121
    print(f"voxels of {DRIFT_VOXEL} m: {count}; largest position error {SG.position_error(D, P):.3f} m -> "
          f"{SG.position_error(solved, P):.3f} m")
    assert count["solved"] < count["drifted"]
    H.close()


# ---- 4: the same bits ------------------------------------------------------------------------------------------------------
def test_two_builds_and_two_contexts_give_the_same_bits(hip_module, ob, ob_run):
    reg = hip_module
    H = ob_run
    H.closed_map_configure()
    a = H.closed_map_build(0)
    first = rows(H)
    b = H.closed_map_build(0)
    assert a == b and rows(H) == first
    H.closed_map_build(1)
    assert rows(H) != first   # (the corrected poses give another map)
    H.closed_map_build(0)
    assert rows(H) == first
    other = ob_context(reg, ob)
    assert other.closed_map_build(0) == a and rows(other) == first
    other.close()


# ---- 5: constant launches --------------------------------------------------------------------------------------------------
def test_the_launches_do_not_depend_on_the_size(hip_module, ob, ob_run):
    reg = hip_module
    thin, poses, _, lists = ob
    H = ob_run
    launches = {}
    for mask in (0x10, 0xFF, 0xF0):
        H.closed_map_configure(cloud_mask=mask)
        launches[mask] = H.closed_map_build(0)
    big = reg.HipRegistration()
    big.place_configure(enabled=1, exclude_recent=EX)
    big.loop_configure(enabled=1)
    n = len(poses)
    for f in range(4 * n):
        assert big.place_add_scan(thin[f % n], poses[f % n], f) == f
        big.place_set_keyframe_clouds(f, *lists[f % n])
    info = big.closed_map_build(0)
    print({k: (v["n_points"], v["launches"]) for k, v in launches.items()}, (info["n_points"], info["launches"]))
    assert info["n_keyframes"] == 4 * n and info["n_points"] == 4 * launches[0xF0]["n_points"]
    assert info["n_voxels"] == launches[0xF0]["n_voxels"]   # (the same points four times over)
    assert info["launches"] == launches[0xF0]["launches"] == launches[0x10]["launches"] == launches[0xFF]["launches"]
    assert launches[0x10]["n_points"] < launches[0xF0]["n_points"] < launches[0xFF]["n_points"]
    V, winfo = restate(list(poses) * 4, list(lists) * 4)
    same_as_restated(big, info, V, winfo)
    big.close()


# ---- 6: undisturbed --------------------------------------------------------------------------------------------------------
def odom_run(reg, scans, hook=None):
    H = reg.HipRegistration()
    H.map_configure(reg.default_map_config(enabled=1))
    H.voxel_map_configure(reg.default_voxel_map_config(enabled=1))
    H.place_configure(enabled=1, **ODOM_PLACE)
    H.loop_configure(enabled=1)
    H.odometry_reset(None, odom_cfg(reg))
    res = []
    for f, xyz in enumerate(scans):
        rc, T, st = H.odometry_frame(xyz)
        assert rc in (0, -7), (f, rc)
        res.append({"pose": T, "stats": st, "reg": H.registered_scan(), "map_info": H.map_info(), "map": H.map_read(),
                    "vinfo": H.voxel_map_info(), "vmap": H.voxel_map_read()})
        if hook:
            hook(f, H)
    H.loop_verify_pending()
    H.graph_optimize()
    return H, res


def test_odometry_is_undisturbed_by_closed_map_builds(hip_module):
    reg = hip_module
    seq = G.sequence(7, seed=3)[0]
    seen = []

    def builds_between_frames(f, H):
        if f in (1, 2, 4, 6):
            if f == 4:
                H.graph_optimize()
            info = H.closed_map_build(1 if f >= 4 else 0)
            H.closed_map_read()
            H.closed_map_poses()
            assert info["n_keyframes"] == H.place_info()["n_keyframes"]
            seen.append(info)
            # the odometry's keyframes: the device's clouds and poses against the restatement
            K = info["n_keyframes"]
            V, winfo = restate(H.closed_map_poses(), [H.place_read_keyframe_clouds(k) for k in range(K)])
            same_as_restated(H, info, V, winfo)

    Hoff, off = odom_run(reg, seq)
    Hon, on = odom_run(reg, seq, hook=builds_between_frames)
    assert len(seen) == 4 and seen[-1]["n_keyframes"] >= 1 and seen[-1]["n_voxels"] > 0
    for f, (a, b) in enumerate(zip(on, off)):
        assert bits(a["pose"]) == bits(b["pose"]), f
        assert bits(a["reg"]) == bits(b["reg"]), f
        sa, sb = a["stats"], b["stats"]
        for key in sb:
            if key != "match":
                assert sa[key] == sb[key], (f, key)
        for key in ("host_syncs", "h2d_bytes", "d2h_bytes"):
            assert sa[key] == sb[key], (f, key)
        for key, v in sb["match"].items():
            if key != "host_wait_us":
                assert np.asarray(sa["match"][key]).tobytes() == np.asarray(v).tobytes(), (f, key)
        assert a["map_info"] == b["map_info"] and bits(a["map"]) == bits(b["map"]), f
        assert a["vinfo"] == b["vinfo"], f
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
    Hon.close(); Hoff.close()


# ---- 7: lifecycle ----------------------------------------------------------------------------------------------------------
def test_lifecycle_and_the_edges_of_the_contract(hip_module, ob):
    reg = hip_module
    _, poses, _, lists = ob

    def unbuilt(H):
        for read in (lambda: H.closed_map_read(0, 0), lambda: H.closed_map_read_box([-1.0] * 3, [1.0] * 3),
                     lambda: H.closed_map_poses(0, 0)):
            with not_ready(reg):
                read()
        assert H.closed_map_info()["n_voxels"] == 0 and H.closed_map_info()["n_keyframes"] == 0

    H = ob_context(reg, ob)
    unbuilt(H)
    with not_ready(reg):
        H.closed_map_build(1)   # before an optimise
    for over in (dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=np.nan), dict(voxel=np.inf), dict(origin=(0.0, np.nan, 0.0)),
                 dict(origin=(np.inf, 0.0, 0.0)), dict(cloud_mask=0), dict(cloud_mask=0x100), dict(cloud_mask=-1),
                 dict(reserve_voxels=-1)):
        with invalid(reg):
            H.closed_map_configure(**over)
    unbuilt(H)
    assert H.loop_verify_pending() > 0
    H.graph_optimize()
    info = H.closed_map_build()
    assert info["pose_source"] == 1 and info["n_voxels"] > 0
    for over in (dict(voxel=0.0), dict(cloud_mask=0)):   # a refused configuration leaves the closed map
        with invalid(reg):
            H.closed_map_configure(**over)
    assert H.closed_map_info() == info
    nv = info["n_voxels"]
    with invalid(reg):
        H.closed_map_read(0, nv + 1)
    with invalid(reg):
        H.closed_map_read(nv + 1, 0)
    with invalid(reg):
        H.closed_map_poses(0, len(poses) + 1)
    assert len(H.closed_map_read(nv, 0)[0]) == 0
    cen, cnt = H.closed_map_read()
    part = H.closed_map_read(7, 100)
    assert bits(part[0]) == bits(cen[7:107]) and part[1].tobytes() == cnt[7:107].tobytes()
    # read_box against the restatement's, and the short-capacity rule
    V, _ = restate(H.graph_poses(), lists)
    for lo, hi, mc in (([-5.0, -3.0, -2.0], [12.0, 3.0, 1.0], 1), ([-1e9] * 3, [1e9] * 3, 3), ([0.0] * 3, [0.5] * 3, 10 ** 9)):
        ids = V.box(lo, hi, mc)
        bc, bn = H.closed_map_read_box(lo, hi, mc)
        assert bits(bc) == bits(cen[ids]) and bn.tobytes() == cnt[ids].tobytes(), (lo, hi, mc)
    lo, hi = np.array([-5.0, -3.0, -2.0]), np.array([12.0, 3.0, 1.0])
    ids = V.box(lo, hi, 1)
    assert len(ids) > 1
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    n = C.c_size_t(0)
    short = np.full((1, 3), 7.0)
    assert H.L.tloam_closed_map_read_box(H.h, dp(lo), dp(hi), 1, 1, C.byref(n), dp(short), None) == -1
    assert n.value == len(ids) and np.all(short == 7.0)   # *n is the size; nothing was copied
    # the closed map survives tloam_graph_configure and a later optimise
    before = rows(H)
    H.graph_configure()
    assert rows(H) == before and H.closed_map_info() == info
    with not_ready(reg):
        H.closed_map_build(1)   # (the corrected poses went with the graph's configuration) ...
    assert rows(H) == before     # ... and the refused build left the closed map
    H.graph_optimize()
    assert rows(H) == before
    # what empties it
    H.closed_map_configure(voxel=2.0)
    unbuilt(H)
    assert H.closed_map_build()["n_voxels"] < nv
    for drop in (lambda: H.odometry_reset(None, odom_cfg(reg)), lambda: H.place_configure(enabled=1, exclude_recent=EX),
                 lambda: H.loop_configure(enabled=1)):
        H.closed_map_build(0)
        H.closed_map_read()
        drop()
        unbuilt(H)
    info = H.closed_map_build(0)   # no keyframes: an empty map, built
    assert info["n_keyframes"] == 0 and info["n_voxels"] == 0 and len(H.closed_map_read()[0]) == 0
    H.closed_map_build(0)
    H.loop_configure(enabled=0)
    with invalid(reg):              # loop verification off
        H.closed_map_build(0)
    unbuilt(H)
    H.close()


def test_the_configuration_persists_across_a_reset(hip_module, ob):
    reg = hip_module
    _, _, _, lists = ob
    H = ob_context(reg, ob)
    H.closed_map_configure(voxel=0.25, origin=(1.0, 2.0, 3.0), cloud_mask=0x0F)
    want = H.closed_map_build(0)
    first = rows(H)
    H.odometry_reset(None, odom_cfg(reg))
    thin, poses, _, _ = ob
    for f in range(len(poses)):
        assert H.place_add_scan(thin[f], poses[f], 100 + f) == f
        H.place_set_keyframe_clouds(f, *lists[f])
    assert H.closed_map_build(0) == want and rows(H) == first
    H.close()


# ---- 8: growth -------------------------------------------------------------------------------------------------------------
def test_the_rows_grow_inside_a_build(ob_run):
    H = ob_run
    H.closed_map_configure()
    want = H.closed_map_build(0)
    first = rows(H)
    assert want["capacity_voxels"] == 1 << 20
    H.closed_map_configure(reserve_voxels=64)
    assert H.closed_map_info()["capacity_voxels"] == 0
    info = H.closed_map_build(0)
    assert want["n_voxels"] <= info.pop("capacity_voxels") < want.pop("capacity_voxels")
    assert info == want and rows(H) == first
    H.closed_map_configure()
