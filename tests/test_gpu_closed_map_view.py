"""-m gpu: the view gain of the closed map (tl_view.hip, tl_api_view.hip) against its numpy restatement
(tests/closed_map_view_np.py), bit for bit: the records, the cells and the info without its diagnostics, under the LDS form and
the global form (at one and at more blocks a view).  The scenes and helpers are tests/test_gpu_closed_map_frontier.py's.

The LDS form is one block of 1024 threads a view, the global form blocks of 256; the ray counts below are chosen around those
numbers, the view counts so that the global form needs three chunks."""
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
import closed_map_view_np as WN  # noqa: E402
import diff_scenes as DS  # noqa: E402
import localise_scenes as LS  # noqa: E402
import test_gpu_closed_map_clearance as TK  # noqa: E402
import test_gpu_closed_map_free as TF  # noqa: E402
import test_gpu_closed_map_frontier as TQ  # noqa: E402
import test_gpu_closed_map_localise as TL  # noqa: E402
import test_gpu_closed_map_route as TR  # noqa: E402
import test_gpu_closed_map_surfel as TS  # noqa: E402
from tloam_amd import map_io  # noqa: E402
from tloam_amd.raycast import lidar_pattern  # noqa: E402

pytestmark = pytest.mark.gpu

bits, invalid, not_ready, built, log_bytes = TF.bits, TF.invalid, TF.not_ready, TF.built, TF.log_bytes
hand_map, boxed, cleared, wall = TK.hand_map, TK.boxed, TK.cleared, TK.wall
fronted, scene = TQ.fronted, TQ.scene
GOAL = TR.GOAL                               # the wall scene's sensor cell
FORMS = ((1, None), (2, "1"), (2, "3"), (2, None))    # (form, blocks a view of the global form: None is the library's own choice)


def plain(info):
    return {k: v for k, v in info.items() if k not in WN.DIAGNOSTICS}


def pose_at(p, turn=None):
    T = np.eye(4) if turn is None else LS.offset(np.eye(4), 0.0, turn)
    T[:3, 3] = p
    return T


@pytest.fixture
def blocks():
    """sets (or clears) the global form's blocks a view for one call"""
    def use(n):
        os.environ.pop("TLOAM_VIEW_BLOCKS", None)
        if n is not None:
            os.environ["TLOAM_VIEW_BLOCKS"] = n
    yield use
    os.environ.pop("TLOAM_VIEW_BLOCKS", None)


def same_gain(H, Vn, poses, ends, use, forms=FORMS, **cfg):
    """the records and the info of every form are the restatement's, and the forms' bytes are equal -> the records"""
    want, winfo = Vn.gain(poses, ends)
    assert winfo["beyond_window"] == 0
    for form, per_view in forms:
        use(per_view)
        H.closed_map_view_configure(max_range=float(Vn.max_range), form=form, **cfg)
        rec = H.closed_map_view_gain(poses, ends)
        info = H.closed_map_view_info()
        assert rec.dtype == WN.GAIN and rec.tobytes() == want.tobytes(), (form, per_view, rec, want)
        assert plain(info) == winfo, (plain(info), winfo)
        assert info["form"] == form and info["waits"] == 1 and info["launches"] == (1 if form == 1 else 2 * info["chunks"])
        if per_view is not None:
            assert info["blocks_per_view"] == int(per_view)
        assert (rec["reserved0"] == 0).all() and (rec["reserved1"] == 0).all()
    use(None)
    return want


# ---- a painted box: the analytic cases --------------------------------------------------------------------------------------------
A = np.array([5, 3, 6])


def painted(reg):
    """one FREE cell, A, in an unknown box of 24 x 20 x 16 cells of 1 m with a voxel at A - (4, 0, 0)"""
    H, G = scene(reg, [tuple(A - (4, 0, 0))], (0, 0, 0), (23, 19, 15), [(A, A)])
    N, info = fronted(H, G, min_cells=1)
    assert (info["free_cells"], info["occupied_cells"], info["frontier_cells"]) == (1, 1, 1)
    return H, G, N


def test_the_analytic_cases(hip_module, blocks):
    H, G, N = painted(hip_module)
    Vn = WN.ViewNP.of(N, 10.0)
    here = pose_at(G.o + (A + 0.5) * G.v)
    table = [([(7, 0, 0)], dict(unknown_cells=7, unknown_visits=7, free_visits=1, steps=8, rays_ended=1)),
             ([(7, 0, 0), (7, 0, 0)], dict(unknown_cells=7, unknown_visits=14, free_visits=2, steps=16, rays_ended=2)),   # distinct cells
             ([(7, 7, 0)], dict(unknown_cells=14, steps=15, rays_ended=1)),
             ([(5, 5, 5)], dict(unknown_cells=15, steps=16, rays_ended=1)),
             ([(-7, 0, 0)], dict(unknown_cells=3, rays_occupied=1, rays_ended=0, steps=5)),                             # the voxel
             ([(0, -7, 0)], dict(unknown_cells=3, rays_left_box=1, rays_ended=0, steps=5)),                             # the box's face
             ([(11, 0, 0)], dict(rays_skipped=1, steps=0, unknown_cells=0))]                                            # longer than max_range
    for d, want in table:
        rec = same_gain(H, Vn, here, np.array(d, np.float64) * G.v, blocks)
        assert {k: int(rec[k][0]) for k in want} == want, (d, rec)
        assert rec["origin_label"][0] == int(N.label[A[2], A[1], A[0]]) < QN.OUTSIDE       # a frontier label counts as free
    # a second context gives the same bytes
    ends = lidar_pattern(4, 33, -0.6, 0.6, 9.0)
    first = same_gain(H, Vn, here, ends, blocks)
    H2, G2, N2 = painted(hip_module)
    assert same_gain(H2, WN.ViewNP.of(N2, 10.0), here, ends, blocks).tobytes() == first.tobytes()
    H.close(); H2.close()


# ---- a mixed box: many views, ray counts round the blocks' threads, chunks --------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(hip_module):
    lo, hi = np.array((-6, -3, -2)), np.array((25, 20, 13))
    blo, bhi = 4 * (lo >> 2), 4 * (hi >> 2) + 3
    n = bhi - blo + 1
    rng = np.random.default_rng(33)
    voxels = blo + np.argwhere(rng.random(n) < 0.03)
    H, V = hand_map(hip_module, voxels)
    centre = 0.5 * (blo + bhi + 1.0) + 0.01
    G = boxed(H, V, lo, hi, rays=TK.star(centre, 0.45 * float(n.max()), n=150, seed=7), max_range=200.0, end_margin=0.0)
    N, info = fronted(H, G, min_cells=1)
    assert info["frontier_cells"] > 0 and info["occupied_cells"] > 0
    yield H, G, N, blo, bhi
    H.close()


def views_of(G, N, blo, bhi, count, seed=3):
    """`count` poses: at random in the box, then (from the fourth on) the special ones"""
    rng = np.random.default_rng(seed)
    poses = [pose_at(rng.uniform(blo + 1.0, bhi), turn=None) for _ in range(count)]
    if count >= 8:
        poses[3] = pose_at(np.array([4.0, 5.0, 6.0]) + [1.0 - 1e-9, 0.5, 1e-12])         # not a cell's centre: next to two faces
        poses[4] = LS.offset(pose_at((3.3, 4.4, 5.5)), 0.7, 0.4)                           # rotated
        poses[5] = pose_at(bhi + 4.5)                                                        # outside the box
        z, y, x = np.argwhere(N.label == QN.OCCUPIED)[0]
        poses[6] = pose_at(np.array([x, y, z]) + blo + 0.5)                                  # inside a voxel
        poses[7] = pose_at(blo + 0.5)                                                        # the box's corner cell
    return np.array(poses)


@pytest.mark.parametrize("rays", [1, 63, 64, 65, 1025])
def test_ray_counts(mixed, blocks, rays):
    H, G, N, blo, bhi = mixed
    Vn = WN.ViewNP.of(N, 6.0)
    ends = lidar_pattern(5, 205, -0.7, 0.7, 5.5)[np.arange(rays) * 1024 // max(rays, 1) % 1025][:rays]
    rec = same_gain(H, Vn, views_of(G, N, blo, bhi, 2), ends, blocks)
    assert rec["steps"].sum() >= rays


@pytest.mark.parametrize("views", [1, 2, 33])
def test_view_counts_and_chunks(mixed, blocks, hip_module, views):
    H, G, N, blo, bhi = mixed
    Vn = WN.ViewNP.of(N, 6.0)
    assert (Vn.S, Vn.bytes) == (15, 4 * 106)
    ends = lidar_pattern(6, 40, -0.8, 0.8, 5.9)
    poses = views_of(G, N, blo, bhi, views)
    rec = same_gain(H, Vn, poses, ends, blocks, max_bytes=16 * Vn.bytes)      # 16 windows at once: 33 views are three chunks
    assert H.closed_map_view_info()["chunks"] == -(-views // 16)
    if views == 33:
        assert rec["unknown_cells"].max() > 50 and len(set(rec["unknown_cells"].tolist())) > 10
        assert (rec["unknown_visits"] >= rec["unknown_cells"]).all() and (rec["unknown_visits"] > rec["unknown_cells"]).any()
        assert rec["origin_label"][5] == QN.OUTSIDE and rec["rays_left_box"][5] == len(ends) and rec["steps"][5] == len(ends)
        assert rec["origin_label"][6] == QN.OCCUPIED and rec["rays_occupied"][6] == len(ends) and rec["unknown_cells"][6] == 0
        # two calls give the same bytes
        assert H.closed_map_view_gain(poses, ends).tobytes() == rec.tobytes()
        # one window at once: 33 chunks; not even one: refused
        same_gain(H, Vn, poses, ends, blocks, forms=((2, None),), max_bytes=Vn.bytes)
        assert H.closed_map_view_info()["chunks"] == 33
        H.closed_map_view_configure(max_range=6.0, form=2, max_bytes=Vn.bytes - 1)
        with invalid(hip_module):
            H.closed_map_view_gain(poses, ends)
        H.closed_map_view_configure()


def test_windows_and_the_form_choice(mixed, blocks, hip_module):
    reg = hip_module
    H, G, N, blo, bhi = mixed
    poses = views_of(G, N, blo, bhi, 8)
    # S = 5: 125 bits, no multiple of 32 (max_range 0.8 at a voxel of 1: W = 2)
    Vn = WN.ViewNP.of(N, 0.8)
    assert (Vn.W, Vn.S, Vn.words) == (2, 5, 4)
    rng = np.random.default_rng(2)
    ends = rng.normal(size=(200, 3))
    ends *= rng.uniform(0.2, 0.85, (200, 1)) / np.linalg.norm(ends, axis=1, keepdims=True)
    rec = same_gain(H, Vn, poses, ends, blocks)
    assert rec["rays_skipped"].min() > 0 and rec["unknown_cells"].max() > 3
    # a window of exactly lds_bytes runs in the LDS form; one word above it form 1 is refused and auto runs the global form
    Vn = WN.ViewNP.of(N, 6.0)
    ends = lidar_pattern(6, 40, -0.8, 0.8, 5.9)
    want, winfo = Vn.gain(poses, ends)
    H.closed_map_view_configure(max_range=6.0, lds_bytes=Vn.bytes)
    assert H.closed_map_view_gain(poses, ends).tobytes() == want.tobytes() and H.closed_map_view_info()["form"] == 1
    H.closed_map_view_configure(max_range=6.0, lds_bytes=Vn.bytes, form=1)
    assert H.closed_map_view_gain(poses, ends).tobytes() == want.tobytes() and H.closed_map_view_info()["form"] == 1
    H.closed_map_view_configure(max_range=6.0, lds_bytes=Vn.bytes - 4)
    assert H.closed_map_view_gain(poses, ends).tobytes() == want.tobytes() and H.closed_map_view_info()["form"] == 2
    last = H.closed_map_view_info()
    H.closed_map_view_configure(max_range=6.0, lds_bytes=Vn.bytes - 4, form=1)
    assert H.closed_map_view_info() == reg.ViewInfo().as_dict()            # a configure clears the last info
    raw = np.zeros(len(poses), WN.GAIN)
    raw["reserved1"] = 9
    flat = np.ascontiguousarray(poses.transpose(0, 2, 1)).reshape(-1)
    dp = C.POINTER(C.c_double)
    assert H.L.tloam_closed_map_view_gain(H.h, flat.ctypes.data_as(dp), len(poses), np.ascontiguousarray(ends).ctypes.data_as(dp), len(ends),
                                          raw.ctypes.data, None) == -1
    assert (raw["reserved1"] == 9).all() and H.closed_map_view_info() == reg.ViewInfo().as_dict()
    assert last["form"] == 2
    # the default window (max_range 20 at a voxel of 1: S = 43, 9 940 bytes) in both forms
    same_gain(H, WN.ViewNP.of(N, 20.0), poses[:3], lidar_pattern(4, 30, -0.5, 0.5, 19.0), blocks, forms=((1, None), (2, None)))
    H.closed_map_view_configure()


# ---- the wall ----------------------------------------------------------------------------------------------------------------------
def test_the_wall_from_its_sensor_cell(wall, blocks, tmp_path):
    H, V, G, poses, clouds, scan, truth = wall
    N, info = fronted(H, G)
    Vn = WN.ViewNP.of(N, 10.0)
    assert (Vn.W, Vn.S) == (21, 43)
    ends = lidar_pattern(8, 90, -0.3, 0.3, 9.5)
    here = pose_at(GOAL[0])
    rec = same_gain(H, Vn, np.array([here, LS.offset(here, 0.4, 0.3), truth]), ends, blocks)
    assert rec["unknown_cells"][0] > 100 and rec["rays_occupied"][0] > 0 and rec["unknown_visits"][0] > rec["unknown_cells"][0]
    # windows above 64 KiB of LDS (the launch needs its attribute raised): the default max_range at this voxel, S = 83 and
    # 71 476 bytes, and the largest side under the default lds_bytes, S = 101 and 128 788 bytes
    for max_range, side, nbytes in ((20.0, 83, 71476), (24.5, 101, 128788)):
        big = WN.ViewNP.of(N, max_range)
        assert (big.S, big.bytes) == (side, nbytes) and nbytes <= 131072
        same_gain(H, big, np.array([here, truth]), lidar_pattern(4, 45, -0.3, 0.3, max_range - 0.5), blocks, forms=((1, None), (2, None)))
    # the cells: the set, the order, the capacities, the PCD export
    H.closed_map_view_configure(max_range=10.0)
    wc, wrec = Vn.cells(here, ends)
    for form in (1, 2):
        H.closed_map_view_configure(max_range=10.0, form=form)
        cen, one = H.closed_map_view_cells(here, ends)
        assert bits(cen) == bits(wc) and one.tobytes() == wrec.tobytes() == rec[:1].tobytes() and len(cen) == rec["unknown_cells"][0]
    assert {tuple(c) for c in np.floor((cen - G.o) / G.v).astype(int).tolist()} == {c for c in WN.cells_by_loop(Vn, here, ends)}
    m = len(cen)
    dp = C.POINTER(C.c_double)
    flat, e = np.ascontiguousarray(here.T).reshape(-1), np.ascontiguousarray(ends)
    out, got, one = np.full((m + 1, 3), 9.0), C.c_size_t(77), np.zeros(1, WN.GAIN)
    args = (H.h, flat.ctypes.data_as(dp), e.ctypes.data_as(dp), len(e))
    for cap in (0, m - 1):
        assert H.L.tloam_closed_map_view_cells(*args, cap, out.ctypes.data_as(dp), C.byref(got), one.ctypes.data) == -1
        assert got.value == m and (out == 9.0).all()
    assert H.L.tloam_closed_map_view_cells(*args, m, None, C.byref(got), None) == 0 and got.value == m
    assert H.L.tloam_closed_map_view_cells(*args, m, out.ctypes.data_as(dp), C.byref(got), one.ctypes.data) == 0
    assert bits(out[:m]) == bits(wc) and (out[m] == 9.0).all() and one.tobytes() == wrec.tobytes()
    assert H.L.tloam_closed_map_view_cells(*args, m, out.ctypes.data_as(dp), None, None) == -1
    for ascii in (False, True):
        path = str(tmp_path / f"view{int(ascii)}.pcd")
        assert map_io.write_view_pcd(path, H, here, ends, ascii=ascii) == m
        assert bits(map_io.read_view_pcd(path)) == bits(wc)
    H.closed_map_view_configure()


def test_frontier_gains(wall, blocks, hip_module):
    reg = hip_module
    H, V, G, poses, clouds, scan, truth = wall
    N, info = fronted(H, G)
    Vn = WN.ViewNP.of(N, 10.0)
    ends = lidar_pattern(4, 60, -0.3, 0.3, 9.0)
    H.closed_map_view_configure(max_range=10.0)
    with not_ready(reg):
        H.closed_map_frontier_gains(ends)                                              # no route field
    seen = []
    for wrap, radius, reach in ((0, 0.0, 2), (1, 1.0, 2), (1, 1.0, 0)):
        K, _ = cleared(H, G, max_distance=4.0, unknown_is_obstacle=wrap)
        TR.routed(H, K, GOAL, radius)
        H.closed_map_frontier_configure(reach=reach)
        H.closed_map_frontier_build()
        cost, approach = H.closed_map_frontier_costs()
        k = len(cost)
        assert k >= 1
        P = np.tile(np.eye(4), (k, 1, 1))
        P[:, :3, 3] = approach
        want, _ = Vn.gain(P, ends)
        for form in (1, 2):
            H.closed_map_view_configure(max_range=10.0, form=form)
            rec, c2, a2 = H.closed_map_frontier_gains(ends)
            assert c2.tobytes() == cost.tobytes() and bits(a2) == bits(approach) and rec.tobytes() == want.tobytes()
            vinfo = H.closed_map_view_info()
            assert vinfo["views"] == k and vinfo["waits"] == 2 and vinfo["form"] == form
            finite = np.isfinite(approach).all(axis=1)
            if finite.any():
                assert rec[finite].tobytes() == H.closed_map_view_gain(P[finite], ends).tobytes()
        none = cost == RN.UNREACHED
        assert (rec["rays_skipped"][none] == len(ends)).all() and (rec["origin_label"][none] == QN.OUTSIDE).all()
        assert (rec["steps"][none] == 0).all() and (rec["steps"][~none] > 0).all()
        seen.append(int(none.sum()))
    assert seen[0] == 0 and seen[2] == k                                               # all reached; none (reach 0, a wide body)
    # the capacity convention of the clusters
    dp = C.POINTER(C.c_double)
    e = np.ascontiguousarray(ends)
    got = C.c_size_t(77)
    rec, cost, app = np.zeros(k + 1, WN.GAIN), np.full(k + 1, 9, np.uint32), np.full((k + 1, 3), 9.0)
    rec["reserved1"] = 9
    call = H.L.tloam_closed_map_frontier_gains
    up = cost.ctypes.data_as(C.POINTER(C.c_uint32))
    for cap in (0, k - 1):
        assert call(H.h, e.ctypes.data_as(dp), len(e), cap, rec.ctypes.data, up, app.ctypes.data_as(dp), C.byref(got)) == -1
        assert got.value == k and (rec["reserved1"] == 9).all() and (cost == 9).all() and (app == 9.0).all()
    assert call(H.h, e.ctypes.data_as(dp), len(e), k, None, None, None, C.byref(got)) == 0 and got.value == k
    assert call(H.h, e.ctypes.data_as(dp), len(e), k, rec.ctypes.data, up, None, C.byref(got)) == 0 and rec["reserved1"][k] == 9 and cost[k] == 9
    assert call(H.h, None, len(e), k, rec.ctypes.data, up, None, C.byref(got)) == -1
    assert call(H.h, e.ctypes.data_as(dp), 0, k, rec.ctypes.data, up, None, C.byref(got)) == -1
    assert call(H.h, e.ctypes.data_as(dp), len(e), k, rec.ctypes.data, up, None, None) == -1
    H.closed_map_frontier_configure()
    H.closed_map_view_configure()


# ---- lifetime and refusals ---------------------------------------------------------------------------------------------------------
def test_not_ready_and_refusals(wall, hip_module):
    reg = hip_module
    H, V, G, poses, clouds, scan, truth = wall
    zero = reg.ViewInfo().as_dict()
    ends = lidar_pattern(2, 30, -0.2, 0.2, 5.0)
    here = pose_at(GOAL[0])
    H.closed_map_view_configure(max_range=10.0)
    calls = (lambda: H.closed_map_view_gain(here, ends), lambda: H.closed_map_view_cells(here, ends), lambda: H.closed_map_frontier_gains(ends))
    drops = [H.closed_map_frontier_configure, lambda: H.closed_map_free_add_scan(scan[:50], truth), H.closed_map_free_reset,
             lambda: H.closed_map_free_configure(**TF.WALL)]
    for k, drop in enumerate(drops):
        H.closed_map_free_build()
        H.closed_map_frontier_build()
        first = H.closed_map_view_gain(here, ends)
        assert H.closed_map_view_info()["views"] == 1
        H.closed_map_frontier_build()                                                  # a new field: the last call was not of it
        assert H.closed_map_view_info() == zero
        assert H.closed_map_view_gain(here, ends).tobytes() == first.tobytes()
        drop()
        assert H.closed_map_view_info() == zero, k
        for call in calls:
            with not_ready(reg):
                call()
    H.closed_map_free_build()
    H.closed_map_frontier_build()
    rec = H.closed_map_view_gain(here, ends)
    info = H.closed_map_view_info()

    def untouched():
        return H.closed_map_view_info() == info and H.closed_map_view_gain(here, ends).tobytes() == rec.tobytes() and H.closed_map_view_info() == info

    for bad in (dict(max_range=0.0), dict(max_range=-1.0), dict(max_range=np.inf), dict(max_range=np.nan), dict(max_bytes=3), dict(max_bytes=-1),
                dict(lds_bytes=-1), dict(lds_bytes=1 << 20), dict(form=-1), dict(form=3)):
        with invalid(reg):
            H.closed_map_view_configure(**bad)
    with pytest.raises(KeyError):
        H.closed_map_view_configure(radius=1.0)
    assert untouched()
    for bad_pose in (2.0 * np.eye(4), np.full((4, 4), np.nan), np.diag([1.0, 1.0, -1.0, 1.0]), pose_at([np.nan, 0.0, 0.0])):
        with invalid(reg):
            H.closed_map_view_gain(np.array([here, bad_pose]), ends)
        with invalid(reg):
            H.closed_map_view_cells(bad_pose, ends)
    dp = C.POINTER(C.c_double)
    flat, e = np.ascontiguousarray(here.T).reshape(-1), np.ascontiguousarray(ends)
    out = np.zeros(2, WN.GAIN)
    out["reserved1"] = 9
    fp, ep = flat.ctypes.data_as(dp), e.ctypes.data_as(dp)
    gain = H.L.tloam_closed_map_view_gain
    assert gain(H.h, None, 1, ep, len(e), out.ctypes.data, None) == -1 and gain(H.h, fp, 1, None, len(e), out.ctypes.data, None) == -1
    assert gain(H.h, fp, 1, ep, len(e), None, None) == -1 and gain(H.h, fp, 0, ep, len(e), out.ctypes.data, None) == -1
    assert gain(H.h, fp, 1, ep, 0, out.ctypes.data, None) == -1 and gain(H.h, fp, 1, ep, (1 << 28) + 1, out.ctypes.data, None) == -1
    assert gain(H.h, fp, 1 << 62, ep, 1 << 40, out.ctypes.data, None) == -1        # V * R beyond int64: refused before anything is read
    assert (out["reserved1"] == 9).all() and untouched()
    vinfo = reg.ViewInfo()
    assert gain(H.h, fp, 1, ep, len(e), out.ctypes.data, C.byref(vinfo)) == 0 and vinfo.as_dict() == info and out[:1].tobytes() == rec.tobytes()
    assert out["reserved1"][1] == 9
    assert H.L.tloam_closed_map_get_view_info(H.h, None) == -1
    # nranks > 1: every call is refused
    X = reg.HipRegistration()
    X.comm_init_callback(0, 2, lambda dev, count, stream: 0)
    for call in (X.closed_map_view_configure, X.closed_map_view_info, lambda: X.closed_map_view_gain(here, ends),
                 lambda: X.closed_map_view_cells(here, ends), lambda: X.closed_map_frontier_gains(ends)):
        with invalid(reg):
            call()
    X.close()
    H.closed_map_view_configure()
    # the configuration persists across an odometry reset
    clouds = [CS.slot0(np.array([[1.5, 1.5, 1.5], [5000.5, 5000.5, 5000.5]]))]
    F, Vf = built(reg, [np.eye(4)], clouds, CS.MASK, 1.0, (0.0, 0.0, 0.0))
    F.closed_map_view_configure(max_range=3.0, form=2)
    F.odometry_reset(None, TS.TC.odom_cfg(reg))
    assert F.place_add_scan(TS.DUMMY, np.eye(4), 0) == 0
    F.place_set_keyframe_clouds(0, *clouds[0])
    F.closed_map_build(2, [np.eye(4)])
    boxed(F, Vf, (0, 0, 0), (7, 7, 7))
    F.closed_map_frontier_build()
    got = F.closed_map_view_gain(pose_at((4.5, 4.5, 4.5)), np.array([[2.0, 0.0, 0.0], [3.5, 0.0, 0.0]]))
    assert (got["rays_skipped"][0], got["unknown_cells"][0]) == (1, 3)
    assert (F.closed_map_view_info()["form"], F.closed_map_view_info()["window_side"]) == (2, 9)
    F.close()


def test_the_view_changes_nothing_else(hip_module, blocks):
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
    K, _ = cleared(H, G, misses=M, unknown_is_obstacle=0)
    cen = G.free_cells(misses=M)
    R, _ = TR.routed(H, K, cen[:2], 0.0)
    N, _ = fronted(H, G, M)
    prior = LS.offset(pose, 0.1, 0.01)

    def everything(X):
        rows = X.closed_map_read()
        found = X.closed_map_localise(scan, prior)
        through, hits = X.closed_map_diff_counts()
        return (bits(rows[0]) + rows[1].tobytes(), X.closed_map_misses().tobytes(), TS.surfel_bytes(X), X.closed_map_free_words().tobytes(),
                X.closed_map_free_info(), X.closed_map_clearance_field().tobytes(), X.closed_map_clearance_info(),
                X.closed_map_route_field().tobytes(), X.closed_map_route_info(),
                X.closed_map_frontier_field().tobytes(), X.closed_map_frontier_info(), X.closed_map_frontier_clusters()[0].tobytes(),
                through.tobytes() + hits.tobytes(), bits(found[0]), {**found[1], "prepared": 0},
                log_bytes(X.closed_map_localise_log()), {**X.closed_map_diff_info(), "prepared": 0, "launches": 0},
                X.closed_map_save(), X.closed_map_save(clouds=True))

    before = everything(H)
    Vn = WN.ViewNP.of(N, 8.0)
    ends = lidar_pattern(6, 60, -0.4, 0.4, 7.5)
    views = np.array([pose, LS.offset(pose, 1.0, 0.5), pose_at(cen[0])])
    rec = same_gain(H, Vn, views, ends, blocks)
    assert rec["unknown_cells"].max() > 0
    wc, _ = Vn.cells(pose, ends)
    assert bits(H.closed_map_view_cells(pose, ends)[0]) == bits(wc)
    got, cost, approach = H.closed_map_frontier_gains(ends)
    assert len(got) == len(N.kept) and cost.tobytes() == N.costs(R.cost)[0].tobytes()
    assert everything(H) == before
    H.close()
