"""-m gpu: the search grids' cell tables -- the frame-size build (32-bit histogram and scan, kinds starting on multiples of 4
entries, 16-byte accesses), its edges towards the small path, a cell that holds tens of thousands of points, re-zeroing of the
histograms across builds and paths on one context, and the cell of a sparse kind growing with its point count.  The checker is
the oracle's k-NN (counts, indices and squared distances bit for bit); every cloud is drawn from a seeded generator and every
case first asserts, on the host, that no query has two candidates at the same distance, so nothing hangs on tie order.
tloam_get_grid_info tells each case which build path it ran."""
import numpy as np
import pytest

from conftest import pose_delta
from oracle import binding as ob
from tloam_amd import synth

pytestmark = pytest.mark.gpu

CELLS_PER_POINT = 32          # a kind's table: at most max(16 Ki, 32 per point) cells (tl_grid_plan.hpp)
SCAN_TILE = 2048              # entries per scan tile (tl_grid_plan.hpp)


def _box_cloud(rng, lo, extent, n):
    """n points uniform in the box, two of them its corners: the grid's dimensions follow from `extent` alone."""
    lo = np.asarray(lo, float); extent = np.asarray(extent, float)
    p = lo + rng.uniform(0, 1, (n, 3)) * extent
    p[0] = lo
    p[1] = lo + extent
    return p


def _assert_no_ties(tgt, q, radius, k):
    """the k + 1 nearest in-radius candidates of every query lie at pairwise different distances"""
    for j in range(len(q)):
        d = tgt - q[j]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        d2 = np.sort(d2[d2 < radius * radius])[:k + 1]
        assert np.all(np.diff(d2) > 0), (j, d2)


def _check_knn(H, O, kind, tgt, q, radius, k):
    _assert_no_ties(tgt, q, radius, k)
    hi, hd, hc = H.knn(kind, q, radius, k)
    oi, od, oc = O.knn(kind, q, radius, k)
    assert np.array_equal(hc, oc)
    assert np.array_equal(hi, oi)
    assert np.array_equal(hd, od)
    return hc


def _pair(reg):
    return reg.HipRegistration(reg.default_config()), ob.Oracle(ob.make_config())


def _set(H, O, kind, tgt):
    H.set_target(kind, tgt)
    O.set_target(kind, tgt)


@pytest.mark.parametrize("cells_per_axis,path", [(25, "small"), (26, "tiles")])
def test_path_edges(hip_module, cells_per_axis, path):
    """25^3 cells (15 626 entries: the one-block scan) and 26^3 (17 576 cells: nine 2048-entry tiles, the last one partial)."""
    reg = hip_module
    rng = np.random.default_rng(100 + cells_per_axis)
    extent = (cells_per_axis - 0.5) * 1.0
    tgt = _box_cloud(rng, (-7.0, 3.0, -2.0), (extent,) * 3, 2000)
    q = np.concatenate([tgt[rng.integers(0, len(tgt), 200)] + rng.normal(0, 0.3, (200, 3)),
                        np.array([-7.0, 3.0, -2.0]) + extent + rng.uniform(40, 60, (50, 3)) * rng.choice([-1.0, 1.0], (50, 3))])
    H, O = _pair(reg)
    _set(H, O, 2, tgt)
    cnt = _check_knn(H, O, 2, tgt, q, 1.0, 5)
    assert cnt[:200].max() > 0 and cnt[200:].max() == 0
    gi = H.grid_info()
    assert gi["dim"][2] == [cells_per_axis] * 3 and gi["ncell"][2] == cells_per_axis ** 3 and gi["n"][2] == 2000
    if path == "small":
        assert gi["scan_path"] == reg.GRID_SCAN_SMALL and gi["table_elem_bytes"] == 8
    else:
        assert gi["scan_path"] == reg.GRID_SCAN_TILES and gi["table_elem_bytes"] == 4
        assert -(-(gi["ncell"][2] + 1) // SCAN_TILE) == 9
    assert H.info()["fallbacks_taken"] == 0
    H.close()


@pytest.fixture(scope="module")
def big_table_context(hip_module):
    """ONE context for the four builds around 2^21 cells below, which run in the order they are listed: a histogram or a table
    that one path's layout left wrong shows in the next build."""
    H, O = _pair(hip_module)
    yield H, O
    H.close()


# cells per axis at radius 1.0 and the path by table size alone: 1024 scan tiles exactly | 1024 tiles packed but 1025 padded, so
# neither the single-pass scan (judged on the packed size) nor the tile path (on the padded one) takes it | 129 blocks of 16 Ki
BIG_TABLES = [("tiles", (126, 130, 128)), ("generic", (150, 341, 41)), ("single_pass", (128, 128, 128)), ("tiles again", (126, 130, 128))]


@pytest.mark.parametrize("step,dims", BIG_TABLES, ids=[s for s, _ in BIG_TABLES])
def test_path_edges_at_two_million_cells(hip_module, big_table_context, step, dims):
    """One kind of 66 000 points (32 cells per point: the sparse bound does not bind) in a box with two corner points."""
    reg = hip_module
    H, O = big_table_context
    rng = np.random.default_rng(300 + dims[1])
    lo = np.array([-60.0, -70.0, -20.0])
    extent = np.array(dims, float) - 0.5
    tgt = _box_cloud(rng, lo, extent, 66000)
    q = np.concatenate([tgt[rng.integers(0, len(tgt), 200)] + rng.normal(0, 0.3, (200, 3)),
                        lo + extent + rng.uniform(40, 60, (50, 3)) * rng.choice([-1.0, 1.0], (50, 3))])
    _set(H, O, 2, tgt)
    cnt = _check_knn(H, O, 2, tgt, q, 1.0, 5)
    assert cnt[:200].max() > 0
    ncell = dims[0] * dims[1] * dims[2]
    cus = H.info()["device_cus"]
    if step.startswith("tiles"):
        path, width = reg.GRID_SCAN_TILES, 4
        n_tab = (ncell + 1 + 3) // 4 * 4 + 3 * 4          # the padded table: every kind without a grid still has its 4 entries
        assert -(-n_tab // SCAN_TILE) == 1024
    elif step == "single_pass" and 129 <= cus - cus // 16:
        path, width = reg.GRID_SCAN_SINGLE_PASS, 8
    else:
        path, width = reg.GRID_SCAN_GENERIC, 8
    gi = H.grid_info()
    print(step, "device_cus", cus, "scan_path", gi["scan_path"], "elem bytes", gi["table_elem_bytes"], "dim", gi["dim"][2], "ncell", gi["ncell"][2])
    assert gi["scan_path"] == path and gi["table_elem_bytes"] == width
    assert gi["dim"][2] == list(dims) and gi["ncell"][2] == ncell and gi["n"][2] == 66000
    assert H.info()["fallbacks_taken"] == 0


def _stepwise_against_oracle(H, O, T_pred, empty_kinds=()):
    """from the second sm_begin call on: outer iteration 0's correspondence index lists, then the final pose, against the oracle"""
    for it in range(8):
        rc_h, done_h, st_h = H.sm_outer()
        rc_o, done_o, st_o = O.sm_outer()
        assert rc_h == 0 and rc_o == 0
        assert st_h["n_corr"] == st_o["n_corr"], (it, st_h["n_corr"], st_o["n_corr"])
        if it == 0:
            for kind in range(4):
                ch, co = H.get_correspondences(kind), O.get_correspondences(kind)
                assert (len(ch["idx"]) > 0) == (kind not in empty_kinds)
                assert np.array_equal(ch["idx"], co["idx"]), kind
                np.testing.assert_allclose(ch["a"], co["a"], rtol=0, atol=1e-9)
        assert done_h == done_o
        if done_h:
            break
    _, T_h, st_h = H.sm_end()
    _, T_o, st_o = O.sm_end()
    dt, dr = pose_delta(T_h, T_o)
    assert dt < 1e-6 and dr < 1e-6, (dt, dr)
    assert st_h["outer_iterations"] == st_o["outer_iterations"]


def test_four_kinds_unaligned_bases(hip_module):
    """A KITTI-density target frame: four kinds in one table of several hundred thousand entries, none of kinds 1..3 starting
    on a tile.  Outer iteration 0's correspondence index lists and the final pose against the oracle."""
    reg = hip_module
    sc = synth.make_scene(seed=5, n_src=synth.SMALL_SRC, n_tgt=synth.KITTI_TGT)
    H, O = _pair(reg)
    H.set_frames(sc.source, sc.target)
    O.set_frames(sc.source, sc.target)
    assert H.sm_begin(sc.T_pred) == 0
    assert O.sm_begin(sc.T_pred) == 0
    gi = H.grid_info()
    assert gi["scan_path"] == reg.GRID_SCAN_TILES and gi["table_elem_bytes"] == 4
    assert gi["n"] == list(synth.KITTI_TGT)
    assert sum(gi["ncell"]) > 200_000
    base = 0
    for k in range(3):                                  # where kinds 1..3 start in the padded table
        base += (gi["ncell"][k] + 1 + 3) // 4 * 4
        assert base % SCAN_TILE != 0
    _stepwise_against_oracle(H, O, sc.T_pred)
    assert H.info()["fallbacks_taken"] == 0
    H.close()


def test_a_kind_without_a_finite_point_in_front_of_the_others(hip_module):
    """The same frame with the planar targets replaced by NaN points (twelve: a scan match takes no cloud of fewer than ten).
    That kind gets no grid and counts nothing, but keeps its twelve places in the point arrays: the cell starts of the kinds
    behind it are relative to the points COUNTED in front of them, not to their offset in those arrays."""
    reg = hip_module
    sc = synth.make_scene(seed=5, n_src=synth.SMALL_SRC, n_tgt=synth.KITTI_TGT)
    H, O = _pair(reg)
    H.set_frames(sc.source, sc.target)
    O.set_frames(sc.source, sc.target)
    _set(H, O, 0, np.full((12, 3), np.nan))
    assert H.sm_begin(sc.T_pred) == 0
    assert O.sm_begin(sc.T_pred) == 0
    gi = H.grid_info()
    assert gi["scan_path"] == reg.GRID_SCAN_TILES and gi["table_elem_bytes"] == 4
    assert gi["n"] == [0] + list(synth.KITTI_TGT[1:]) and gi["ncell"][0] == 0 and min(gi["ncell"][1:]) > 0
    _stepwise_against_oracle(H, O, sc.T_pred, empty_kinds=(0,))
    assert H.info()["fallbacks_taken"] == 0
    H.close()


def test_heavy_cell(hip_module):
    """70 000 points inside one cell: a count or a rank narrower than 32 bits cannot hold it."""
    reg = hip_module
    rng = np.random.default_rng(7)
    c = np.array([11.25, -3.75, 2.25])                 # the middle of a 0.5 m cell of the box below
    v = rng.normal(0, 1, (70000, 3))
    ball = c + v / np.linalg.norm(v, axis=1)[:, None] * (0.1 * rng.uniform(0, 1, (70000, 1)) ** (1 / 3))
    tgt = np.concatenate([_box_cloud(rng, (0.0, -15.0, -13.0), (30.0,) * 3, 2000), ball])
    v = rng.normal(0, 1, (32, 3))
    q = np.concatenate([c + v / np.linalg.norm(v, axis=1)[:, None] * 0.09 * rng.uniform(0, 1, (32, 1)),
                        tgt[rng.integers(0, 2000, 32)] + rng.normal(0, 0.2, (32, 3))])
    H, O = _pair(reg)
    _set(H, O, 0, tgt)
    cnt = _check_knn(H, O, 0, tgt, q, 0.5, 5)
    assert np.all(cnt[:32] == 5)
    gi = H.grid_info()
    assert gi["scan_path"] == reg.GRID_SCAN_TILES and gi["n"][0] == 72000
    assert H.info()["fallbacks_taken"] == 0
    H.close()


def test_histograms_are_empty_again_across_builds_and_paths(hip_module):
    """ONE context, four builds: tiles (A), small (B, another box), tiles with more cells (C), A again -- a histogram entry that
    a build left behind shifts every cell start behind it in the next build that uses the same buffer."""
    reg = hip_module
    rng = np.random.default_rng(21)
    A = _box_cloud(rng, (0.0, 0.0, 0.0), (29.5,) * 3, 2000)          # 30^3 = 27 000 cells
    B = _box_cloud(rng, (50.0, -20.0, 5.0), (9.5,) * 3, 1500)         # 10^3
    Cc = _box_cloud(rng, (-10.0, -10.0, -10.0), (37.5,) * 3, 2500)    # 38^3 = 54 872 cells
    H, O = _pair(reg)
    seen = []
    for tgt in (A, B, Cc, A):
        _set(H, O, 0, tgt)
        q = np.concatenate([tgt[rng.integers(0, len(tgt), 150)] + rng.normal(0, 0.3, (150, 3)), tgt[:2] + 0.01])
        cnt = _check_knn(H, O, 0, tgt, q, 1.0, 5)
        assert cnt.max() > 0
        gi = H.grid_info()
        seen.append((gi["scan_path"], gi["ncell"][0]))
    T, S = reg.GRID_SCAN_TILES, reg.GRID_SCAN_SMALL
    assert seen == [(T, 27000), (S, 1000), (T, 54872), (T, 27000)]
    assert H.info()["fallbacks_taken"] == 0
    H.close()


@pytest.mark.parametrize("k", [1, 5])
def test_sparse_kind_grows_its_cell(hip_module, k):
    """300 points over 70 x 70 x 6 m: at radius 0.5 the box is 235 k cells; the table is bounded by the points instead, the cell
    grows past the radius, and the search stays exact -- for queries at targets, near them, on the box's faces and 5 m outside."""
    reg = hip_module
    rng = np.random.default_rng(33)
    lo, ext = np.array([-35.0, -35.0, -1.0]), np.array([70.0, 70.0, 6.0])
    tgt = _box_cloud(rng, lo, ext, 300)
    tgt[2:42] = tgt[42:82] + rng.normal(0, 0.15, (40, 3))             # some points with neighbours inside the radius
    tgt[2:42] = np.clip(tgt[2:42], lo, lo + ext)
    u = rng.uniform(0, 1, (60, 3))
    u[np.arange(60), rng.integers(0, 3, 60)] = rng.integers(0, 2, 60)
    face = lo + u * ext
    outside = lo + rng.uniform(0, 1, (40, 3)) * ext
    outside[:, 0] = np.where(rng.uniform(0, 1, 40) < 0.5, lo[0] - 5.0, lo[0] + ext[0] + 5.0)
    q = np.concatenate([tgt[:100], tgt[rng.integers(0, 300, 100)] + rng.normal(0, 0.2, (100, 3)), face, outside])
    H, O = _pair(reg)
    _set(H, O, 3, tgt)
    cnt = _check_knn(H, O, 3, tgt, q, 0.5, k)
    assert np.all(cnt[:100] >= 1) and cnt[-40:].max() == 0
    gi = H.grid_info()
    assert gi["cell"][3] >= 0.5 * (1 + 1e-6)
    assert gi["ncell"][3] <= max(16384, CELLS_PER_POINT * 300)
    assert gi["cell"][3] > 1.0                                         # (the bound was binding: 235 k cells at the radius)
    assert H.info()["fallbacks_taken"] == 0
    H.close()
