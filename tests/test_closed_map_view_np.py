"""The view gain's restatement (tests/closed_map_view_np.py) on hand-made label arrays, without a GPU:
the analytic walks, the four rules of a visited cell, the skip rule, the window bound and the set against a plain loop."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import closed_map_carve_np as CN  # noqa: E402
import closed_map_frontier_np as QN  # noqa: E402
import closed_map_view_np as WN  # noqa: E402

V, O = 0.5, np.array([-1.0, 0.25, 2.0])            # the grid: voxel and origin
A = np.array([3, 4, 5])                            # the cell the views stand in
LO, N = np.array([-2, -1, 0]), np.array([24, 20, 16])


def centre(c):
    return O + (np.asarray(c, np.float64) + 0.5) * V


def pose_at(p):
    T = np.eye(4)
    T[:3, 3] = p
    return T


def box(fill=QN.UNKNOWN, free=(A,), occupied=()):
    """-> ViewNP over a box of `fill` with the cells `free` FREE and `occupied` OCCUPIED (absolute cells)"""
    label = np.full(N[::-1], fill, np.uint32)
    for c, val in [(c, QN.FREE) for c in free] + [(c, QN.OCCUPIED) for c in occupied]:
        x, y, z = np.asarray(c) - LO
        label[z, y, x] = val
    return WN.ViewNP(label, LO, O, V, max_range=10.0)


def ends_to(*cells):
    """segment ends, in the frame of the view at A's centre, at the centres of the cells A + d"""
    return np.array([centre(A + np.asarray(d)) - centre(A) for d in cells])


@pytest.mark.parametrize("d, cells", [((7, 0, 0), 8), ((7, 7, 0), 15), ((5, 5, 5), 16)])
def test_the_analytic_walks(d, cells):
    """centre to centre: n + 1 cells, the end cell included; on a diagonal every tie goes to the lowest axis"""
    path, last = CN.walk((centre(A) - O) / V, (centre(A + np.asarray(d)) - O) / V)
    assert len(path) + 1 == cells and last.tolist() == (A + np.asarray(d)).tolist()
    if d == (7, 7, 0):
        assert (path[1] - path[0]).tolist() == [1, 0, 0] and (path[2] - path[1]).tolist() == [0, 1, 0]
    rec, info = box().gain(pose_at(centre(A)), ends_to(d))
    assert rec["steps"][0] == cells and rec["unknown_cells"][0] == cells - 1 and rec["rays_ended"][0] == 1
    assert info["beyond_window"] == 0


def test_distinct_cells_not_visits():
    Vw = box()
    rec, info = Vw.gain(pose_at(centre(A)), ends_to((7, 0, 0)))
    assert (rec["unknown_cells"][0], rec["unknown_visits"][0], rec["free_visits"][0], rec["rays_ended"][0]) == (7, 7, 1, 1)
    assert rec["origin_label"][0] == QN.FREE and rec["steps"][0] == 8
    rec, info = Vw.gain(pose_at(centre(A)), ends_to((7, 0, 0), (7, 0, 0)))
    assert (rec["unknown_cells"][0], rec["unknown_visits"][0], rec["free_visits"][0], rec["rays_ended"][0]) == (7, 14, 2, 2)
    assert info == dict(views=1, rays=2, window_side=2 * 21 + 1, window_bytes=4 * ((43 ** 3 + 31) // 32), steps=16, unknown_visits=14,
                        unknown_cells=7, beyond_window=0)
    # two rays that share their first three unknown cells
    rec, _ = Vw.gain(pose_at(centre(A)), ends_to((7, 0, 0), (3, 0, 0)))
    assert (rec["unknown_cells"][0], rec["unknown_visits"][0]) == (7, 10)
    # a frontier label counts as free
    Vw.label[(A - LO)[2], (A - LO)[1], (A - LO)[0] + 1] = 12345
    rec, _ = Vw.gain(pose_at(centre(A)), ends_to((7, 0, 0)))
    assert (rec["unknown_cells"][0], rec["free_visits"][0]) == (6, 2)


def test_a_voxel_and_a_box_face_stop_the_ray():
    rec, _ = box(occupied=[A + (4, 0, 0)]).gain(pose_at(centre(A)), ends_to((7, 0, 0)))
    assert (rec["unknown_cells"][0], rec["rays_occupied"][0], rec["rays_ended"][0], rec["steps"][0]) == (3, 1, 0, 5)
    # the box's low x face is 5 cells from A; a face 3 cells away: a view at LO + (2, ...)
    a = np.array([LO[0] + 2, A[1], A[2]])
    Vw = box(free=(a,))
    ends = np.array([centre(a + (-7, 0, 0)) - centre(a)])
    rec, _ = Vw.gain(pose_at(centre(a)), ends)
    assert (rec["rays_left_box"][0], rec["unknown_cells"][0], rec["steps"][0], rec["rays_ended"][0]) == (1, 2, 4, 0)


def test_bad_origins_and_long_rays():
    Vw = box()
    ends = ends_to((7, 0, 0), (0, 3, 0), (0, 0, -2))
    outside = pose_at(centre(LO - (3, 0, 0)))
    rec, _ = Vw.gain(outside, ends)                                # every ray ends at its first cell
    assert (rec["rays_left_box"][0], rec["steps"][0], rec["unknown_cells"][0], rec["rays_skipped"][0]) == (3, 3, 0, 0)
    assert rec["origin_label"][0] == QN.OUTSIDE
    nan = pose_at([np.nan, 1.0, 1.0])
    rec, _ = Vw.gain(nan, ends)
    assert (rec["rays_skipped"][0], rec["steps"][0], rec["origin_label"][0]) == (3, 0, QN.OUTSIDE)
    # inside a voxel: every ray stops at its first cell
    rec, _ = box(free=(), occupied=[A]).gain(pose_at(centre(A)), ends)
    assert (rec["rays_occupied"][0], rec["steps"][0], rec["origin_label"][0]) == (3, 3, QN.OCCUPIED)
    # longer than max_range, of no length, not finite: skipped
    far = np.array([[10.0 + 1e-9, 0.0, 0.0], [0.0, 0.0, 0.0], [np.inf, 0.0, 0.0], [10.0, 0.0, 0.0]])
    rec, _ = Vw.gain(pose_at(centre(A)), far)
    assert (rec["rays_skipped"][0], rec["rays_left_box"][0]) == (3, 1)


@pytest.mark.parametrize("max_range, voxel", [(20.0, 0.5), (10.0, 0.5), (0.4, 0.5), (7.3, 0.3)])
def test_every_visited_cell_lies_in_the_window(max_range, voxel):
    """random rays of up to max_range from random origins in an all-unknown box that holds them all: no cell beyond the window,
    and the worst offset is at most W"""
    rng = np.random.default_rng(5)
    W, S, words, nbytes = WN.window(max_range, voxel)
    assert W == int(np.ceil(max_range / voxel)) + 1 and S == 2 * W + 1 and nbytes == 4 * words
    n = 2 * W + 8
    label = np.full((n, n, n), QN.UNKNOWN, np.uint32)
    Vw = WN.ViewNP(label, (-W - 4,) * 3, (0.1, -0.2, 0.3), voxel, max_range)
    worst = 0
    for k in range(6):
        o = np.array([0.1, -0.2, 0.3]) + rng.uniform(-1.0, 1.0, 3) * voxel
        d = rng.normal(size=(500, 3))
        d *= (max_range * rng.uniform(0.9, 1.0, (500, 1))) / np.linalg.norm(d, axis=1, keepdims=True)
        d[:50] = np.eye(3)[rng.integers(0, 3, 50)] * max_range * rng.choice([-1.0, 1.0], (50, 1))      # along the axes, full length
        rec, bits, beyond, cO = Vw.view(pose_at(o), d)
        assert beyond == 0 and rec["rays_left_box"][0] == 0
        row, dx = np.divmod(bits, S)
        dz, dy = np.divmod(row, S)
        worst = max(worst, int(np.abs(np.stack([dx, dy, dz]) - W).max()))
    assert worst <= W


def test_the_set_is_the_plain_loops():
    rng = np.random.default_rng(9)
    label = np.where(rng.random(N[::-1]) < 0.5, QN.UNKNOWN, QN.FREE).astype(np.uint32)
    label[rng.random(N[::-1]) < 0.03] = QN.OCCUPIED
    label[rng.random(N[::-1]) < 0.05] = 77                        # frontier labels
    Vw = WN.ViewNP(label, LO, O, V, max_range=6.0)
    d = rng.normal(size=(120, 3))
    d *= rng.uniform(0.5, 6.5, (120, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    pose = pose_at(centre(A) + [0.2, -0.1, 0.24])
    pose[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    cen, rec = Vw.cells(pose, d)
    want = WN.cells_by_loop(Vw, pose, d)
    assert rec["unknown_cells"][0] == len(cen) == len(want) > 50
    got = {tuple(int(v) for v in np.floor((c - O) / V)) for c in cen}
    assert got == want
    assert rec["unknown_visits"][0] > rec["unknown_cells"][0]      # rays from one origin share their first cells
    assert rec["rays_skipped"][0] > 0 and rec["rays_occupied"][0] > 0 and rec["rays_left_box"][0] + rec["rays_ended"][0] > 0
    assert rec["rays_skipped"][0] + rec["rays_occupied"][0] + rec["rays_left_box"][0] + rec["rays_ended"][0] == 120
    # ascending in bit index
    _, bits, _, cO = Vw.view(pose, d)
    assert (np.diff(bits) > 0).all() and np.array_equal(Vw.centres(bits, cO), cen)
