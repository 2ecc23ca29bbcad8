"""CPU: every scene of tests/loop_scenes.py meets the condition it is named for, from the scene alone (no device): the clipped
windows, the sphere totals that pass 10 by the clamp alone, the span counts and launches, the rows of one launch and the points
of one kind beyond the kernels' thread counts, and what all scenes share (rigid poses with roll and pitch a metre apart, clouds
that are all different, sizes)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import loop_np as LN  # noqa: E402
import loop_scenes as LS  # noqa: E402

SMALL = [n for n in LS.NAMES if n not in ("big_rows", "big_source")]


@pytest.mark.parametrize("name", LS.NAMES)
def test_what_every_scene_has(name):
    sc = LS.scene(name)
    n = len(sc.poses)
    assert len(sc.src) == len(sc.tgt) == n and 0 <= sc.m < sc.q < n
    for k, P in enumerate(sc.poses):
        R = P[:3, :3]
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-14 and np.linalg.det(R) > 0 and LS.bits(P[3]) == LS.bits([0, 0, 0, 1])
        roll, pitch = np.degrees(np.arctan2(R[2, 1], R[2, 2])), np.degrees(-np.arcsin(R[2, 0]))
        assert 0.5 < abs(roll) < 5.0 and 0.5 < abs(pitch) < 5.0, k      # (full 3-D rotation, a few degrees off the flat)
        if k:
            assert np.linalg.norm(P[:3, 3] - sc.poses[k - 1][:3, 3]) <= 1.0, k
    assert np.abs(sc.poses[:, :2, 3]).max() < 4.0   # (every keyframe stands well inside the 12 m patch and sees all of it)
    seen = set()
    for k in range(n):
        for side in (sc.src[k], sc.tgt[k]):
            assert len(side) == 4
            for c in side:
                assert c.dtype == np.float64 and c.ndim == 2 and c.shape[1] == 3 and c.flags.c_contiguous
                assert np.isfinite(c).all()
                if len(c):
                    assert c.tobytes() not in seen   # (no two clouds are equal)
                    seen.add(c.tobytes())
    # in the world frame every cloud lies on the world: the ground at z = 0, nothing outside the patch's box
    for k in (sc.m, sc.q):
        g = LN.move(sc.poses[k], sc.tgt[k][LS.GROUND]) if len(sc.tgt[k][LS.GROUND]) else np.zeros((1, 3))
        assert np.abs(g[:, 2]).max() < 1e-12 and np.abs(g[:, :2]).max() <= LS.GROUND_HALF + 1e-12
    assert len(LS.scan_of(sc, sc.q)) >= 100


@pytest.mark.parametrize("name", SMALL)
def test_small_scenes_stay_small(name):
    sc = LS.scene(name)
    assert sum(len(c) for k in range(len(sc.poses)) for side in (sc.src[k], sc.tgt[k]) for c in side) <= 12 * 2 * sum(LS.BASE_N) + LS.FAR_N
    assert max(len(c) for k in range(len(sc.poses)) for side in (sc.src[k], sc.tgt[k]) for c in side) <= max(LS.BASE_N)


def test_base():
    sc = LS.scene("base")
    assert (len(sc.poses), sc.q, sc.m, sc.window) == (12, 11, 5, None)
    assert LS.window_of(sc) == [3, 4, 5, 6, 7] and LS.span_rows(sc) == list(LS.BASE_N) + [n for n in LS.BASE_N for _ in range(5)]
    assert [len(c) for c in sc.src[11]] == list(LS.BASE_N) and min(LS.target_totals(sc)) >= LS.MIN_POINTS
    # at the true relative pose the score clears the default bounds (0.6, 0.2 m) with room: the device's match has to find it
    truth = LN.t_rel(sc.poses[5], sc.poses[11])
    ov, rmse, inl, pts = LN.score(sc.src[11], LN.assemble(11, 5, 2, sc.poses, sc.tgt), truth, 0.3)
    assert pts == sum(LS.BASE_N) and ov >= 0.9 and rmse <= 0.15


def test_base_keyframes_give_loop_records_of_many_headings():
    """what the init_mode test needs: under PLACE_FOR_LOOPS the place search (tests/place_np.py) finds records among base's
    keyframes, of several yaws, some of them large"""
    import place_np as P
    sc = LS.scene("base")
    db = P.PlaceDB(**LS.PLACE_FOR_LOOPS)
    for k in range(len(sc.poses)):
        db.add(LS.scan_of(sc, k), sc.poses[k], 100 + k)
    yaws = [L["yaw"] for L in db.loops]
    assert len(yaws) >= 5 and len(set(yaws)) >= 4 and max(abs(y) for y in yaws) > 1.0
    assert all(L["d"] < 0.25 for L in db.loops)   # (none near the search's 0.30: the device finds the same records)
    assert not P.PlaceDB().c["exclude_recent"] < 12   # (and by default none: the other tests verify pairs only)


def test_clipped_windows():
    lo, hi = LS.scene("clip_low"), LS.scene("clip_high")
    assert (lo.m, lo.window) == (1, 3) and LS.window_of(lo) == [0, 1, 2, 3, 4]
    assert (hi.m, hi.window) == (hi.q - 1, 3) and LS.window_of(hi) == [7, 8, 9, 10]
    for sc in (lo, hi):
        assert len(LS.window_of(sc)) < 2 * sc.window + 1 and min(LS.target_totals(sc)) >= LS.MIN_POINTS
        # the neighbouring windows the device test tells apart are other windows
        assert LS.window_of(sc, sc.window - 1) != LS.window_of(sc) != LS.window_of(sc, sc.window + 1)


def test_window_zero_and_huge():
    z, h = LS.scene("window_zero"), LS.scene("window_huge")
    assert z.window == 0 and LS.window_of(z) == [5] and min(LS.target_totals(z)) >= LS.MIN_POINTS
    assert h.window == 1 << 20 and len(h.poses) == 12 and LS.window_of(h) == list(range(11))
    assert len(LS.span_rows(h)) == 4 + 4 * 11


def test_spread_sphere():
    sc = LS.scene("spread_sphere")
    assert all(len(sc.tgt[k][LS.SPHERE]) == 4 for k in range(len(sc.poses)))
    assert len(sc.src[sc.q][LS.SPHERE]) >= LS.MIN_POINTS
    assert LS.SPREAD_RUNS == ((5, 1, 12), (5, 0, 4), (0, 1, 8))
    for m, w, want in LS.SPREAD_RUNS:
        tot = LS.target_totals(sc, w, m)
        assert tot[LS.SPHERE] == want and min(tot[:3]) >= LS.MIN_POINTS
    # TLOAM_E_TOO_FEW_POINTS by the clamp alone: 12 can run, 4 and 8 cannot
    assert [want >= LS.MIN_POINTS for _, _, want in LS.SPREAD_RUNS] == [True, False, False]


def test_holes():
    sc = LS.scene("holes")
    ks = LS.window_of(sc)
    assert ks == [3, 4, 5, 6, 7] and LS.HOLES == {(4, LS.PLANAR), (6, LS.EDGE), (6, LS.GROUND)}
    for k in range(len(sc.poses)):
        for kind in range(4):
            assert (len(sc.tgt[k][kind]) == 0) == ((k, kind) in LS.HOLES)
            assert len(sc.filled[k][kind]) == LS.BASE_N[kind]
            if (k, kind) not in LS.HOLES:
                assert sc.tgt[k][kind] is sc.filled[k][kind]
    assert len(LS.span_rows(sc)) == sc.spans == 21 and min(LS.target_totals(sc)) >= LS.MIN_POINTS
    assert LS.target_totals(sc) == [4 * 300, 4 * 400, 4 * 150, 5 * 40]


@pytest.mark.parametrize("name, spans, launches", [("spans_16", 16, 1), ("spans_17", 17, 2), ("spans_33", 33, 3)])
def test_span_counts(name, spans, launches):
    sc = LS.scene(name)
    rows = LS.span_rows(sc)
    assert len(rows) == sc.spans == spans and len(LS.launch_rows(sc)) == launches
    assert len(rows) == sum(1 for c in sc.src[sc.q] if len(c)) + sum(1 for k in LS.window_of(sc) for c in sc.tgt[k] if len(c))
    assert min(LS.target_totals(sc)) >= LS.MIN_POINTS and min(len(c) for c in sc.src[sc.q]) >= LS.MIN_POINTS
    if spans == 17:
        assert len(rows[16:]) == 1   # (a one-span tail)
    assert all(r > 0 for r in rows)


def test_big_rows():
    sc = LS.scene("big_rows")
    ks = LS.window_of(sc)
    assert sc.window == 8 and ks == list(range(17)) and len(ks) == 2 * sc.window + 1
    assert all(len(sc.tgt[k][LS.GROUND]) == LS.BIG_ROWS_N >= 16000 for k in ks)
    rows, per_launch = LS.span_rows(sc), LS.launch_rows(sc)
    assert sum(rows) > LS.ASSEMBLE_THREADS == 262144
    # one launch alone passes the walk's 1024 x 256 threads: its threads take a second row, across span boundaries
    assert rows[16:32] == [LS.BIG_ROWS_N] * 16 and per_launch[1] == 16 * LS.BIG_ROWS_N > LS.ASSEMBLE_THREADS
    assert 16 * 16000 < LS.ASSEMBLE_THREADS   # (why 16 000 a keyframe was not enough)
    assert min(LS.target_totals(sc)) >= LS.MIN_POINTS


def test_far_points():
    sc = LS.scene("far_points")
    src = sc.src[sc.q][LS.SPHERE]
    assert len(src) == LS.BASE_N[LS.SPHERE] + LS.FAR_N and [len(c) for c in sc.src[sc.q]][:3] == list(LS.BASE_N[:3])
    truth = LN.t_rel(sc.poses[sc.m], sc.poses[sc.q])
    tgt = LN.assemble(sc.q, sc.m, LS.DEFAULT_WINDOW, sc.poses, sc.tgt)
    d = np.sqrt(LN.nearest_d2(LN.move(truth, src), tgt[LS.SPHERE]))
    # the far points are many sphere cells (0.5 m) from every sphere target: more than 3 m apart means more than 1.7 m, three
    # cells, along some axis, so a reach of 1 cannot find a target for them; and a reach of ceil(5 / 0.5) can
    assert (d[-LS.FAR_N:] > LS.FAR_MIN + 0.1).all() and (d[-LS.FAR_N:] < LS.FAR_MAX - 0.1).all()
    assert LS.FAR_MIN / np.sqrt(3.0) > 3 * 0.5 * (1.0 + 1e-6)
    assert (d[:-LS.FAR_N] < 0.3).all()   # (the blobs' own points are inliers at the default distance)
    for kind in range(3):                # (and no other kind has a point that far from its targets)
        dk = np.sqrt(LN.nearest_d2(LN.move(truth, sc.src[sc.q][kind]), tgt[kind]))
        assert dk.max() < 1.0


def test_big_source_and_nine_sphere():
    b, n = LS.scene("big_source"), LS.scene("nine_sphere")
    assert len(b.src[b.q][LS.GROUND]) == LS.SCORE_THREADS + 300 > 65536
    assert [len(c) for i, c in enumerate(b.src[b.q]) if i != LS.GROUND] == [300, 150, 40]
    assert len(n.src[n.q][LS.SPHERE]) == 9 < LS.MIN_POINTS and min(LS.target_totals(n)) >= LS.MIN_POINTS
    assert [len(c) for c in n.src[n.q]][:3] == [300, 400, 150]
