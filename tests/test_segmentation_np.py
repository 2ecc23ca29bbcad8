"""The numpy restatement of the segmentation node (tests/segmentation_np.py) on hand-made inputs: every quirk of
segmentation.cpp the device has to reproduce, and the committed golden files."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import segmentation_np as S  # noqa: E402

CFG = S.SegCfg()


def test_near_filter_compares_the_norm_with_nine_metres():
    xyz = np.array([[8.99, 0, 0], [9.0, 0, 0], [0, 5.0, 0], [np.nan, 20, 0], [np.inf, 0, 0], [0, 0, -12.0]])
    kept, _ = S.near_filter(xyz, CFG)
    assert kept.tolist() == [1, 5]


def test_section_bounds_of_the_shipped_config():
    b = S.section_bounds(CFG)
    assert len(b) == 2                      # ring 62 never appends: the angle stops advancing from ring 52 on
    assert abs(b[0] - 5.6941) < 1e-4 and abs(b[1] - 14.5082) < 1e-4
    assert all(float(np.float32(v)) == v for v in b)   # float-rounded (static_cast<float>, :211)
    r = np.array([1.0, 5.69, 5.7, 14.5, 14.6, 200.0])
    assert S.get_section(r, b, 3).tolist() == [0, 0, 1, 1, 2, 2]   # the missing third bound never matches


def test_fast_atan2_and_the_360_drop():
    a = S.fast_atan2(np.float32([1, 1, -1, -1, 0]), np.float32([1, -1, -1, 1, 1]))
    np.testing.assert_allclose(a, [45, 135, 225, 315, 0], atol=0.02)
    # y > 0 (so -y < 0) with |y| / x below ~2.6e-7: 360.0f -- in no region, out of ground AND object
    P = np.array([[20.0, 1e-6, -1.7], [20.0, 1e-5, -1.7], [20.0, -1e-6, -1.7]])
    reg, _ = S.region_of(P, S.section_bounds(CFG), CFG)
    assert reg.tolist() == [-1, 3 * 3 + 2, 0 * 3 + 2]
    assert S.fast_atan2(np.float32(-1e-6), np.float32(20.0)) == np.float32(360.0)


def test_ring_count_saturates_at_63():
    q = np.array(([1, 2, 3, 4] * 70), np.int32)
    r = S.rings(q)
    assert r.max() == 63 and r[0] == 0
    np.testing.assert_array_equal(r, S.rings_literal(q))
    rng = np.random.default_rng(0)
    q = rng.integers(1, 5, 5000).astype(np.int32)
    np.testing.assert_array_equal(S.rings(q), S.rings_literal(q))
    assert S.rings_literal(np.array([1, 4, 1], np.int32)).tolist() == [0, 0, 1]   # the first point's prev_q is 0


def _flat_region(m, rng, z=-1.73):
    P = np.column_stack([rng.uniform(10, 30, m), rng.uniform(1, 20, m), z + rng.normal(0, 0.01, m)])
    return P


def test_region_dropped_at_three_seeds():
    rng = np.random.default_rng(1)
    P = _flat_region(31, rng)               # subsample k % 10 == 0: k = 0, 10, 20, 30 -> 4 seeds
    g, v, _ = S.ground_region(P, CFG)
    assert len(g) > 0
    g, v, _ = S.ground_region(P[:30], CFG)  # 3 seeds: the region is dropped from both outputs
    assert len(g) == 0 and len(v) == 0


def test_skipped_iteration_keeps_the_last_fit_set_and_no_vertical_point(monkeypatch):
    # five seeds (k = 0, 10, ..., 40); the plane z = -1.73 leaves only k = 0, 5, 10 of the k % 5 == 0 points within 0.3 m:
    # iteration 0's fit set has 3 points, so iterations 1 and 2 are skipped (:671) -- the region emits those 3 as ground
    # and no vertical point, although most of its points are 0.35 m off the plane
    m = 45
    k = np.arange(m)
    P = np.column_stack([10.0 + 0.2 * k, 2.0 + 0.1 * (k % 7), np.full(m, -1.73 + 0.35)])
    P[[0, 5, 10], 2] = -1.73
    monkeypatch.setattr(S, "find_best_plane", lambda F: np.array([0.0, 0.0, 1.0, 1.73]))
    g, v, _ = S.ground_region(P, CFG)
    assert g.tolist() == [0, 5, 10] and len(v) == 0
    # without the skip (a plane that keeps more): the last iteration splits ground from vertical
    monkeypatch.setattr(S, "find_best_plane", lambda F: np.array([0.0, 0.0, 1.0, 1.73 - 0.35]))
    g, v, _ = S.ground_region(P, CFG)
    assert g.tolist() == [i for i in range(m) if i not in (0, 5, 10)] and v.tolist() == [0, 5, 10]


def test_zero_normal_makes_every_point_ground():
    P = np.array([[10.0, 1.0, -1.7]] * 5)
    pl = S.find_best_plane(P)
    assert pl.tolist() == [0.0, 0.0, 0.0, 0.0] or np.all(pl == 0)
    assert (S.plane_dist(P + 3.0, pl) == 0).all()


def test_first_frame_min_polar_and_the_zero_voxel_of_far_points():
    P = np.array([[20.0, 1.0, 0.5], [30.0, -2.0, -1.0], [150.0, 10.0, 1.0]])
    V1 = S.polar_voxels(P, CFG, first_frame=True)
    V2 = S.polar_voxels(P, CFG, first_frame=False)
    assert V1["min_polar"] == 5.0 and V2["min_polar"] == 0.0
    assert V1["bounds"][0] == 5.0 + (0.35 - 0.0004) and V2["bounds"][0] == 0.35 - 0.0004
    # the point beyond 120 m keeps polarCor (0, 0, 0): polar 0, azimuth 0, pitch round(-minPitch / deltaP)
    assert V1["pol"][2] == 0 and V1["az"][2] == 0
    assert V1["pit"][2] == S.std_round(np.array([-V1["min_pitch"] / 1.2]))[0]


def test_one_way_edges_part_the_literal_loop_from_the_components():
    # voxels along the azimuth only: a (az 0), b (az 3), i (az 1), j (az 2) in this order.  a labels {a, i}, b labels
    # {b, j}; i and j are skipped as already labelled, so the literal loop never walks i -- j
    V = dict(pol=np.zeros(4, np.int64), pit=np.zeros(4, np.int64), az=np.array([10, 13, 11, 12]), polarNum=1, width=301,
             height=0)
    lit = S.dcvc_literal(V)
    comp = S.dcvc_components(V)
    assert len(set(S.canonical(lit).tolist())) == 2
    assert len(set(S.canonical(comp).tolist())) == 1
    assert S.partition_differs(lit, comp)
    np.testing.assert_array_equal(S.canonical(S.dcvc_literal_fast(V)), S.canonical(lit))
    # azimuth column 0 sees column 300, column 300 does not see 0
    V = dict(pol=np.zeros(2, np.int64), pit=np.zeros(2, np.int64), az=np.array([300, 0]), polarNum=1, width=301, height=0)
    assert len(set(S.canonical(S.dcvc_literal(V)).tolist())) == 1   # 0 walks into 300 (it comes second)
    V = dict(pol=np.zeros(2, np.int64), pit=np.zeros(2, np.int64), az=np.array([0, 300]), polarNum=1, width=301, height=0)
    assert len(set(S.canonical(S.dcvc_literal(V)).tolist())) == 1   # 0 labels 300 as its neighbour
    # a point in row height + 1 does not see its own voxel: two of them with no other neighbour stay apart
    V = dict(pol=np.zeros(2, np.int64), pit=np.array([1, 1]), az=np.array([5, 5]), polarNum=1, width=301, height=0)
    assert len(set(S.canonical(S.dcvc_components(V)).tolist())) == 2


def test_cluster_kept_strictly_above_min_seg_and_ordered():
    lab = np.array([0] * 80 + [1] * 81 + [2] * 85 + [3] * 81)
    cl = S.label_analysis(lab, 80)
    assert [len(c) for c in cl] == [85, 81, 81]
    assert cl[1][0] == 80 and cl[2][0] == 80 + 81 + 85     # equal sizes: smallest member first
    assert all((np.diff(c) > 0).all() for c in cl)


def _ring(m, rng):
    t = np.linspace(0, 2 * np.pi, m, endpoint=False)
    R = np.column_stack([20 * np.cos(t), 20 * np.sin(t), np.zeros(m)])
    R[rng.choice(np.arange(10, m - 10), 12, replace=False), 0] += 3.0     # spikes: high curvature
    return R


def test_last_entry_of_every_sector_is_in_neither_output():
    rng = np.random.default_rng(4)
    m = 200
    R = _ring(m, rng)
    e, g = S.extract_edges(R, np.zeros(m, np.int32), CFG)
    tp = m - 10
    L = tp // 6
    lost = [L * (j + 1) - 1 + 5 for j in range(5)] + [tp - 1 + 5]
    assert not (set(lost) & (set(e.tolist()) | set(g.tolist())))
    assert len(set(e.tolist()) & set(g.tolist())) == 0
    # rings below ringMinNum emit nothing
    e2, g2 = S.extract_edges(R[:130], np.zeros(130, np.int32), CFG)
    assert len(e2) == 0 and len(g2) == 0


def test_picked_neighbours_are_in_neither_output():
    m = 40
    R = np.column_stack([np.arange(m) * 0.1, np.full(m, 20.0), np.zeros(m)])   # consecutive distance^2 0.01 <= 0.05
    R[20, 1] += 2.0                                                            # one spike
    ent = np.arange(5, 35)
    cv = S.curvature(R)[: len(ent)]
    edge, general = S.extract_from_section(R, ent, cv)
    assert edge[0] == 20
    # the spike's neighbours are 2 m away: no mark; mark the flat neighbours of the second pick instead
    marked = set(ent.tolist()) - set(edge) - set(general)
    for p in edge:
        for k in range(1, 6):
            d = R[p + k] - R[p + k - 1]
            if d @ d > 0.05:
                break
            assert p + k not in general
    assert marked or len(edge) + len(general) == len(ent)


def test_picks_stop_at_the_21st():
    m = 400
    rng = np.random.default_rng(6)
    R = np.column_stack([np.arange(m) * 1.0, np.full(m, 20.0), np.zeros(m)])
    R[::3, 1] += rng.uniform(1, 2, len(R[::3]))                                 # curvature everywhere, no marks
    ent = np.arange(5, m - 5)
    cv = S.curvature(R)
    edge, general = S.extract_from_section(R, ent, cv)
    assert len(edge) == 20
    assert len(edge) + len(general) == len(ent) - 1   # the 21st pick is in neither list


def test_vectorised_dcvc_matches_the_literal_loop_on_small_scans():
    rng = np.random.default_rng(7)
    for trial in range(6):
        n = 300
        P = np.column_stack([rng.uniform(-30, 30, n), rng.uniform(-30, 30, n), rng.uniform(-2, 3, n)])
        P = P[np.linalg.norm(P, axis=1) > 9]
        V = S.polar_voxels(P, CFG, first_frame=bool(trial % 2))
        a, b = S.dcvc_literal(V), S.dcvc_literal_fast(V)
        np.testing.assert_array_equal(S.canonical(a), S.canonical(b))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_committed_golden_files_reproduce(seed):
    import make_seg_golden as MG
    g = np.load(os.path.join(HERE, "golden", f"seg_{seed}.npz"))
    xyz = MG.golden_scan(seed)
    assert MG.digest(xyz) == str(g["digest"])
    o = S.segment(xyz, first_frame=True)
    assert o["status"] == 0 and not o["margins"]
    np.testing.assert_array_equal(o["ring"], g["ring"])
    for k in ("ground", "object", "segmented", "label", "edge", "general"):
        np.testing.assert_array_equal(o[k], g[k], err_msg=k)
    assert o["boxes"].tobytes() == g["boxes"].tobytes()


def test_unsupported_models_are_invalid():
    o = S.segment(np.zeros((10, 3)), S.SegCfg(sensorModel=16))
    assert o["status"] == S.STATUS_INVALID
    o = S.segment(np.zeros((0, 3)))
    assert o["status"] == S.STATUS_TOO_FEW
