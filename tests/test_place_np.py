"""The numpy restatement of place recognition (tests/place_np.py) without a GPU: the properties the device
is checked against it by -- the integer image of the bin maximum, the declared summation orders, the shift search and its yaw
sign, the margin report of the scenes the GPU tests use, the keyframe policy."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "golden")]

import place_np as P  # noqa: E402
import make_seg_golden as MG  # noqa: E402
from tloam_amd import synth_hdl64 as G  # noqa: E402
from tloam_amd import synth_revisit as RV  # noqa: E402


def test_integer_image_preserves_order_and_round_trips():
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.normal(0, 5, 1000), [-0.0, 0.0, -1e-300, 1e-300, -1e300, 1e300, -np.inf, np.inf]])
    k = P.okey(v)
    assert np.all(k > 0)   # 0 is the empty bin
    o = np.argsort(v, kind="stable")
    assert np.all(np.diff(k[o].astype(object)) >= 0)
    assert P.from_okey(k).tobytes() == v.tobytes()
    assert P.from_okey(np.zeros(3, np.uint64)).tobytes() == np.zeros(3).tobytes()


def test_bins_follow_the_declared_grid():
    R, S, rmax = 20, 60, 80.0
    # one return in the middle of every ring / sector pair
    r = (np.arange(R) + 0.5) * (rmax / R)
    a = (np.arange(S) + 0.5) * (2 * np.pi / S) - np.pi
    rr, aa = np.meshgrid(r, a, indexing="ij")
    z = np.arange(R * S, dtype=float).reshape(R, S) * 0.01 - 3.0
    p = np.column_stack([(rr * np.cos(aa)).ravel(), (rr * np.sin(aa)).ravel(), z.ravel()])
    d, _, _ = P.describe(p)
    assert np.array_equal(d, z + 2.0)
    # an empty bin is 0.0, a negative maximum stays negative, the maximum wins, the radius and non-finite gates
    q = np.array([[1.0, 0.1, -5.0], [1.0, 0.1, -4.0], [0.0, 0.0, 7.0], [80.0, 0.0, 1.0], [79.0, 0.0, np.nan], [np.inf, 1.0, 0.0]])
    d, rk, sk = P.describe(q)
    i, j = 0, int((math.atan2(0.1, 1.0) + math.pi) // (2 * math.pi / 60))
    assert d[i, j] == -2.0 and np.count_nonzero(d) == 1


def test_keys_use_the_declared_summation_order():
    rng = np.random.default_rng(1)
    d = rng.normal(0, 1, (20, 60)) * 10.0 ** rng.integers(-8, 9, (20, 60))
    rk, sk = P.keys(d)
    for i in range(20):
        acc = 0.0
        for j in range(60):
            acc = acc + float(d[i, j])
        assert rk[i] == acc / 60.0
    for j in range(60):
        acc = 0.0
        for i in range(20):
            acc = acc + float(d[i, j])
        assert sk[j] == acc / 20.0
    # (and the pairwise sum would not have given these bits)
    assert any(np.sum(d[i]) / 60.0 != rk[i] for i in range(20))


@pytest.mark.parametrize("k", (0, 1, 17, 59))
def test_rolled_columns_give_their_shift_at_zero(k):
    W = G.make_street(1)
    p, _ = G.scan(W, G.trajectory(1)[0], n_az=600, seed=5, rings=np.arange(0, 64, 2))
    d, _, _ = P.describe(p)
    c = np.roll(d, k, axis=1)   # c[:, j] = d[:, j - k]: the candidate's column j + k matches the query's j
    ds = P.shift_distances(d, c)
    assert int(np.argmin(ds)) == k
    assert abs(ds[k]) < 1e-12
    assert np.sort(ds)[1] > 0.01


def test_yaw_is_the_query_heading_relative_to_the_match():
    """the same place seen with the sensor turned by +psi: the best shift's yaw is +psi (within one sector)"""
    W = G.make_street(2)
    base = G.trajectory(1)[0]
    for psi in (0.5, -1.2, 2.9, np.pi - 0.02):
        T = base.copy()
        c, s = np.cos(psi), np.sin(psi)
        T[:2, :2] = [[c, -s], [s, c]]
        a, _ = G.scan(W, base, n_az=600, seed=1, rings=np.arange(0, 64, 2))
        b, _ = G.scan(W, T, n_az=600, seed=2, rings=np.arange(0, 64, 2))
        da, db = P.describe(a)[0], P.describe(b)[0]
        ds = P.shift_distances(db, da)   # query b (turned), match a
        yaw = P.yaw_of(int(np.argmin(ds)), 60)
        err = (yaw - RV.relative_yaw(T, base) + np.pi) % (2 * np.pi) - np.pi
        assert abs(err) <= 2 * np.pi / 60, (psi, yaw)


def test_margin_report_lists_boundary_returns():
    R, S, rmax = 20, 60, 80.0
    on_ring = np.array([[4.0, 0.0, 0.0]])   # r = 4 m = one ring width: a boundary
    ang = 7 * (2 * np.pi / S) - np.pi       # a sector boundary
    on_sector = np.array([[10.0 * np.cos(ang), 10.0 * np.sin(ang), 0.0]])
    inside = np.array([[10.0 * np.cos(ang + 0.01), 10.0 * np.sin(ang + 0.01), 0.0]])
    p = np.vstack([inside, on_ring, on_sector, [[90.0, 0.0, 0.0]]])
    assert list(P.margins(p)) == [1, 2]


def test_the_gpu_scenes_have_no_margins():
    for seed in MG.SEEDS:
        assert len(P.margins(MG.golden_scan(seed))) == 0, seed
    scans, _, _ = RV.out_and_back(3, seed=0, n_az=600, rings=np.arange(0, 64, 2))
    for s in scans:
        assert len(P.margins(s)) == 0


def test_search_ties_and_exclusion():
    db = P.PlaceDB(exclude_recent=2, num_candidates=2, dist_thres=0.5)
    rng = np.random.default_rng(3)
    d0 = np.abs(rng.normal(0, 1, (20, 60)))
    for f in range(4):   # the same descriptor four times: every candidate ties; ids and shifts go to the lowest
        db.add_described(d0, *P.keys(d0), np.eye(4), 10 + f)
    assert db.candidates(3) == [0, 1]
    assert [(L["query"], L["match"], L["shift"], L["query_frame"], L["match_frame"]) for L in db.loops] == \
        [(2, 0, 0, 12, 10), (3, 0, 0, 13, 10)]
    assert db.candidates(0) == [] and db.candidates(1) == []


def test_keyframe_policy():
    A = np.eye(4)
    B = np.eye(4); B[:3, 3] = [0.6, 0.0, 0.0]
    assert not P.moved(A, B, 1.0, 0.2)
    B[:3, 3] = [0.6, 0.8, 0.0]
    assert P.moved(A, B, 1.0, 0.2)   # exactly 1.0 m
    c, s = np.cos(0.21), np.sin(0.21)
    C_ = np.eye(4); C_[:2, :2] = [[c, -s], [s, c]]
    assert P.moved(A, C_, 1.0, 0.2) and not P.moved(A, C_, 1.0, 0.22)
    db = P.PlaceDB()
    assert db.is_keyframe(A)


def test_generator_revisits_and_one_way():
    poses, leg = RV.out_and_back_poses(10, step=2.0, lane=0.8)
    out = [T for T, g in zip(poses, leg) if g == 0]
    back = [T for T, g in zip(poses, leg) if g == 1]
    for T in back:
        near = min(np.linalg.norm(T[:3, 3] - U[:3, 3]) for U in out)
        assert near < 1.5
        assert min(abs(RV.relative_yaw(T, U)) for U in out) > np.pi - 0.05
    for T, U in zip(out, back[::-1]):
        assert abs(T[1, 3] - U[1, 3]) <= 1.0   # the return lane within 1 m of the outbound one
    ow = RV.one_way_poses(10)
    assert all(ow[k + 1][0, 3] - ow[k][0, 3] == 2.0 for k in range(9))
