"""CPU: tests/loop_np.py, the yardstick of the loop verification tests, against independent references -- the window at its
clamps, T_rel / rigid_inverse / mat_mul / move against np.longdouble within bounds derived from the length of their sums, the
score against a brute-force longdouble nearest neighbour, and score_device_order against score and against hand-made sums.

Rounding bounds: u = 2^-53, gamma(n) = n u / (1 - n u) (a sum of n terms each rounded at most n times: the product and the
additions after it).  Every bound below is gamma(n) times the sum of the absolute values of the exact terms, n read off the
expression, plus what the inputs themselves contribute; none is taken from what loop_np returns."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import loop_np as LN  # noqa: E402
import loop_scenes as LS  # noqa: E402

LD = np.longdouble
U = 2.0 ** -53


def gamma(n):
    return n * U / (1.0 - n * U)


def ld(a):
    return np.asarray(a, float).astype(LD)


def poses():
    """rigid poses with full 3-D rotation, angles of every size, translations of a few metres"""
    rng = np.random.default_rng(17)
    out = [LS.pose(*p) for p in LS.TRACK_12]
    for _ in range(12):
        a = rng.uniform(-180.0, 180.0, 3)
        out.append(LS.pose(*rng.uniform(-8.0, 8.0, 3), a[0], a[1] / 2, a[2]))
    return out


def inverse_ld(P):
    """inv(P) in longdouble: the double inverse refined by two Newton steps X <- X (2 I - P X), each squaring the residual"""
    X = ld(np.linalg.inv(P))
    P, I2 = ld(P), 2 * np.eye(4, dtype=LD)
    for _ in range(2):
        X = X @ (I2 - P @ X)
    assert np.abs(P @ X - np.eye(4, dtype=LD)).max() < 1e-17
    return X


def rigid_ld(P):
    """(R^T, -R^T t) in longdouble: what rigid_inverse means, exactly"""
    P = ld(P)
    X = np.eye(4, dtype=LD)
    X[:3, :3] = P[:3, :3].T
    X[:3, 3] = -(P[:3, :3].T @ P[:3, 3])
    return X


# ---- window -----------------------------------------------------------------------------------------------------------------
def test_window_at_the_clamps():
    assert LN.window(11, 5, 2) == [3, 4, 5, 6, 7]
    assert LN.window(11, 1, 3) == [0, 1, 2, 3, 4]          # m - w < 0
    assert LN.window(11, 0, 1) == [0, 1]
    assert LN.window(11, 9, 3) == [6, 7, 8, 9, 10]         # m + w > q - 1
    assert LN.window(11, 10, 3) == [7, 8, 9, 10]           # m = q - 1: nothing above m
    assert LN.window(11, 10, 0) == [10]
    assert LN.window(11, 5, 0) == [5]                      # w = 0
    assert LN.window(11, 5, 1 << 20) == list(range(11))    # w larger than q
    assert LN.window(1, 0, 1 << 20) == [0]
    for q in range(1, 9):
        for m in range(q):
            for w in range(0, 10):
                ks = LN.window(q, m, w)
                assert ks == [k for k in range(q) if abs(k - m) <= w] and m in ks and q not in ks


# ---- the transforms -------------------------------------------------------------------------------------------------------
def test_mat_mul_against_longdouble():
    Ps = poses()
    for A, B in zip(Ps, Ps[1:]):
        got = LN.mat_mul(A, B)
        exact = ld(A) @ ld(B)
        # ((a0 b0 + a1 b1) + a2 b2) + a3 b3: the first product is rounded once and passes three additions -> gamma(4)
        bound = gamma(4) * (np.abs(ld(A)) @ np.abs(ld(B)))
        assert (np.abs(ld(got) - exact) <= bound).all()


def test_rigid_inverse_against_longdouble():
    for P in poses():
        got = LN.rigid_inverse(P)
        assert LS.bits(got[:3, :3]) == LS.bits(P[:3, :3].T) and LS.bits(got[3]) == LS.bits([0.0, 0.0, 0.0, 1.0])
        exact = rigid_ld(P)
        # -((r0 t0 + r1 t1) + r2 t2): three terms, the first rounded three times -> gamma(3)
        bound = gamma(3) * (np.abs(ld(P[:3, :3])).T @ np.abs(ld(P[:3, 3])))
        assert (np.abs(ld(got[:3, 3]) - exact[:3, 3]) <= bound).all()


def test_t_rel_against_the_longdouble_inverse():
    Ps = poses()
    worst = 0.0
    for Pm, Pk in zip(Ps, Ps[3:] + Ps[:3]):
        got = LN.t_rel(Pm, Pk)
        truth = inverse_ld(Pm) @ ld(Pk)
        A, B = rigid_ld(Pm), ld(Pk)
        # the restatement's own rounding: gamma(4) per entry of the product (four-term sums), plus, in the last column, the
        # gamma(3) of the inverse's translation (three-term sums), which the product multiplies by 1 and rounds again
        e = gamma(3) * (np.abs(ld(Pm[:3, :3])).T @ np.abs(ld(Pm[:3, 3])))
        absA = np.abs(A)
        absA[:3, 3] += e
        bound = gamma(4) * (absA @ np.abs(B))
        bound[:3, 3] += e
        # the inputs' own share: a pose's rotation is a rotation rounded to double, so (R^T, -R^T t) is not exactly inv(P);
        # the difference, known from the inputs in longdouble, times P_k
        bound += np.abs(inverse_ld(Pm) - A) @ np.abs(B)
        err = np.abs(ld(got) - truth)
        assert (err <= bound).all()
        worst = max(worst, float((err / (U * np.maximum(np.abs(truth), 1.0))).max()))
    print(f"t_rel: worst error {worst:.2f} u of max(|entry|, 1)")


def test_move_against_longdouble():
    rng = np.random.default_rng(5)
    for T in poses():
        p = rng.uniform(-30.0, 30.0, (257, 3))
        got = LN.move(T, p)
        R, t = ld(T[:3, :3]), ld(T[:3, 3])
        exact = ld(p) @ R.T + t
        # ((R0 x + R1 y) + R2 z) + t: four terms, the first product rounded once and passing three additions -> gamma(4)
        bound = gamma(4) * (np.abs(ld(p)) @ np.abs(R).T + np.abs(t))
        assert (np.abs(ld(got) - exact) <= bound).all()


def test_assemble_is_window_t_rel_and_move():
    sc = LS.scene("holes")
    got = LN.assemble(sc.q, sc.m, sc.window, sc.poses, sc.tgt)
    for kind in range(4):
        parts = [LN.move(LN.t_rel(sc.poses[sc.m], sc.poses[k]), sc.tgt[k][kind]) for k in (3, 4, 5, 6, 7)
                 if (k, kind) not in LS.HOLES]
        assert LS.bits(got[kind]) == LS.bits(np.concatenate(parts))


# ---- the score --------------------------------------------------------------------------------------------------------------
def random_pair(seed, n_src=(700, 900, 300, 50), n_tgt=(900, 900, 500, 80)):
    rng = np.random.default_rng(seed)
    src = [rng.random((n, 3)) * 4.0 for n in n_src]
    tgt = [rng.random((n, 3)) * 4.0 for n in n_tgt]
    T = LS.pose(0.01, 0.02, -0.01, 0.4, -0.3, 0.2)
    return src, tgt, T


def test_score_against_brute_force_longdouble():
    dist = 0.3
    for seed in range(3):
        src, tgt, T = random_pair(seed, (200, 260, 90, 30), (300, 280, 150, 40))
        inl, pts = 0, 0
        for kind in range(4):
            p = ld(src[kind]) @ ld(T[:3, :3]).T + ld(T[:3, 3])
            d = ((p[:, None, :] - ld(tgt[kind])[None, :, :]) ** 2).sum(axis=2).min(axis=1)
            # no nearest distance within rounding of inlier_dist: coordinates below 8, so the double path's d^2 is off by less
            # than 2 |d| sqrt(3) gamma(4) 32 + gamma(3) d^2 < 1e-13; the guard leaves four orders of magnitude
            assert (np.abs(d - LD(dist) * LD(dist)) > 1e-9).all()
            inl += int((d < LD(dist) * LD(dist)).sum())
            pts += len(p)
        ov, rmse, got_inl, got_pts = LN.score(src, tgt, T, dist)
        assert (got_inl, got_pts) == (inl, pts) and 0 < inl < pts
        assert ov == inl / pts and np.isfinite(rmse) and 0.0 < rmse < dist


def test_score_without_targets_or_inliers():
    src, tgt, T = random_pair(0)
    empty = [np.zeros((0, 3))] * 4
    for f in (LN.score, LN.score_device_order):
        ov, rmse, inl, pts = f(src, empty, T, 0.3)
        assert (ov, inl, pts) == (0.0, 0, sum(len(c) for c in src)) and rmse == np.inf
        ov, rmse, inl, pts = f(src, tgt, T, 1e-9)
        assert (ov, inl) == (0.0, 0) and rmse == np.inf
        one = [tgt[0], empty[1], tgt[2], empty[3]]   # (kinds without targets count their points, none an inlier)
        ov, rmse, inl, pts = f(src, one, T, 10.0)
        assert inl == len(src[0]) + len(src[2]) and pts == sum(len(c) for c in src) and ov == inl / pts


def test_device_order_agrees_with_score_and_is_another_order():
    differ = 0
    cases = [random_pair(seed) for seed in range(8)]
    for name in ("base", "window_zero", "holes"):
        sc = LS.scene(name)
        w = LS.DEFAULT_WINDOW if sc.window is None else sc.window
        cases.append((sc.src[sc.q], LN.assemble(sc.q, sc.m, w, sc.poses, sc.tgt), LN.t_rel(sc.poses[sc.m], sc.poses[sc.q])))
    for src, tgt, T in cases:
        a, b = LN.score(src, tgt, T, 0.3), LN.score_device_order(src, tgt, T, 0.3)
        assert a[0] == b[0] and a[2:] == b[2:] and a[2] > 0
        assert abs(a[1] - b[1]) <= 1e-12 * a[1]
        differ += float(a[1]).hex() != float(b[1]).hex()
    assert differ >= 1   # (the orders really differ)


def test_device_sum_by_hand():
    # one wave's butterfly: lane 0 ends with ((((v0 + v32) + (v16 + v48)) + ...): checked against the tree written out
    rng = np.random.default_rng(3)
    v = rng.random(64)
    t = v.copy()
    for off in (32, 16, 8, 4, 2, 1):
        t = np.array([t[i] + t[i ^ off] for i in range(64)])
    assert len(set(t.tolist())) == 1   # (every stage adds a pair commutatively: all lanes hold the same bits)
    c, s = LN.device_sum(np.ones(64, bool), v)
    assert (c, s) == (64.0, t[0])
    # four waves and two blocks: ((w0 + w1) + w2) + w3, then 0.0 + b0 + b1
    v = rng.random(512)
    w = []
    for i in range(8):
        t = v[64 * i:64 * i + 64].copy()
        for off in (32, 16, 8, 4, 2, 1):
            t = t + t[np.arange(64) ^ off]
        w.append(t[0])
    b0, b1 = ((w[0] + w[1]) + w[2]) + w[3], ((w[4] + w[5]) + w[6]) + w[7]
    assert LN.device_sum(np.ones(512, bool), v) == (512.0, (0.0 + b0) + b1)
    # what is not kept is not added
    keep = rng.random(512) < 0.5
    c, s = LN.device_sum(keep, np.where(keep, v, np.inf))
    assert (c, s) == (float(keep.sum()), LN.device_sum(np.ones(512, bool), np.where(keep, v, 0.0))[1])


def test_a_second_turn_gives_threads_0_to_6_two_points():
    n = LN.SCORE_THREADS + 7
    assert LN.SCORE_THREADS == 65536
    # points t and 65 536 + t belong to thread t: with 1.0 and u = 2^-53 the thread's own sum 1 + u rounds back to 1, and the
    # seven threads give exactly 7.  Were the late points summed anywhere else first, their 7 u (more than half an ulp of 7)
    # would round the total up
    d = np.zeros(n)
    d[:7] = 1.0
    d[LN.SCORE_THREADS:] = U
    assert (0.0 + 7 * U) + 7.0 > 7.0
    c, s = LN.device_sum(np.ones(n, bool), d)
    assert (c, s) == (float(n), 7.0)
    # and through score_device_order: a kind of 65 536 + 7 source points
    rng = np.random.default_rng(9)
    src = [rng.random((20, 3)), rng.random((n, 3)), rng.random((20, 3)), rng.random((20, 3))]
    tgt = [rng.random((40, 3)) for _ in range(4)]
    a, b = LN.score(src, tgt, np.eye(4), 0.3), LN.score_device_order(src, tgt, np.eye(4), 0.3)
    assert a[0] == b[0] and a[2:] == b[2:] and b[3] == n + 60 and abs(a[1] - b[1]) <= 1e-12 * a[1]
    d2 = LN.nearest_d2(src[1], tgt[1])
    keep = d2 < 0.3 * 0.3
    assert keep[:7].any() or keep[LN.SCORE_THREADS:].any()
    per_thread = np.zeros(LN.SCORE_THREADS)
    per_thread[:] = np.where(keep[:LN.SCORE_THREADS], d2[:LN.SCORE_THREADS], 0.0)
    per_thread[:7] = per_thread[:7] + np.where(keep[LN.SCORE_THREADS:], d2[LN.SCORE_THREADS:], 0.0)
    assert LN.device_sum(keep, d2)[1] == LN.device_sum(np.ones(LN.SCORE_THREADS, bool), per_thread)[1]
