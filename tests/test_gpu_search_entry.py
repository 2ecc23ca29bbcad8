"""The entry, the kind handling and the unpack of the correspondence search (tl_nn.hip, tl_knn.hpp) on small hand-made frames,
through tloam_sm_* / tloam_scan_match and the set getters, against the oracle, bit for bit: the correspondence index lists
(which source slots carry a factor is the search's flag word; in a whole tloam_scan_match of a small frame the one-launch Solve
compacts from the flag BYTES instead) and the records a, b, d.

The sixteen-lane search cuts the source slots into waves of four queries.  What a wave does at its entry -- which kind its
queries are, whether the kind is active and has a grid, whether the gate of the device-driven loop is open -- and how the kept
list is unpacked when it is shorter than K are the cases here.  `_census` counts them with numpy BEFORE anything is handed to
the GPU: a frame that misses a case fails in a test that needs no GPU, not in a kernel.
  * kind boundaries at positions 1, 2 and 3 of a group of four slots, and all at 0; last groups of one, two and three queries
  * inactive kinds (factor_num 3 and 2): no factor, nothing counted -- except that the sphere builder, where it runs, counts the
    points without a neighbour --, beside active kinds in one group of four
  * lists shorter than K: queries with 0, 1, 3, 4 and 5 targets in their 27 cells (K = 5) and with 0 and 1 (K = 1), queries
    outside the grid
  * the gate: a frame whose loop ends after two of its four outer iterations (the searches enqueued for the others find their
    gate closed and return at their entry; had one run, the set would be rebuilt at the final pose), frames where the pose
    moves and the gated searches run
  * a kind of 4100 source points: no flag bytes (kFlagbStride = 4096), so the finish rides on the next search
    (k_build_finish_small; tl_forms.hpp decides, tests/test_frame_forms_host.py holds the decision) -- same results as stepwise
  * just above 16384 source slots: four lanes per query, the same unpack
  * the PCA pass (K = 20) on a cloud where many points have fewer than twenty neighbours
"""
import functools

import numpy as np
import pytest

from conftest import pose_delta
from oracle import binding as ob
from test_gpu_walk_pieces import K_OF_KIND, PLANAR, SPHERE, WIDE_LIMIT, _cells, _grid_of, _radii, _rows

FLAGB_STRIDE = 4096           # flag bytes per kind (tl_forms.hpp kFlagbStride)

# source points per kind (planar, ground, edge, sphere) of the hand-made frames
COUNTS = {
    "b123": (41, 41, 41, 14),       # boundaries at 41, 82, 123: positions 1, 2, 3; 137 slots: a last group of one
    "b000": (40, 40, 40, 18),       # boundaries at multiples of four; 138 slots: a last group of two
    "b313": (43, 42, 42, 12),       # boundaries at 43, 85, 127: positions 3, 1, 3; 139 slots: a last group of three
    "ride": (4100, 40, 41, 14),     # a kind beyond the flag bytes
    "quad": (16000, 200, 150, 41),  # 16391 slots: just above the sixteen-lane limit
}
# hand-placed planar targets in the room's air, 3 m from each other and from everything else: groups of 1, 3, 4 and 5
GROUPS = {1: (3.0, 3.0, 2.0), 3: (6.0, 3.0, 2.0), 4: (9.0, 3.0, 2.0), 5: (3.0, 6.0, 2.0)}
EMPTY_SPOT, OUTSIDE = (6.0, 6.0, 2.0), (-5.0, -6.0, -7.0)
LONE_BALL, BALL_FREE_SPOT = (8.0, 8.0, 3.6), (4.0, 4.0, 3.7)


@functools.lru_cache(maxsize=None)
def _room():
    """Targets: a 12 x 12 x 3 m room -- ground sheet, two walls (planar), six poles (edge), scattered sphere points -- and the
    hand-placed groups."""
    rng = np.random.default_rng(77)
    g, gz = np.arange(0.125, 12.0, 0.25), np.arange(0.125, 3.0, 0.25)
    xx, yy = [a.ravel() for a in np.meshgrid(g, g)]
    ground = np.stack([xx + rng.uniform(-0.05, 0.05, xx.size), yy + rng.uniform(-0.05, 0.05, xx.size), rng.normal(0, 0.01, xx.size)], 1)
    aa, zz = [a.ravel() for a in np.meshgrid(g, gz)]
    walls = np.concatenate([np.stack([rng.normal(0, 0.01, aa.size), aa, zz], 1), np.stack([aa, 12.0 + rng.normal(0, 0.01, aa.size), zz], 1)])
    pz = np.arange(0.05, 3.5, 0.1)
    poles = np.concatenate([np.stack([px + rng.normal(0, 0.01, pz.size), py + rng.normal(0, 0.01, pz.size), pz], 1)
                            for px, py in ((2, 2), (5, 3), (9, 2), (3, 8), (7, 7), (10, 10))])
    balls = np.stack([rng.uniform(0.5, 11.5, 150), rng.uniform(0.5, 11.5, 150), rng.uniform(0.5, 3.0, 150)], 1)
    groups = [np.asarray(c) + rng.uniform(-0.04, 0.04, (m, 3)) for m, c in GROUPS.items()]
    planar = np.concatenate([walls] + groups)
    sphere = np.concatenate([balls, np.asarray(LONE_BALL)[None]])
    return [np.ascontiguousarray(t) for t in (planar, ground, poles, sphere)]


@functools.lru_cache(maxsize=None)
def _frame(name):
    """The frame `name`: the room, and COUNTS[name] query positions W per kind in the map frame -- the hand-placed ones first,
    the others near targets drawn at random.  The source clouds are W taken back through the predicted pose."""
    from tloam_amd import synth
    tgt = _room()
    counts = COUNTS[name]
    rng = np.random.default_rng(sum(counts))

    def near(t, n, sigma):
        return t[rng.choice(len(t), n, replace=n > len(t))] + rng.normal(0, sigma, (n, 3))
    hand_p = np.array([np.add(c, (0.05, 0.03, 0.02)) for c in GROUPS.values()] + [EMPTY_SPOT, OUTSIDE])
    hand_s = np.array([np.add(LONE_BALL, (0.1, 0.0, 0.05)), BALL_FREE_SPOT, OUTSIDE])
    W = [np.concatenate([hand_p, near(tgt[0][:-13], counts[0] - len(hand_p), 0.02)]),
         near(tgt[1], counts[1], 0.02),
         near(tgt[2], counts[2], 0.05),
         np.concatenate([hand_s, near(tgt[3][:-1], counts[3] - len(hand_s), 0.05)])]
    T_pred = synth.se3_exp_np([0.4, -0.3, 0.1, 0.01, -0.02, 0.05])
    R, t = T_pred[:3, :3], T_pred[:3, 3]
    return dict(tgt=tgt, W=W, src=[np.ascontiguousarray((w - t) @ R) for w in W], T_pred=T_pred, n_hand=(len(hand_p), 0, 0, len(hand_s)))


@functools.lru_cache(maxsize=None)
def _still_frame():
    """A frame whose optimum is exact: targets exactly on the planes z = 0 and x = 0, on vertical lines and anywhere (sphere), the
    source points a subset of them, the predicted pose the identity.  The first Solve takes the start's perturbation back, the
    second has nothing to do, and the loop ends on its plateau test with two iterations left."""
    g = np.arange(0.0, 6.0, 0.25)
    a, b = [v.ravel() for v in np.meshgrid(g, g)]
    ground = np.stack([a + 1.0, b + 1.0, np.zeros(a.size)], 1)
    planar = np.stack([np.zeros(a.size), a + 1.0, b + 0.5], 1)
    pz = np.arange(0.0, 3.0, 0.125)
    poles = np.concatenate([np.stack([np.full(pz.size, px), np.full(pz.size, py), pz], 1) for px, py in ((2.0, 2.0), (4.0, 2.0), (2.0, 4.0))])   # (powers of two: the moments are exact)
    rng = np.random.default_rng(5)
    balls = np.round(rng.uniform(1.0, 6.0, (60, 3)) * 64.0) / 64.0
    tgt = [np.ascontiguousarray(t) for t in (planar, ground, poles, balls)]
    pick = lambda t, n: np.ascontiguousarray(t[rng.choice(len(t), n, replace=False)])
    return dict(tgt=tgt, src=[pick(planar, 41), pick(ground, 42), pick(poles, 21), pick(balls, 13)], T_pred=np.eye(4))


@functools.lru_cache(maxsize=None)
def _census(name):
    """Per hand-placed query of frame `name`: the targets in its 27 cells (unclipped) and in the rows the walk keeps, and the
    query's cell -- the same 1e-9 m to either side."""
    fr, radii = _frame(name), _radii()
    out = {}
    for k in (PLANAR, SPHERE):
        org, cell, dim = _grid_of(fr["tgt"][k], radii[k])
        assert int(np.prod(dim)) <= 16384, (k, dim)                         # no growth step: the cell is the radius
        tc = _cells(fr["tgt"][k], org, cell, dim)
        rows = []
        for pw in fr["W"][k][:fr["n_hand"][k]]:
            lens, full, c, _ = _rows(pw, tc, org, cell, dim, radii[k])
            for e in (1e-9, -1e-9):
                l2, f2, _, _ = _rows(pw + e, tc, org, cell, dim, radii[k])
                assert np.array_equal(lens, l2) and np.array_equal(full, f2), (k, pw)
            d = fr["tgt"][k] - pw
            in_reach = int(np.count_nonzero((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] < radii[k] ** 2))
            rows.append(dict(kept=int(lens.sum()), full=int(full.sum()), in_reach=in_reach,
                             outside=bool(np.any(c < 0) or np.any(c >= dim))))
        out[k] = rows
    return out


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_the_frames_hold_the_cases(name):
    fr, cen, counts = _frame(name), _census(name), COUNTS[name]
    assert [len(s) for s in fr["src"]] == list(counts) and all(c >= 10 for c in counts)
    assert 2000 <= sum(len(t) for t in fr["tgt"]) <= 10000
    # short lists, K = 5: 1, 3, 4 and 5 targets in the cells and in reach, then none, then a query outside the grid
    assert [(r["kept"], r["in_reach"]) for r in cen[PLANAR][:4]] == [(m, m) for m in GROUPS], cen[PLANAR]
    assert cen[PLANAR][4]["full"] == 0 and not cen[PLANAR][4]["outside"] and cen[PLANAR][5]["kept"] == 0 and cen[PLANAR][5]["outside"]
    # K = 1: one target, none, outside
    assert cen[SPHERE][0]["kept"] == 1 and cen[SPHERE][0]["in_reach"] == 1 and cen[SPHERE][1]["full"] == 0 and cen[SPHERE][2]["outside"]
    assert counts[SPHERE] < ob.make_config().sphere_maxnum                  # (the sphere cap stops no builder here)


def test_the_kind_boundaries_and_sizes():
    off = {name: np.cumsum(c) for name, c in COUNTS.items()}
    assert [int(o) % 4 for o in off["b123"]] == [1, 2, 3, 1]                # boundaries at 1, 2, 3; a last group of one
    assert [int(o) % 4 for o in off["b000"]] == [0, 0, 0, 2]                # ... all at 0; a last group of two
    assert [int(o) % 4 for o in off["b313"]] == [3, 1, 3, 3]                # ... a last group of three
    for name in ("b123", "b000", "b313"):
        assert off[name][-1] <= WIDE_LIMIT and max(COUNTS[name]) <= FLAGB_STRIDE
    assert off["ride"][-1] <= WIDE_LIMIT and max(COUNTS["ride"]) > FLAGB_STRIDE
    assert WIDE_LIMIT < off["quad"][-1] <= WIDE_LIMIT + 64 and off["quad"][-1] % 4 != 0


def test_the_still_frame_ends_early():
    fr, cfg = _still_frame(), ob.make_config()
    O = ob.Oracle(cfg)
    for k in range(4):
        O.set_source(k, fr["src"][k]); O.set_target(k, fr["tgt"][k])
    rc, T, st = O.scan_match(fr["T_pred"])
    assert rc == 0 and np.abs(T - np.eye(4)).max() < 1e-12 and min(st["n_corr"]) >= 10, (T, st)
    assert st["converged_early"] == 1 and st["outer_iterations"] == 2 and cfg.max_iterations == 4, st


@functools.lru_cache(maxsize=None)
def _pca_cloud():
    """Dense patches (twenty neighbours and more), thin lines and loners (fewer, or none)"""
    rng = np.random.default_rng(11)
    cfg = ob.make_feature_config()
    r = cfg.radius
    dense = np.concatenate([c + rng.uniform(-0.5, 0.5, (400, 3)) * (2 * r, 2 * r, 0.05 * r) for c in ((0, 0, 0), (20 * r, 0, 0))])
    thin = np.stack([np.arange(60) * 0.12 * r, np.full(60, 10 * r), np.zeros(60)], 1) + rng.normal(0, 0.01 * r, (60, 3))
    sparse = rng.uniform(-1, 1, (150, 3)) * (3 * r, 3 * r, 0.5 * r) + (10 * r, -20 * r, 0)
    loners = np.array([[100 * r, 0, 0], [0, 100 * r, 0], [-100 * r, -100 * r, 5 * r]])
    return np.ascontiguousarray(np.concatenate([dense, thin, sparse, loners])[rng.permutation(800 + 60 + 150 + 3)])


def test_the_pca_cloud_holds_short_lists():
    cfg, o = ob.make_feature_config(), ob.pca_info(_pca_cloud())
    cnt = (o["neigh"] >= 0).sum(axis=1)     # (a list below min_neigh is not reported at all)
    assert cfg.K == 20 and cfg.min_neigh == 10 and np.any(cnt == cfg.K) and np.any(cnt == 0), np.bincount(cnt)
    assert len(set(cnt[(cnt > 0) & (cnt < cfg.K)].tolist())) >= 8, np.bincount(cnt)


def _pair(reg, fr, **cfg):
    H, O = reg.HipRegistration(reg.default_config(**cfg)), ob.Oracle(ob.make_config(**cfg))
    for k in range(4):
        H.set_source(k, fr["src"][k]); O.set_source(k, fr["src"][k])
        H.set_target(k, fr["tgt"][k]); O.set_target(k, fr["tgt"][k])
    return H, O


def _same_sets(H, O, active):
    for k in range(4):
        ch, co = H.get_correspondences(k), O.get_correspondences(k)
        assert (len(co["idx"]) >= 10) == (k < active), (k, len(co["idx"]))
        assert np.array_equal(ch["idx"], co["idx"]), k
        for name in ("a", "b", "d"):    # the same un-fused fp64 operations on the same five (one) neighbours: the same bits
            assert np.array_equal(ch[name], co[name]), (k, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name,factor_num", [("b123", 4), ("b000", 4), ("b313", 4), ("b123", 3), ("b313", 2), ("ride", 4), ("quad", 4)])
def test_first_search_matches_oracle(hip_module, name, factor_num):
    """Outer iteration 0: the search at the predicted pose, where the census holds; the compaction reads the flag words."""
    test_the_frames_hold_the_cases(name)
    fr, cen = _frame(name), _census(name)
    H, O = _pair(hip_module, fr, factor_num=factor_num)
    assert H.sm_begin(fr["T_pred"]) == 0 and O.sm_begin(fr["T_pred"]) == 0
    rc_h, _, st_h = H.sm_outer()
    rc_o, _, st_o = O.sm_outer()
    assert rc_h == 0 and rc_o == 0 and st_h["n_corr"] == st_o["n_corr"]
    assert [c > 0 for c in st_o["n_corr"]] == [k < factor_num for k in range(4)]            # an inactive kind adds no factor
    _same_sets(H, O, factor_num)
    # the hand-placed queries: fewer than five targets in reach is no factor of the planar kind (slot 3 has its five); the sphere
    # kind's lone ball is a factor, its record the ball
    assert not np.any(np.isin(H.get_correspondences(PLANAR)["idx"], (0, 1, 2, 4, 5)))
    if factor_num == 4:
        cs = H.get_correspondences(SPHERE)
        assert cen[SPHERE][0]["in_reach"] == 1 and cs["idx"][0] == 0 and np.array_equal(cs["a"][0], fr["tgt"][SPHERE][-1])
        assert not np.any((cs["idx"] == 1) | (cs["idx"] == 2))
    assert H.info()["fallbacks_taken"] == 0
    H.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,factor_num", [("b123", 4), ("b000", 4), ("b313", 4), ("b123", 3), ("b313", 2), ("ride", 4), ("quad", 4)])
def test_scan_match_matches_oracle(hip_module, name, factor_num):
    """The whole frame in one call: the later searches are gated on the pose having moved (it has) or ride on the finish of the
    iteration before; small frames compact from the flag bytes inside the Solve.  The stepwise path gives the same."""
    fr = _frame(name)
    H, O = _pair(hip_module, fr, factor_num=factor_num)
    rh, Th, sh = H.scan_match(fr["T_pred"])
    ro, To, so = O.scan_match(fr["T_pred"])
    assert rh == ro == 0 and sh["n_corr"] == so["n_corr"] and so["accepted_steps"] > 0
    for k in range(4):
        assert np.array_equal(H.get_correspondences(k)["idx"], O.get_correspondences(k)["idx"]), k
    for key in ("gn_evaluations", "gn_iterations", "accepted_steps", "outer_iterations"):
        assert sh[key] == so[key], key
    dt, dr = pose_delta(Th, To)
    print("pose delta", dt, dr)
    assert dt < 1e-6 and dr < 1e-6
    # stepwise, in a context of its own
    S, _ = _pair(hip_module, fr, factor_num=factor_num)
    assert S.sm_begin(fr["T_pred"]) == 0
    done = False
    while not done:
        rc, done, _ = S.sm_outer()
        assert rc == 0
    rc, Ts, ss = S.sm_end()
    assert rc == 0 and ss["n_corr"] == sh["n_corr"] and ss["outer_iterations"] == sh["outer_iterations"]
    for k in range(4):
        assert np.array_equal(S.get_correspondences(k)["idx"], H.get_correspondences(k)["idx"]), k
    dt, dr = pose_delta(Ts, Th)
    assert dt < 1e-9 and dr < 1e-9
    assert H.info()["fallbacks_taken"] == 0 and S.info()["fallbacks_taken"] == 0
    H.close(); S.close()


@pytest.mark.gpu
def test_closed_gate(hip_module):
    """The loop ends early: the searches enqueued behind it find their gate closed and the last set built stands."""
    test_the_still_frame_ends_early()
    fr = _still_frame()
    H, O = _pair(hip_module, fr)
    rh, Th, sh = H.scan_match(fr["T_pred"])
    ro, To, so = O.scan_match(fr["T_pred"])
    assert rh == ro == 0 and sh["n_corr"] == so["n_corr"] and max(pose_delta(Th, To)) < 1e-9
    for key in ("gn_evaluations", "gn_iterations", "accepted_steps", "outer_iterations"):
        assert sh[key] == so[key], key
    _same_sets(H, O, 4)
    H.close()


@pytest.mark.gpu
def test_pca_short_lists_match_oracle(hip_module):
    test_the_pca_cloud_holds_short_lists()
    p = _pca_cloud()
    H = hip_module.HipRegistration()
    g, o = H.pca_info(p), ob.pca_info(p)
    for k in ("num_sum", "neigh", "flatness", "cvr", "sphericity", "normal"):
        assert np.array_equal(g[k], o[k], equal_nan=True), k
    H.close()
