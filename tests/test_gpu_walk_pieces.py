"""The sixteen-lane search's piece walk (tl_walk.hpp, LPQ = 16) on one small hand-made frame, through tloam_sm_* /
tloam_scan_match and the set getters, against the oracle, bit for bit: the correspondence index lists (which source slots
carry a factor is the search's flag word) and the records a, b, d -- the sphere kind's is a copy of the neighbour found, the
five-neighbour kinds' are fitted to the neighbours in the oracle's operation order.

The walk cuts a query's candidates -- its nine (z, y) rows one after the other, T records -- into 16-byte pieces, sixteen
lanes load sixteen consecutive pieces per instruction, a trip covers 32 records.  The frame is built so that the cases below
all occur, and `_census` counts every query's rows with numpy BEFORE anything is handed to the GPU: a frame that misses a case
fails in test_the_frame_holds_every_case (no GPU needed), not in a kernel.
  * T = 0 (all rows empty; all rows clipped away or outside the grid), T = 1
  * T = 32, 33 and 65: one, two and three trips (dense clumps, the 33 and the 65 split over two rows)
  * a three-trip query in one wave (four consecutive source slots) with one-trip queries
  * rows cut by the grid border (x0 clamped; y or z outside the grid) and by the clipped walk, a query near a cell face
  * a row boundary at an odd record (so inside a sixteen-piece run)
  * two targets at bit-equal distance among a query's nearest K + 1 (exact duplicates): the ambiguous-key redo
  * the sphere kind (K = 1) and a five-neighbour kind in one wave; a last wave with fewer than four live queries
"""
import functools

import numpy as np
import pytest

from conftest import pose_delta
from oracle import binding as ob
from tloam_amd import synth

WIDE_LIMIT = 16384            # at most this many source points: sixteen lanes per query (tl_forms.hpp)
RADIUS_SLACK = 1.0 + 1e-6     # cell = radius * this (tl_grid_plan.hpp); nothing grows here: every kind's box is below 16 Ki cells
K_OF_KIND = (5, 5, 5, 1)      # planar, ground, edge, sphere
PLANAR, GROUND, EDGE, SPHERE = 0, 1, 2, 3


def _radii():
    c = ob.make_config()
    return (c.planar_dist_thres, c.ground_dist_thres, c.edge_dist_thres, c.sphere_dist_thres)


def _clump(rng, centre, n, spread=0.04):
    return np.asarray(centre, float) + rng.uniform(-spread, spread, (n, 3))


def _grid_of(tgt, radius):
    """(org, cell, dim) as plan_grids sizes a kind's grid (tl_grid_plan.hpp), without the growth steps"""
    lo, hi = tgt.min(axis=0), tgt.max(axis=0)
    cell = radius * RADIUS_SLACK
    dim = (np.floor((hi - lo) / cell) + 1.0).astype(int)
    return lo, cell, dim


def _cells(p, org, cell, dim):
    """cell_coord (tl_knn.hpp) per axis"""
    f = np.floor((p - org) * (1.0 / cell))
    return np.minimum(np.maximum(f, -2.0), dim + 1.0).astype(int)


def _rows(pw, tc, org, cell, dim, radius):
    """The nine row lengths of one query as knn_rows resolves them (clipped walk), the same without the clip, and the query's
    cell and position inside it."""
    inv = 1.0 / cell
    c = _cells(pw, org, cell, dim)
    f = (pw - org) * inv - c
    reach = radius * (1.0 + 1e-6)
    c2 = reach * reach
    lo2, hi2 = (f * cell) ** 2, ((1.0 - f) * cell) ** 2
    lens, full = np.zeros(9, int), np.zeros(9, int)
    for r in range(9):
        rz, ry = r // 3, r % 3
        z, y = c[2] - 1 + rz, c[1] - 1 + ry
        if not (0 <= z < dim[2] and 0 <= y < dim[1]):
            continue
        row = tc[(tc[:, 2] == z) & (tc[:, 1] == y), 0]
        full[r] = np.count_nonzero((row >= max(c[0] - 1, 0)) & (row <= min(c[0] + 1, dim[0] - 1)))
        s2 = (lo2[2] if rz == 0 else hi2[2] if rz == 2 else 0.0) + (lo2[1] if ry == 0 else hi2[1] if ry == 2 else 0.0)
        xa = max(c[0] - (1 if s2 + lo2[0] <= c2 else 0), 0)
        xb = min(c[0] + (1 if s2 + hi2[0] <= c2 else 0), dim[0] - 1)
        if s2 <= c2 and xa <= xb:
            lens[r] = np.count_nonzero((row >= xa) & (row <= xb))
    return lens, full, c, f


@functools.lru_cache(maxsize=None)
def _frame():
    """The hand-made frame: a 12 x 12 x 4 m room in the map frame -- a ground sheet, two walls (planar), six poles (edge),
    scattered sphere points -- plus the clumps, loners and duplicates of the cases; the source clouds are the wanted query
    positions W taken back through the predicted pose, so the search of outer iteration 0 runs at W (to ~1e-14)."""
    rng = np.random.default_rng(2025)
    g = np.arange(0.125, 12.0, 0.25)
    gz = np.arange(0.125, 3.0, 0.25)
    # ---- targets
    xx, yy = [a.ravel() for a in np.meshgrid(g, g)]
    ground = np.stack([xx + rng.uniform(-0.05, 0.05, xx.size), yy + rng.uniform(-0.05, 0.05, xx.size), rng.normal(0, 0.01, xx.size)], 1)
    aa, zz = [a.ravel() for a in np.meshgrid(g, gz)]
    wall_a = np.stack([rng.normal(0, 0.01, aa.size), aa, zz], 1)            # x = 0
    wall_b = np.stack([aa, 12.0 + rng.normal(0, 0.01, aa.size), zz], 1)     # y = 12
    walls = np.concatenate([wall_a, wall_b])
    pz = np.arange(0.05, 3.5, 0.1)
    poles = np.concatenate([np.stack([px + rng.normal(0, 0.01, pz.size), py + rng.normal(0, 0.01, pz.size), pz], 1)
                            for px, py in ((2, 2), (5, 3), (9, 2), (3, 8), (7, 7), (10, 10))])
    balls = np.stack([rng.uniform(0.5, 11.5, 150), rng.uniform(0.5, 11.5, 150), rng.uniform(0.5, 3.0, 150)], 1)
    radii = _radii()
    # the planar kind's clumps hang in the room's air, 3 m from each other and from the walls: a query at a clump sees it alone
    org0, cell0, _ = _grid_of(walls, radii[PLANAR])       # (the clumps lie inside the walls' box: it stays the kind's grid)
    mid32 = org0 + (np.floor((np.array([6.0, 3.0, 2.0]) - org0) / cell0) + 0.5) * cell0   # the middle of a cell
    c65, c33, lone = np.array([3.0, 3.0, 2.0]), np.array([9.0, 3.0, 2.0]), np.array([3.0, 6.0, 2.0])
    planar = np.concatenate([walls, walls[::50],                                            # (exact duplicates)
                             _clump(rng, c65, 40), _clump(rng, c65 + [0, 0.5, 0], 25),      # 65 over two y rows
                             _clump(rng, mid32, 32),                                        # 32 in one cell
                             _clump(rng, c33, 20), _clump(rng, c33 + [0, 0, 0.5], 13),      # 33 over two z rows
                             lone[None]])
    s33, slone = np.array([4.0, 4.0, 3.6]), np.array([8.0, 8.0, 3.6])
    sphere = np.concatenate([balls, balls[::15], _clump(rng, s33, 33), slone[None]])
    tgt = [np.ascontiguousarray(planar), np.ascontiguousarray(ground), np.ascontiguousarray(poles), np.ascontiguousarray(sphere)]
    # ---- query positions in the map frame, the hand-placed ones first (source slots run planar, ground, edge, sphere)
    def near(t, n, sigma=0.02):
        return t[rng.choice(len(t), n, replace=False)] + rng.normal(0, sigma, (n, 3))
    W = [
        np.concatenate([[c65 + [0.05, 0.25, 0.02], lone + [0.1, 0.05, 0.02], [6.0, 6.0, 2.0], mid32 + [0.05, 0.03, 0.02],
                         c33 + [0.05, 0.02, 0.25]],
                        walls[::50][:20] + rng.normal(0, 0.02, (20, 3)),     # at the duplicated wall points
                        near(walls, 100)]),
        np.concatenate([[[-0.3, 5.03, 0.0], [5.03, -0.2, 0.01], [-0.8, 5.0, 0.0], [5.0, 5.0, 0.6], [12.2, 12.15, 0.0],
                         [6.126, 6.374, 0.004]],
                        near(ground, 150)]),
        np.concatenate([near(poles, 57, 0.05), [[5.0, 9.0, 2.0], [2.3, 2.2, 3.9], [11.0, 11.0, 0.2], [2.0, 2.0, -0.4]]]),
        np.concatenate([[s33 + [0.05, 0.03, 0.02], slone + [0.1, 0.0, 0.05], [10.0, 4.0, 3.6]],
                        balls[::15][:8] + rng.normal(0, 0.02, (8, 3)),       # at the duplicated sphere points
                        near(balls, 24, 0.05)]),
    ]
    T_pred = synth.se3_exp_np([0.4, -0.3, 0.1, 0.01, -0.02, 0.05])
    R, t = T_pred[:3, :3], T_pred[:3, 3]
    src = [np.ascontiguousarray((w - t) @ R) for w in W]                    # R^T (w - t)
    return dict(tgt=tgt, W=W, src=src, T_pred=T_pred, radii=radii)


@functools.lru_cache(maxsize=None)
def _census():
    """Per kind and query: the row lengths of the walk (numpy), T, the trips, ties among the nearest K + 1 -- and the proof that
    none of it hangs on the last bits of the query position (the same row lengths 1e-9 m to either side)."""
    fr = _frame()
    out = []
    for k in range(4):
        tgt, radius = fr["tgt"][k], fr["radii"][k]
        org, cell, dim = _grid_of(tgt, radius)
        assert int(np.prod(dim)) <= 16384, (k, dim)                         # no growth step: the cell is the radius
        tc = _cells(tgt, org, cell, dim)
        rows = []
        for pw in fr["W"][k]:
            lens, full, c, f = _rows(pw, tc, org, cell, dim, radius)
            for e in (1e-9, -1e-9):
                l2, f2, _, _ = _rows(pw + e, tc, org, cell, dim, radius)
                assert np.array_equal(lens, l2) and np.array_equal(full, f2), (k, pw)
            d = tgt - pw
            d2 = np.sort((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:K_OF_KIND[k] + 1]
            rows.append(dict(lens=lens, full=full, cell=c, frac=f, T=int(lens.sum()), tie=bool(np.any(np.diff(d2) == 0.0)),
                             d2min=float(d2[0])))
        out.append(dict(org=org, cell=cell, dim=dim, rows=rows))
    return out


def _slots():
    """(kind, row-table entry) of every source slot in slot order"""
    return [(k, r) for k, g in enumerate(_census()) for r in g["rows"]]


def test_the_frame_holds_every_case():
    fr, cen = _frame(), _census()
    slots = _slots()
    n = len(slots)
    assert all(len(fr["src"][k]) >= 10 and len(fr["tgt"][k]) >= 10 for k in range(4))
    assert 300 <= n <= 1000 and n <= WIDE_LIMIT and 2000 <= sum(len(t) for t in fr["tgt"]) <= 10000
    T = np.array([r["T"] for _, r in slots])
    for want in (0, 1, 32, 33, 65):
        assert np.any(T == want), want
    # T = 0 three ways: nothing there; clipped away / outside the grid although the unclipped rows hold targets or the query lies outside
    assert any(r["T"] == 0 and r["full"].sum() == 0 for _, r in slots)
    assert any(r["T"] == 0 and (np.any(r["cell"] < 0) or np.any(r["cell"] >= cen[k]["dim"])) for k, r in slots)
    # the 33 and the 65 are split over two rows; the 32 sits in one
    assert any(r["T"] == 33 and np.count_nonzero(r["lens"]) == 2 for _, r in slots)
    assert any(r["T"] == 65 and np.count_nonzero(r["lens"]) == 2 for _, r in slots)
    assert any(r["T"] == 32 and np.count_nonzero(r["lens"]) == 1 for _, r in slots)
    # a wave = four consecutive slots: a three-trip query beside one-trip (and empty) ones
    trips = -(-T // 32)
    assert any(trips[w:w + 4].max() == 3 and np.any(trips[w:w + 4] == 1) and np.any(trips[w:w + 4] == 0) for w in range(0, n, 4))
    # the grid border: x0 clamped, y outside, z outside -- each with candidates left
    assert any(r["cell"][0] <= 0 and r["T"] > 0 for _, r in slots)
    assert any((r["cell"][1] < 0 or r["cell"][1] >= cen[k]["dim"][1]) and r["T"] > 0 for k, r in slots)
    assert any((r["cell"][2] < 0 or r["cell"][2] >= cen[k]["dim"][2]) and r["T"] > 0 for k, r in slots)
    assert any(np.all(r["cell"] >= cen[k]["dim"] - 1) and r["T"] > 0 for k, r in slots)      # the far corner: xb clamped
    # the clipped walk: whole rows dropped that hold targets, rows shortened at an end; a query within 2 % of a cell face
    assert any(np.any((r["lens"] == 0) & (r["full"] > 0)) and r["T"] > 0 for _, r in slots)
    assert any(np.any((r["lens"] > 0) & (r["lens"] < r["full"])) for _, r in slots)
    assert any(r["T"] > 0 and (r["frac"].min() < 0.02 or r["frac"].max() > 0.98) for _, r in slots)
    # a row that starts at an odd record behind a non-empty one
    def odd_start(r):
        pre = np.concatenate([[0], np.cumsum(r["lens"])[:-1]])
        return np.any((r["lens"] > 0) & (pre % 2 == 1))
    assert sum(odd_start(r) for _, r in slots) >= 10
    # bit-equal distances among the nearest K + 1, in a five-neighbour kind and in the sphere kind
    assert any(r["tie"] for k, r in slots if k == PLANAR) and any(r["tie"] for k, r in slots if k == SPHERE)
    # the sphere kind shares a wave with the edge kind; the last wave has fewer than four live queries
    assert (n - len(fr["src"][SPHERE])) % 4 != 0 and n % 4 != 0
    assert len(fr["src"][SPHERE]) < ob.make_config().sphere_maxnum          # (the sphere cap stops no builder here)


def _pair(reg):
    fr = _frame()
    H, O = reg.HipRegistration(reg.default_config()), ob.Oracle(ob.make_config())
    for k in range(4):
        H.set_source(k, fr["src"][k]); O.set_source(k, fr["src"][k])
        H.set_target(k, fr["tgt"][k]); O.set_target(k, fr["tgt"][k])
    return H, O


@pytest.mark.gpu
def test_first_search_matches_oracle(hip_module):
    """Outer iteration 0: the search at the predicted pose, where the census above holds."""
    test_the_frame_holds_every_case()
    fr, cen = _frame(), _census()
    H, O = _pair(hip_module)
    assert H.sm_begin(fr["T_pred"]) == 0 and O.sm_begin(fr["T_pred"]) == 0
    gi = H.grid_info()
    for k in range(4):
        assert gi["dim"][k] == list(cen[k]["dim"]) and gi["cell"][k] == cen[k]["cell"] and gi["n"][k] == len(fr["tgt"][k]), (k, gi)
    rc_h, _, st_h = H.sm_outer()
    rc_o, _, st_o = O.sm_outer()
    assert rc_h == 0 and rc_o == 0 and st_h["n_corr"] == st_o["n_corr"]
    for k in range(4):
        ch, co = H.get_correspondences(k), O.get_correspondences(k)
        assert len(co["idx"]) >= 10, k
        assert np.array_equal(ch["idx"], co["idx"]), k
        for name in ("a", "b", "d"):    # the same un-fused fp64 operations on the same five (one) neighbours: the same bits
            print("kind", k, name, "max |hip - oracle|", float(np.abs(ch[name] - co[name]).max()))
            assert np.array_equal(ch[name], co[name]), (k, name)
    # the hand-placed sphere queries: a factor where the census says a neighbour is in reach, its record the nearest target
    rows = cen[SPHERE]["rows"]
    r2 = fr["radii"][SPHERE] ** 2
    have = [i for i, r in enumerate(rows) if r["d2min"] < r2 and r["d2min"] <= 0.2]
    assert H.get_correspondences(SPHERE)["idx"].tolist() == have
    assert H.info()["fallbacks_taken"] == 0
    H.close()


@pytest.mark.gpu
def test_scan_match_matches_oracle(hip_module):
    """The whole frame in one call (the searches of the later outer iterations ride on the finish of the one before)."""
    fr = _frame()
    H, O = _pair(hip_module)
    rh, Th, sh = H.scan_match(fr["T_pred"])
    ro, To, so = O.scan_match(fr["T_pred"])
    assert rh == ro == 0 and sh["n_corr"] == so["n_corr"]
    for k in range(4):
        assert np.array_equal(H.get_correspondences(k)["idx"], O.get_correspondences(k)["idx"]), k
    for key in ("gn_evaluations", "gn_iterations", "accepted_steps", "outer_iterations"):
        assert sh[key] == so[key], key
    dt, dr = pose_delta(Th, To)
    print("pose delta", dt, dr)
    assert dt < 1e-6 and dr < 1e-6
    assert H.info()["fallbacks_taken"] == 0
    H.close()
