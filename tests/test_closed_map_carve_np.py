"""The carve's restatement (tests/closed_map_carve_np.py) without a GPU: its walk against a brute-force
segment / box intersection, the tie rule, the edge cases, the ghost scene's condition and the static pass's false-removal share."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_carve_np as CN  # noqa: E402
import voxel_map_np as VN  # noqa: E402


def overlap_with_cells(s0, s1, cells):
    """the length, in the ray's parameter t in [0, 1], of the piece of the segment s0 -> s1 inside each closed unit cell
    (negative: the segment passes the cell by)"""
    d = s1 - s0
    lo, hi = np.zeros(len(cells)), np.ones(len(cells))
    for a in range(3):
        if d[a] == 0.0:
            out = ~((cells[:, a] <= s0[a]) & (s0[a] <= cells[:, a] + 1))
            lo[out], hi[out] = 1.0, 0.0
            continue
        t0, t1 = (cells[:, a] - s0[a]) / d[a], (cells[:, a] + 1 - s0[a]) / d[a]
        lo, hi = np.maximum(lo, np.minimum(t0, t1)), np.minimum(hi, np.maximum(t0, t1))
    return hi - lo


@pytest.mark.parametrize("voxel,origin", [(1.0, (0.3, -0.7, 0.11)), (0.25, (1.0, -2.0, 0.5))])
def test_the_walk_visits_the_cells_a_brute_force_intersection_gives(voxel, origin):
    """2000 random rays without ties, origins off the grid, negative coordinates: every cell the segment crosses by more than
    EPS of its length is walked, every walked cell is crossed or touched within EPS.  EPS = 1e-9 of the ray is far above the
    walk's rounding (a few 2^-53 of a coordinate of at most 64 cells) and far below the crossings of random rays."""
    EPS = 1e-9
    rng = np.random.default_rng(21)
    o = np.asarray(origin)
    O = rng.uniform(-8.0, 8.0, (2000, 3))
    E = O + rng.uniform(-8.0, 8.0, (2000, 3)) * voxel
    s0, s1 = (O - o) / voxel, (E - o) / voxel
    W = CN.Walk(s0, s1)
    n = W.n.copy()
    visited = [[] for _ in range(len(O))]
    for rows, cells in W:
        for r, c in zip(rows.tolist(), cells.tolist()):
            visited[r].append(tuple(c))
    assert (W.c == W.ce).all()   # n steps end in the end cell
    assert n.max() > 15 and (s0 < 0).any() and (s1 < 0).any()
    for r in range(len(O)):
        assert len(visited[r]) == n[r] == len(set(visited[r]))
        walked = set(visited[r]) | {tuple(W.ce[r].tolist())}
        lo = np.minimum(np.floor(s0[r]), np.floor(s1[r])).astype(np.int64) - 1
        hi = np.maximum(np.floor(s0[r]), np.floor(s1[r])).astype(np.int64) + 1
        box = np.stack(np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij"), axis=-1).reshape(-1, 3)
        ov = overlap_with_cells(s0[r], s1[r], box)
        crossed = {tuple(c) for c in box[ov > EPS].tolist()}
        touched = {tuple(c) for c in box[ov > -EPS].tolist()}
        assert crossed <= walked <= touched, r


def test_ties_go_to_the_lowest_axis():
    cells, end = CN.walk([0.5, 0.5, 0.5], [2.5, 2.5, 2.5])   # through two cell corners
    assert cells.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1], [2, 1, 1], [2, 2, 1]] and end.tolist() == [2, 2, 2]
    cells, end = CN.walk([2.5, 2.5, 2.5], [0.5, 0.5, 0.5])
    assert cells.tolist() == [[2, 2, 2], [1, 2, 2], [1, 1, 2], [1, 1, 1], [0, 1, 1], [0, 0, 1]] and end.tolist() == [0, 0, 0]
    cells, end = CN.walk([0.5, 0.5, 0.5], [0.5, 2.5, 2.5])   # through two cell edges: y before z
    assert cells.tolist() == [[0, 0, 0], [0, 1, 0], [0, 1, 1], [0, 2, 1]] and end.tolist() == [0, 2, 2]
    cells, end = CN.walk([-0.5, 0.5, -0.5], [-2.5, 0.5, 1.5])  # x before z, downwards in x
    assert cells.tolist() == [[-1, 0, -1], [-2, 0, -1], [-2, 0, 0], [-3, 0, 0]] and end.tolist() == [-3, 0, 1]
    cells, end = CN.walk([0.0, 0.0, 0.0], [2.0, 2.0, 0.0])     # from a corner to a corner, along the cells' diagonal
    assert cells.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [2, 1, 0]] and end.tolist() == [2, 2, 0]


def test_edge_cases_of_the_walk():
    for a in range(3):
        for sign in (1.0, -1.0):
            s0, s1 = np.array([0.5, 0.25, -0.75]), np.array([0.5, 0.25, -0.75])
            s1[a] += sign * 4.0
            cells, end = CN.walk(s0, s1)
            want = np.tile(np.floor(s0).astype(np.int64), (4, 1))
            want[:, a] += (sign * np.arange(4)).astype(np.int64)
            assert cells.tolist() == want.tolist() and end.tolist() == np.floor(s1).astype(np.int64).tolist(), (a, sign)
    cells, end = CN.walk([0.1, 0.2, 0.3], [0.9, 0.8, 0.7])   # inside one cell: the end cell is never visited
    assert len(cells) == 0 and end.tolist() == [0, 0, 0]
    cells, end = CN.walk([3.0, 0.5, 0.5], [1.0, 0.5, 0.5])   # from a cell's face downwards: tMax 0 at the start
    assert cells.tolist() == [[3, 0, 0], [2, 0, 0]] and end.tolist() == [1, 0, 0]


def test_skipped_rays_and_the_end_margin():
    P = np.eye(4)
    P[:3, 3] = [0.5, 0.5, 0.5]
    target = np.array([[0.0, 0.0, 0.0],      # L = 0
                       [np.nan, 0.0, 0.0], [np.inf, 0.0, 0.0],
                       [61.0, 0.0, 0.0],     # L > max_range
                       [60.0, 0.0, 0.0],     # L == max_range: a ray
                       [0.25, 0.0, 0.0],     # inside one cell
                       [float(1 << 21), 0.0, 0.0]])
    clouds = [CS.slot0(target)]
    occupied = CS.slot0(np.array([[5.0, 0.0, 0.0]] * 4 + [[59.3, 0.0, 0.0]]))
    V = CN.build_map([P], [occupied], CS.MASK)
    M, info = CN.carve(V, [P], clouds, CS.MASK)
    assert info == dict(n_keyframes=1, n_rays=7, skipped_rays=5, steps=60, tested=2, misses=1, voxels_missed=1)
    assert M.tolist() == [1, 0]   # the voxel at 59.3 m lies within end_margin of the return at 60 m
    M, info = CN.carve(V, [P], clouds, CS.MASK, end_margin=60.0)   # end_margin >= L: tt < 0 never holds with 0 <= tt
    assert info["misses"] == 0 and info["tested"] == 2
    M, info = CN.carve(V, [P], clouds, CS.MASK, end_margin=0.0)
    assert M.tolist() == [1, 1]
    assert CN.read_carved(V, M).tolist() == [0, 1]                                # M = 1 < min_miss
    assert CN.read_carved(V, M, min_miss=1).tolist() == [0, 1]                    # M > N holds for neither (N = 4, 1)
    assert CN.read_carved(V, M, min_miss=1, miss_ratio=0.5).tolist() == [0]       # 1 > 0.5 * 1, but not 1 > 0.5 * 4
    assert CN.read_carved(V, M, min_miss=1, miss_ratio=0.2).tolist() == []
    assert CN.read_carved(V, M, min_count=2, min_miss=1, miss_ratio=0.5).tolist() == [0]
    assert CN.read_carved(V, M, [50.0, 0.0, 0.0], [70.0, 1.0, 1.0]).tolist() == [1]


def test_the_ghost_scene_loses_the_ghost_and_keeps_the_wall():
    """DESIGN.md section 21's condition: every voxel the box created is left out by read_carved at the wrapper's defaults, and
    no wall voxel is."""
    poses, clouds, wall, box = CS.ghost_scene()
    v = CS.GHOST["voxel"]
    V = CN.build_map(poses, clouds, CS.MASK, v)
    M, info = CN.carve(V, poses, clouds, CS.MASK, max_range=CS.GHOST["max_range"])
    id_of = {int(k): i for i, k in enumerate(V.keys)}
    key_of = lambda pts: {int(k) for k in VN.pack(np.floor(pts / v).astype(np.int64))}  # noqa: E731
    box_ids = sorted(id_of[k] for k in key_of(box))
    wall_ids = sorted(id_of[k] for k in key_of(wall))
    assert not set(box_ids) & set(wall_ids) and len(box_ids) + len(wall_ids) == len(V.keys)
    kept = set(CN.read_carved(V, M, **CN.READ_DEFAULTS).tolist())
    print(f"ghost scene: {info}; box voxels {len(box_ids)} (N {V.N[box_ids].min()}..{V.N[box_ids].max()}, "
          f"M {M[box_ids].min()}..{M[box_ids].max()}), wall voxels {len(wall_ids)} (M max {M[wall_ids].max()})")
    assert len(box_ids) >= 27 and info["skipped_rays"] == 0
    assert not kept & set(box_ids)
    assert set(wall_ids) <= kept


def test_the_static_pass_reports_its_false_removals():
    """Nothing in the generator moves, so every voxel read_carved leaves out of this pass is a false removal.  The share is
    reported (DESIGN.md section 21 records it), not asserted against a bar."""
    poses, clouds = CS.static_pass()
    V = CN.build_map(poses, clouds, CS.MASK, CS.STATIC["voxel"])
    M, info = CN.carve(V, poses, clouds, CS.MASK, max_range=CS.STATIC["max_range"])
    kept = CN.read_carved(V, M, **CN.READ_DEFAULTS)
    nv = len(V.keys)
    print(f"static pass: {info}; voxels {nv}, left out {nv - len(kept)} ({100.0 * (nv - len(kept)) / nv:.2f} %)")
    assert info["n_rays"] == sum(len(c[1][0]) for c in clouds) and info["misses"] == int(M.sum()) and nv > 1000
    assert len(CN.read_carved(V, M, min_miss=10 ** 9)) == nv   # nothing is left out when nothing can be missed enough
