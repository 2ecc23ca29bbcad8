"""The restatement of the closed map's surfels (tests/closed_map_surfel_np.py) without a GPU: the ghost
scene's wall, the sums against a plain per-point loop, the eigen stage against LAPACK, the gate and the PCD round trip."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_carve_np as CN  # noqa: E402
import closed_map_surfel_np as SN  # noqa: E402
import voxel_map_np as VN  # noqa: E402
from tloam_amd import map_io  # noqa: E402


@pytest.fixture(scope="module")
def ghost():
    poses, clouds, wall, box = CS.ghost_scene()
    v = CS.GHOST["voxel"]
    V = CN.build_map(poses, clouds, CS.MASK, v)
    return poses, clouds, wall, V, SN.surfels(V, poses, clouds, CS.MASK, min_points=5)


def test_the_ghost_scene_wall(ghost):
    poses, clouds, wall, V, (S, normals, evals, info) = ghost
    v = CS.GHOST["voxel"]
    assert np.array_equal(S[:, 0], V.N) and info["orphan_points"] == 0 and info["n_points"] == int(V.N.sum())
    cells = {tuple(c) for c in np.floor(wall / v).astype(np.int64).tolist()}
    is_wall = np.array([tuple(c) in cells for c in V.i.tolist()])
    assert int(is_wall.sum()) == 175
    ids = SN.read_box(V, S, evals, min_planarity=0.05)
    kept = ids[is_wall[ids]]
    assert len(kept) == 144
    assert np.all(normals[kept] == np.array([0.0, -1.0, 0.0])) and np.all(evals[kept, 0] == 0.0)
    assert info["solved_voxels"] == int((V.N >= 5).sum())


def test_sums_against_a_per_point_loop():
    rng = np.random.default_rng(2)
    v, o = 0.3, np.array([0.25, -1.5, 0.125])
    poses = [np.eye(4), np.eye(4)]
    poses[1][:3, 3] = [1.0, -2.0, 0.5]
    pts = [rng.uniform(-2.0, 2.0, (300, 3)), np.concatenate([rng.uniform(-2.0, 2.0, (200, 3)), [[np.nan, 0.0, 0.0]]])]
    clouds = [CS.slot0(p) for p in pts]
    V = CN.build_map(poses, clouds, CS.MASK, v, o)
    S, orphans = SN.moments(V, poses, clouds, CS.MASK)
    want = np.zeros_like(S)
    for P, p in zip(poses, pts):
        for x in p[np.isfinite(p).all(axis=1)]:
            E = CN.transform(P, x[None])[0]
            s = (E - o) / v
            i = np.floor(s)
            q = np.floor((s - i) * VN.QSCALE + 0.5).astype(np.int64)
            r = [int(a) >> 8 for a in q]
            w = [int(np.floor(min(max(((P[a, 3] - E[a]) / v) * 256.0, -2.0 ** 30), 2.0 ** 30) + 0.5)) for a in range(3)]
            j = V.id_of[int(VN.pack(i.astype(np.int64)[None])[0])]
            want[j] += [1, *r, r[0] * r[0], r[0] * r[1], r[0] * r[2], r[1] * r[1], r[1] * r[2], r[2] * r[2], *w]
    assert orphans == 0 and np.array_equal(S, want) and S[:, 1:4].max() <= 65536 * S[:, 0].max()
    # clouds re-attached since the build: the points outside the map's voxels are orphans, the others still add
    moved = [CS.slot0(p + 40.0) for p in pts]
    S2, orphans2 = SN.moments(V, poses, moved, CS.MASK)
    assert orphans2 == 500 and not S2.any()
    # an overflow keyframe adds nothing, even where its other points fall into voxels of the map
    far = [clouds[0], CS.slot0(np.concatenate([pts[1][:200], [[v * 2.0 ** 20, 0.0, 0.0]]]))]
    S3, orphans3 = SN.moments(V, poses, far, CS.MASK)
    S0, _ = SN.moments(V, poses[:1], clouds[:1], CS.MASK)
    assert orphans3 == 0 and np.array_equal(S3, S0)


@pytest.mark.parametrize("seed", range(6))
def test_eigen_stage_against_lapack(seed):
    """test_eig3_vs_lapack's tolerances on covariances of integer moments: planes, blobs and lines in a voxel"""
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(5, 400))
    shape = [(1.0, 1.0, 1.0), (1.0, 1.0, 0.01), (1.0, 0.02, 0.01)][seed % 3]
    A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    r = np.clip(np.floor(32768.0 + (rng.normal(size=(n, 3)) * shape) @ A.T * 8000.0), 0, 65536).astype(np.int64)
    w = rng.integers(-1000, 1000, (n, 3))
    S = np.concatenate([[n], r.sum(0), [(r[:, a] * r[:, b]).sum() for a, b in SN.PAIRS], w.sum(0)]).astype(np.int64)[None]
    v = 0.5
    normals, evals, solved = SN.solve(S, v, 5)
    assert solved[0]
    m = S[0, 1:4] / n
    c = np.array([[S[0, 4 + SN.PAIRS.index((min(a, b), max(a, b)))] / n - m[a] * m[b] for b in range(3)] for a in range(3)])
    ev_ref, V_ref = np.linalg.eigh(c)
    s2 = (v * 2.0 ** -16) ** 2
    np.testing.assert_allclose(evals[0], ev_ref * s2, rtol=1e-12, atol=1e-14 * ev_ref[-1] * s2)
    assert abs(np.linalg.norm(normals[0]) - 1.0) < 1e-13
    assert np.allclose(c @ normals[0], normals[0] * ev_ref[0], atol=1e-12 * ev_ref[-1])
    assert normals[0] @ S[0, 10:13] >= 0.0
    # the exact integer covariance agrees with the centred one to rounding
    x = r - r.mean(0)
    np.testing.assert_allclose(c, x.T @ x / n, rtol=0, atol=1e-9 * np.abs(c).max())


def test_unsolved_and_degenerate_voxels():
    pts = lambda rows: np.array(rows, np.int64)  # noqa: E731
    line = pts([[100 * t, 200 * t, 300 * t] for t in range(5)])
    same = pts([[7, 7, 7]] * 6)
    four = pts([[0, 0, 0], [10, 0, 0], [0, 10, 0], [10, 10, 0]])
    S = np.array([np.concatenate([[len(r)], r.sum(0), [(r[:, a] * r[:, b]).sum() for a, b in SN.PAIRS], [0, 0, 1]])
                  for r in (line, same, four)], np.int64)
    normals, evals, solved = SN.solve(S, 1.0, 5)
    assert solved.tolist() == [True, True, False] and not normals[2].any() and not evals[2].any()
    assert evals[0, 2] > 0.0 and abs(evals[0, 1]) <= 1e-12 * evals[0, 2]     # a line: solved, one variance
    assert not evals[1].any() and abs(np.linalg.norm(normals[1]) - 1.0) < 1e-15   # a point: solved, no extent

    class Rows:
        N = S[:, 0]

        @staticmethod
        def centroids():
            return np.zeros((3, 3))

    assert len(SN.read_box(Rows, S, evals)) == 0                              # the gate rejects all three
    assert SN.read_box(Rows, S, evals, min_planarity=-1.0).tolist() == [0]    # ev2 > 0 still holds the point back
    assert SN.solve(S, 1.0, 4)[2].all()


def test_surfel_pcd_round_trip(tmp_path, ghost):
    poses, clouds, wall, V, (S, normals, evals, info) = ghost
    ids = SN.read_box(V, S, evals)
    cen = V.centroids()[ids]
    for ascii in (False, True):
        path = str(tmp_path / f"surfels_{int(ascii)}.pcd")
        map_io.write_surfel_pcd(path, cen, normals[ids], S[ids, 0], ascii=ascii)
        c, n, k = map_io.read_surfel_pcd(path)
        assert c.tobytes() == cen.tobytes() and n.tobytes() == normals[ids].tobytes() and k.tobytes() == S[ids, 0].tobytes()
        head = open(path, "rb").read(200).decode("ascii", "replace")
        assert "FIELDS x y z normal_x normal_y normal_z count" in head
    with pytest.raises(ValueError):
        map_io.write_surfel_pcd(str(tmp_path / "bad.pcd"), cen, normals[ids][:-1], S[ids, 0])
    map_io.write_voxel_pcd(str(tmp_path / "vox.pcd"), cen, S[ids, 0])
    with pytest.raises(ValueError):
        map_io.read_surfel_pcd(str(tmp_path / "vox.pcd"))
