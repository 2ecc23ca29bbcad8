"""The extension's restatement (tests/closed_map_extend_np.py) without a GPU: extended keyframe by keyframe
it is the full build and the full surfel pass, integer for integer; its carve is the compositional one, with the static pass's
figures; and the two scenes meet the conditions the section states."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_carve_np as CN  # noqa: E402
import closed_map_extend_np as EN  # noqa: E402
import closed_map_surfel_np as SN  # noqa: E402
import extend_scenes as ES  # noqa: E402

GHOST_CUTS = ((1,), (2,), (3,), (5,), (1, 2, 3, 4, 5))
GHOST_CARVE = dict(max_range=CS.GHOST["max_range"], end_margin=1.0, radius=0.25)
STATIC_CARVE = dict(max_range=CS.STATIC["max_range"], end_margin=1.0, radius=0.25)


def extended(poses, clouds, cuts, voxel, carve=None):
    """the map built from the keyframes before cuts[0] and extended at every cut"""
    A = EN.ExtendedMapNP(CS.MASK, voxel, surfels=True, carve=carve)
    edges = [0, *cuts, len(poses)]
    infos = [A.extend(poses[a:b], clouds[a:b]) for a, b in zip(edges[:-1], edges[1:])]
    return A, infos


def same_rows(A, B):
    return all(getattr(A, f).tobytes() == getattr(B, f).tobytes() for f in ("keys", "i", "N", "Q"))


def box_ids(V, box):
    want = ES.cells(box, V.voxel)
    return np.flatnonzero([tuple(c) in want for c in V.i.tolist()])


def kept_cells(V, M):
    return {tuple(c) for c in V.i[CN.read_carved(V, M)].tolist()}


@pytest.fixture(scope="module")
def static():
    poses, clouds = CS.static_pass()
    B = CN.build_map(poses, clouds, CS.MASK, CS.STATIC["voxel"])
    return poses, clouds, B


@pytest.mark.parametrize("cuts", GHOST_CUTS)
def test_rows_and_sums_are_the_full_builds_on_the_ghost_scene(cuts):
    poses, clouds, _, _ = CS.ghost_scene()
    v = CS.GHOST["voxel"]
    A, infos = extended(poses, clouds, cuts, v)
    B = CN.build_map(poses, clouds, CS.MASK, v)
    S, normals, evals, sinfo = SN.surfels(B, poses, clouds, CS.MASK)
    assert same_rows(A.V, B)
    got = A.surfels()
    assert got[0].tobytes() == S.tobytes() and got[1].tobytes() == normals.tobytes() and got[2].tobytes() == evals.tobytes()
    assert got[3] == sinfo
    assert sum(i["points"] for i in infos) == int(B.N.sum()) and sum(i["new_voxels"] for i in infos) == len(B.keys)
    assert infos[-1]["solved_voxels"] == sinfo["solved_voxels"]
    assert A.poses.tobytes() == np.asarray(poses, np.float64).tobytes()


def test_rows_and_sums_are_the_full_builds_on_the_static_pass(static):
    poses, clouds, B = static
    A, infos = extended(poses, clouds, (4,), CS.STATIC["voxel"], STATIC_CARVE)
    assert same_rows(A.V, B)
    assert (int(B.N.sum()), len(B.keys), infos[0]["new_voxels"]) == (152074, 11557, 7808)
    S, orphans = SN.moments(B, poses, clouds, CS.MASK)
    assert A.S.tobytes() == S.tobytes() and A.orphans == orphans == 0
    # the carve is compositional: the base's counts, then the new keyframes' rays through the map as extended
    M0, _ = CN.carve(CN.build_map(poses[:4], clouds[:4], CS.MASK, CS.STATIC["voxel"]), poses[:4], clouds[:4], CS.MASK, **STATIC_CARVE)
    M1, c1 = CN.carve(B, poses[4:], clouds[4:], CS.MASK, **STATIC_CARVE)
    want = np.concatenate([M0, np.zeros(len(B.keys) - len(M0), np.int64)]) + M1
    assert A.M.tobytes() == want.tobytes()
    assert infos[1]["misses"] == c1["misses"] and A.carve_info["misses"] == int(want.sum())
    Mf, _ = CN.carve(B, poses, clouds, CS.MASK, **STATIC_CARVE)
    assert (int(A.M.sum()), int(Mf.sum())) == (17589, 19064)            # ... which is deliberately not the full carve
    assert (len(CN.read_carved(A.V, A.M)), len(CN.read_carved(B, Mf))) == (11125, 11079)


def test_a_removed_box_is_carved_out_by_the_extension():
    poses, clouds, wall, box = ES.removed()
    v = CS.GHOST["voxel"]
    A = EN.ExtendedMapNP(CS.MASK, v, surfels=True, carve=GHOST_CARVE)
    A.build(poses[:ES.CUT], clouds[:ES.CUT])
    b = box_ids(A.V, box)
    kept = kept_cells(A.V, A.M)
    assert (len(b), len(kept & ES.cells(box, v)), len(kept), len(A.V.keys)) == (27, 20, 192, 199)
    assert (int(A.M[b].min()), int(A.M[b].max())) == (0, 34)
    A.extend(poses[ES.CUT:], clouds[ES.CUT:])
    kept = kept_cells(A.V, A.M)
    assert not kept & ES.cells(box, v)                    # none of the box is kept after its removal ...
    assert kept == ES.cells(wall, v) and len(kept) == 175   # ... and the wall is whole
    assert (int(A.M[b].min()), int(A.M[b].max())) == (27, 111)
    assert same_rows(A.V, CN.build_map(poses, clouds, CS.MASK, v))


def test_an_appeared_box_is_not_held_to_account_for_earlier_rays():
    poses, clouds, wall, box = ES.appeared()
    v = CS.GHOST["voxel"]
    A = EN.ExtendedMapNP(CS.MASK, v, surfels=True, carve=GHOST_CARVE)
    A.build(poses[:ES.CUT], clouds[:ES.CUT])
    A.extend(poses[ES.CUT:], clouds[ES.CUT:])
    B = CN.build_map(poses, clouds, CS.MASK, v)
    Mf, _ = CN.carve(B, poses, clouds, CS.MASK, **GHOST_CARVE)
    assert same_rows(A.V, B)
    b = box_ids(B, box)
    assert len(b) == 27 and b.min() >= 175                # the box's voxels all came with the extension
    assert (A.M[b] <= Mf[b]).all()
    assert (int(A.M[b].min()), int(A.M[b].max()), int(Mf[b].min()), int(Mf[b].max())) == (0, 43, 41, 88)
    ext, full = kept_cells(A.V, A.M), kept_cells(B, Mf)
    assert (len(ext & ES.cells(box, v)), len(full & ES.cells(box, v))) == (17, 1)   # strictly more of it than a full carve keeps
    assert ES.cells(wall, v) <= ext and len(ES.cells(wall, v)) == 175               # the wall whole
