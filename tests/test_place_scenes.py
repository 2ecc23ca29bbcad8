"""The scenes of tests/place_scenes.py on the numpy restatement (CPU): every scene's margin report holds exactly the returns it
declares (none, but for axis_clamps), the restatement describes every scan as the descriptor it was made from, to the bit,
and the witness shows that the branch the scene is named for is reached -- the tie is a tie, the clamp is hit, nv == 0
occurs.  Keeps tests/test_gpu_place_edges.py from going vacuous when a helper changes."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import place_np as P  # noqa: E402
import place_scenes as SC  # noqa: E402


@pytest.mark.parametrize("R,S", [(1, 2), (4, 8), (7, 37), (20, 60), (64, 360)])
def test_scan_of_gives_the_descriptor_back(R, S):
    for over in (dict(), dict(max_radius=50.0, height_offset=-1.5)):
        grid = SC.grid_of(n_rings=R, n_sectors=S, **over)
        d = SC.dyadic(R * S, R, S, lo=0)          # (some bins empty)
        d64 = SC.dyadic(R + S, R, S, lo=-64, hi=65, step=64.0)   # negative values, multiples of 1 / 64
        for want in (d, d64):
            xyz = SC.scan_of(want, **grid)
            assert len(xyz) == np.count_nonzero(want)
            assert len(P.margins(xyz, **grid)) == 0
            got, rk, sk = P.describe(xyz, **grid)
            assert SC.bits(got) == SC.bits(want)
            assert SC.bits(rk) == SC.bits(P.keys(want)[0]) and SC.bits(sk) == SC.bits(P.keys(want)[1])


@pytest.mark.parametrize("name", SC.DESC_NAMES)
def test_descriptor_scene(name):
    sc = SC.desc_scene(name)
    assert sc.name == name
    assert list(P.margins(sc.xyz, **sc.grid)) == list(sc.boundary)
    assert SC.bits(SC.described(name)[0]) == SC.bits(sc.desc)
    assert sc.witness(sc.xyz, sc.grid)


def test_only_axis_clamps_declares_boundary_returns():
    for name in SC.DESC_NAMES:
        sc = SC.desc_scene(name)
        if name.startswith("axis_clamps"):
            assert 3 <= len(sc.boundary) <= 5 and max(sc.boundary) < SC.AXIS_USED
            y = sc.xyz[list(sc.boundary), 1]
            assert (y == 0.0).all()   # only atan2's IEEE special values sit on a sector boundary
        else:
            assert sc.boundary == ()
    assert {n for n in SC.DESC_NAMES if n.startswith("axis_clamps")} == {f"axis_clamps_{R}x{S}" for R, S in SC.AXIS_GRIDS}


def test_runs_cover_every_length_and_position():
    table, end = SC.run_table()
    assert sorted({L for _, L, *_ in table}) == sorted(SC.RUN_LENGTHS) and len(table) == 21
    for L in (63, 64, 65, 256, 257):
        assert {p for _, l, p, *_ in table if l == L} == {0, L // 2, L - 1}
    tops = [t for *_, t in table]
    assert tops == sorted(tops, reverse=True) and min(tops) > 5.0   # earlier runs hold the larger maxima


def test_two_turns_size():
    sc = SC.desc_scene("two_turns")
    assert len(sc.xyz) == 262144 + 3 * 256 + 17 == SC.TWO_TURNS_N
    assert sc.xyz.nbytes < 7e6


@pytest.mark.parametrize("name", SC.DB_NAMES)
def test_database_scene(name):
    sc = SC.db_scene(name)
    assert sc.name == name and len(sc.scans) == len(sc.descs)
    grid = SC.grid_of(**{k: v for k, v in sc.cfg.items() if k in SC.GRID_KEYS})
    db = SC.restated(name)
    for k, (xyz, want) in enumerate(zip(sc.scans, sc.descs)):
        assert want.shape == (grid["n_rings"], grid["n_sectors"])
        assert len(P.margins(xyz, **grid)) == 0, k
        assert SC.bits(db.desc[k]) == SC.bits(want), k
    assert db.frames == list(range(SC.FIRST_FRAME, SC.FIRST_FRAME + len(sc.scans)))
    assert sc.witness(db, sc.descs)


def test_scene_names_cover_every_family():
    fam = {n.split("_")[0] for n in SC.DESC_NAMES + SC.DB_NAMES}
    assert {"axis", "heights", "runs", "two", "rank", "shift", "pick", "yaw", "empty", "threshold", "recent", "grids",
            "many"} <= fam
    assert {f"grids_{R}x{S}" for R, S in [(1, 2), (7, 37), (20, 64), (20, 65), (64, 360), (20, 60)]} <= set(SC.DB_NAMES)
    assert SC.db_scene("grids_7x37").cfg["num_candidates"] == 32
    many = SC.db_scene("many")
    assert len(many.scans) == 600 and many.device == dict(reserve_keyframes=4) and many.cfg["num_candidates"] == 32
    assert max(len(s) for s in many.scans) <= 32
