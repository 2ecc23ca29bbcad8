"""The ray-cast of the closed map without a GPU: its numpy restatement (tests/closed_map_raycast_np.py) on
the wall against analytic ranges, on the ghost gate and on the static pass.  Every integer here is one the restatement gives;
the device is held to the same results bit for bit (tests/test_gpu_closed_map_raycast.py)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_carve_np as CN  # noqa: E402
import closed_map_raycast_np as RN  # noqa: E402
import diff_scenes as DS  # noqa: E402
import localise_scenes as LS  # noqa: E402
import raycast_scenes as RS  # noqa: E402
from tloam_amd import raycast as RC  # noqa: E402


def test_the_restatement_borrows_the_walk_the_records_and_the_transform():
    src = open(os.path.join(HERE, "closed_map_raycast_np.py")).read()
    assert "CN.Walk(" in src and "CN.transform(" in src and "T.find(" in src and "T.eligible" in src
    assert "class Walk" not in src and "class Target" not in src and "def transform" not in src and "searchsorted" not in src


def test_the_pattern():
    ends = RS.pattern()
    assert ends.shape == (2880, 3) and ends.flags["C_CONTIGUOUS"] and ends.dtype == np.float64
    assert np.allclose(np.linalg.norm(ends, axis=1), RS.LENGTH, rtol=0, atol=1e-12)
    el = np.arcsin(ends[:, 2] / RS.LENGTH).reshape(16, 180)
    assert np.allclose(el, el[:, :1]) and np.allclose(el[:, 0], np.linspace(-0.3, 0.3, 16))   # ring-major
    az = np.arctan2(ends[:180, 1], ends[:180, 0]) % (2.0 * np.pi)
    assert np.allclose(az, 2.0 * np.pi * np.arange(180) / 180)
    assert RC.lidar_pattern(1, 4, 0.1, 0.2, 2.0).shape == (4, 3)
    with pytest.raises(ValueError):
        RC.lidar_pattern(0, 4, 0.0, 0.0, 1.0)


@pytest.fixture(scope="module")
def wall():
    poses, clouds, _, _ = LS.wall()
    V, _, _, _, T = LS.target(poses, clouds, CS.MASK, DS.VOXEL)
    assert len(V.keys) == 175 and int(T.eligible.sum()) == 144
    return V, T


# rays of the on-wall set that leak through, per sensor, at radius_cells (1.0, 0.75, 0.5) and planes (0, 1)
LEAKS = {0: {1.0: (0, 0), 0.75: (1, 3), 0.5: (94, 127)}, 1: {1.0: (0, 0), 0.75: (1, 3), 0.5: (94, 128)},
         2: {1.0: (0, 0), 0.75: (0, 0), 0.5: (49, 74)}}


@pytest.mark.parametrize("k,n_on", zip(range(3), (501, 490, 390)))
def test_the_wall_against_analytic_ranges(wall, k, n_on):
    V, T = wall
    sensor = DS.SENSORS[k]
    ends, pose = RS.pattern(), DS.pose_at(sensor)
    t, on, off = RS.wall_ranges(sensor)
    assert int(on.sum()) == n_on and not (on & off).any() and off.sum() > 2000
    for radius_cells in (1.0, 0.75, 0.5):
        for planes in (0, 1):
            R = RN.cast(T, V, ends, pose, dict(radius_cells=radius_cells, planes=planes))
            hit = R["status"] >= RN.HIT_CENTROID
            err = np.abs(R["ranges"][on & hit] - t[on & hit])
            print(f"sensor {k} radius_cells {radius_cells} planes {planes}: leaks {int((on & ~hit).sum())} max error {err.max():.3g}"
                  f" {R['info']}")
            assert not (off & hit).any()                                        # at every radius: no off-wall ray hits
            assert int((on & ~hit).sum()) == LEAKS[k][radius_cells][planes]
            if radius_cells == 1.0:
                assert hit[on].all()                                            # the condition: every on-wall ray hits
            if planes == 1:
                assert (R["status"][on & hit] == RN.HIT_PLANE).all() and err.max() <= 1e-6
            else:
                assert (R["status"][hit] == RN.HIT_CENTROID).all() and err.max() < V.voxel / 2
            assert (R["ranges"][~hit] == -1.0).all() and (R["ids"][~hit] == -1).all() and (R["ids"][hit] >= 0).all()
            I = R["info"]
            assert I["rays"] == 2880 == I["skipped"] + I["missed"] + I["hits_centroid"] + I["hits_plane"] and I["skipped"] == 0
    R = RN.cast(T, V, ends, DS.pose_at(DS.SENSORS[0]), dict(radius_cells=1.0, planes=0))
    assert (R["info"]["steps"], R["info"]["tested"]) == (83497, 641)


def test_planes_two_never_returns_a_centroid_hit(wall):
    V, T = wall
    ends, pose = RS.pattern(), DS.pose_at(DS.SENSORS[0])
    one = RN.cast(T, V, ends, pose, dict(planes=1))
    two = RN.cast(T, V, ends, pose, dict(planes=2))
    assert one["info"]["hits_centroid"] == 24 and two["info"]["hits_centroid"] == 0 and not (two["status"] == RN.HIT_CENTROID).any()
    assert two["info"]["hits_plane"] == one["info"]["hits_plane"] == 613
    assert two["info"]["tested"] < one["info"]["tested"] and two["info"]["steps"] > one["info"]["steps"]


def test_min_count_lets_the_ray_through(wall):
    V, T = wall
    ends, pose = RS.pattern(), DS.pose_at(DS.SENSORS[0])
    base = RN.cast(T, V, ends, pose)
    hit = np.flatnonzero(base["status"] >= RN.HIT_CENTROID)
    g = hit[0]
    N = int(V.N[base["ids"][g]])
    same = RN.cast(T, V, ends[g:g + 1], pose, dict(min_count=N))
    through = RN.cast(T, V, ends[g:g + 1], pose, dict(min_count=N + 1))
    assert same["ids"][0] == base["ids"][g] and through["ids"][0] != base["ids"][g]
    none = RN.cast(T, V, ends, pose, dict(min_count=int(V.N.max()) + 1))
    assert (none["status"] == RN.MISS).all() and none["info"]["tested"] == 0


def test_a_cast_is_the_concatenation_of_its_halves(wall):
    V, T = wall
    ends, pose = RS.pattern(), LS.offset(DS.pose_at(DS.SENSORS[2]), 0.3, 0.02)
    whole = RN.cast(T, V, ends, pose)
    a, b = RN.cast(T, V, ends[:1337], pose), RN.cast(T, V, ends[1337:], pose)
    for key in ("status", "ranges", "ids"):
        assert whole[key].tobytes() == a[key].tobytes() + b[key].tobytes()
    assert whole["info"] == {k: a["info"][k] + b["info"][k] for k in whole["info"]}


def test_skipped_rays(wall):
    V, T = wall
    pose = DS.pose_at(DS.SENSORS[0])
    ends = np.array([[np.nan, 1.0, 1.0], [np.inf, 0.0, 0.0], [2.0 ** 19 + 5.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 121.0, 0.0],
                     [0.0, 8.0, 0.0]])
    R = RN.cast(T, V, ends, pose)
    assert list(R["status"]) == [RN.SKIPPED] * 5 + [RN.HIT_PLANE] and R["info"]["skipped"] == 5
    assert (R["ranges"][:5] == -1.0).all() and (R["ids"][:5] == -1).all() and abs(R["ranges"][5] - 5.0) < 1e-9


def test_the_ghost_gate():
    poses, clouds, _, pose, _ = DS.ghost_gate()
    V, _, _, _, T = LS.target(poses, clouds, CS.MASK, DS.VOXEL)
    M, _ = CN.carve(V, poses, clouds, CS.MASK, max_range=DS.MAX_RANGE)
    box = DS.box_voxels(V)
    assert len(box) == 8
    aim = V.centroids()[box] - pose[:3, 3]
    r = np.linalg.norm(aim, axis=1)
    ends = aim * ((r + 6.0) / r)[:, None]          # through each box voxel's centroid and on past the wall
    for planes in (0, 1):
        off = RN.cast(T, V, ends, pose, dict(planes=planes, carve_gate=0), misses=M)
        on = RN.cast(T, V, ends, pose, dict(planes=planes, carve_gate=1), misses=M)
        assert np.isin(off["ids"], box).all() and (off["status"] == RN.HIT_CENTROID).all()   # (the box's voxels hold no plane)
        assert not np.isin(on["ids"], box).any()
        assert (on["status"] == (RN.HIT_PLANE if planes else RN.HIT_CENTROID)).all() and (on["ranges"] > 5.0).all()
        assert (off["ranges"] < 2.2).all()


@pytest.fixture(scope="module")
def static():
    poses, clouds = CS.static_pass()
    scan, truth = LS.static_scan(poses)
    V, _, _, _, T = LS.target(poses, clouds, CS.MASK, CS.STATIC["voxel"])
    return V, T, scan, truth


def test_the_static_figures(static):
    """no bar: the figures DESIGN.md section 28 quotes, recorded.  The counts are the restatement's integers."""
    V, T, scan, truth = static
    assert len(V.keys) == 11557 and int(T.eligible.sum()) == 4069 and len(scan) == 18988
    counts = {}
    for planes in (1, 2, 0):
        status, dr = RC.scan_check(RN.Handle(T, V, dict(planes=planes)), scan, truth, extend=2.0)
        counts[planes] = tuple(int((status == k).sum()) for k in range(4))
        for k, name in ((RN.HIT_CENTROID, "centroid"), (RN.HIT_PLANE, "plane")):
            sel = status == k
            if sel.any():
                a = np.abs(dr[sel])
                print(f"planes {planes} {name} hits {int(sel.sum())}: median |predicted - measured| {np.median(a):.4f} m, p90 "
                      f"{np.percentile(a, 90):.4f} m, short by more than 0.5 m {float((dr[sel] < -0.5).mean()):.4f}")
        assert np.isnan(dr[status < RN.HIT_CENTROID]).all() and np.isfinite(dr[status >= RN.HIT_CENTROID]).all()
    assert counts == {1: (0, 201, 2223, 16564), 2: (0, 1504, 0, 17484), 0: (0, 168, 18820, 0)}
