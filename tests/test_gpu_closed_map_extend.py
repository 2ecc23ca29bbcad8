"""-m gpu: the closed map extended in place (tl_extend.hip, tl_api_extend.hip), bit for bit.  Context A builds
from the first keyframes (with surfels and a carve when asked), takes the rest through place_add_scan + place_set_keyframe_clouds
and extends; context B holds every keyframe and does the full build and the full surfel pass.  Rows, ids, surfels, poses, infos,
localisation and the snapshot's bytes are B's; a carved map's M is the restatement's (tests/closed_map_extend_np.py)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_carve_np as CN  # noqa: E402
import closed_map_extend_np as EN  # noqa: E402
import extend_scenes as ES  # noqa: E402
import localise_scenes as LS  # noqa: E402
import relocalise_scenes as RS  # noqa: E402
import test_gpu_closed_map_localise as TL  # noqa: E402
import test_gpu_closed_map_snapshot as TSN  # noqa: E402

pytestmark = pytest.mark.gpu

bits, invalid, not_ready, log_bytes, map_bytes = TL.bits, TL.invalid, TL.not_ready, TL.log_bytes, TSN.map_bytes
DUMMY = np.random.default_rng(5).uniform(-20.0, 20.0, (200, 3))   # the scan a hand-made keyframe is described by
NONE = CS.NONE
GHOST_CUTS = ((1,), (2,), (3,), (5,), (1, 2, 3, 4, 5))
CARVE_KEYS = ("misses", "carved", "carve_info")
COUNTED = ("n_keyframes", "added_keyframes", "empty_keyframes", "overflow_keyframes", "points", "new_voxels", "touched_voxels", "rays",
           "skipped_rays", "steps", "tested", "misses", "solved_voxels")


def new_context(reg, place=None, **cmap_cfg):
    H = reg.HipRegistration()
    H.place_configure(enabled=1, **(place or dict(exclude_recent=8)))
    H.loop_configure(enabled=1)
    H.closed_map_configure(**cmap_cfg)
    return H


def add(H, ks, poses, clouds, scans=None):
    """keyframes ks with their stored poses and clouds"""
    for k in ks:
        assert H.place_add_scan(DUMMY if scans is None else scans[k], poses[k], k) == k
        H.place_set_keyframe_clouds(k, *clouds[k])


def pair(reg, poses, clouds, cuts, surfels=True, carve=None, scans=None, place=None, source=2, **cfg):
    """-> (A: built from the keyframes before cuts[0] and extended at every cut, B: the full build, the extends' infos)"""
    edges = [0, *cuts, len(poses)]
    A = new_context(reg, place, **cfg)
    add(A, range(edges[1]), poses, clouds, scans)
    A.closed_map_build(source, poses[:edges[1]] if source == 2 else None)
    if surfels:
        A.closed_map_surfels()
    if carve is not None:
        A.closed_map_carve_configure(**carve)
        A.closed_map_carve()
    infos = []
    for a, b in zip(edges[1:-1], edges[2:]):
        add(A, range(a, b), poses, clouds, scans)
        infos.append(A.closed_map_extend(source, poses[a:b] if source == 2 else None))
        print(f"extend [{a}, {b}) source {source} surfels {surfels} carve {carve}: {infos[-1]}")
        assert A.closed_map_extend_info() == infos[-1] and infos[-1]["first_keyframe"] == a
    B = new_context(reg, place, **cfg)
    add(B, range(len(poses)), poses, clouds, scans)
    B.closed_map_build(source, poses if source == 2 else None)
    if surfels:
        B.closed_map_surfels()
    return A, B, infos


def same_map(A, B, reg, carved=False):
    """every getter of the closed map and the keyframe database (the carve's aside when A is carved: it is compositional)"""
    got, want = map_bytes(A, reg), map_bytes(B, reg)
    for k in want:
        if not (carved and k in CARVE_KEYS):
            assert got[k] == want[k], k


def restated(poses, clouds, cuts, mask, voxel, origin=(0.0, 0.0, 0.0), surfels=True, carve=None, ray_mask=0):
    R = EN.ExtendedMapNP(mask, voxel, origin, surfels=surfels,
                         carve=None if carve is None else {**CN.DEFAULTS, **{k: v for k, v in carve.items() if k != "ray_mask"}},
                         ray_mask=ray_mask)
    edges = [0, *cuts, len(poses)]
    return R, [R.extend(poses[a:b], clouds[a:b]) for a, b in zip(edges[:-1], edges[1:])]


def same_as_restated(A, R, infos, rinfos):
    """the extends' counters, and of a carved map M and the carve info"""
    for got, want in zip(infos, rinfos[1:]):
        assert {k: got[k] for k in COUNTED} == {k: want[k] for k in COUNTED}
    cen, cnt = A.closed_map_read()
    assert cnt.tobytes() == R.V.N.tobytes() and bits(cen) == bits(R.V.centroids())
    if R.S is not None:
        assert A.closed_map_moments().tobytes() == R.S.tobytes()
    if R.M is not None:
        assert A.closed_map_misses().tobytes() == R.M.tobytes()
        assert {k: v for k, v in A.closed_map_carve_info().items() if k not in ("launches", "reserved0")} == R.carve_info


def queries(H, scan, truth):
    """localisations from section 23's starts with their logs, and a relocalisation, as bytes"""
    out = []
    for s in LS.STARTS:
        pose, info = H.closed_map_localise(scan, LS.offset(truth, *s))
        out.append(bits(pose) + repr(info).encode() + log_bytes(H.closed_map_localise_log()))
    pose, info = H.closed_map_relocalise(scan)
    hyps = H.closed_map_relocalise_hypotheses()
    out.append(bits(pose) + repr(info).encode() +
               repr([sorted((k, bits(v) if isinstance(v, np.ndarray) else v) for k, v in h.items()) for h in hyps]).encode())
    return out


def kept_cells(H, voxel):
    cen, _, _ = H.closed_map_read_carved()
    return ES.cells(cen, voxel)


# ---- 1: against a second context ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", GHOST_CUTS)
def test_the_ghost_cuts(hip_module, cuts):
    poses, clouds, _, _ = CS.ghost_scene()
    v = CS.GHOST["voxel"]
    A, B, infos = pair(hip_module, poses, clouds, cuts, voxel=v, cloud_mask=CS.MASK)
    same_map(A, B, hip_module)
    assert A.closed_map_save() == B.closed_map_save() and A.closed_map_save(clouds=True) == B.closed_map_save(clouds=True)
    R, rinfos = restated(poses, clouds, cuts, CS.MASK, v)
    same_as_restated(A, R, infos, rinfos)
    _, _, scan, truth = LS.wall()
    first = A.closed_map_localise(scan, truth)[1]
    assert first["prepared"] == 1                              # the voxel records went stale with the extension
    B.closed_map_localise(scan, truth)
    assert queries(A, scan, truth) == queries(B, scan, truth)
    assert all(i["grown"] == 0 and i["launches"] == infos[0]["launches"] for i in infos)
    A.close(); B.close()


@pytest.mark.parametrize("name", ["removed", "appeared"])
def test_the_scenes(hip_module, name):
    poses, clouds, wall, box = getattr(ES, name)()
    v, carve = CS.GHOST["voxel"], dict(max_range=CS.GHOST["max_range"])
    A, B, infos = pair(hip_module, poses, clouds, (ES.CUT,), carve=carve, voxel=v, cloud_mask=CS.MASK)
    same_map(A, B, hip_module, carved=True)
    R, rinfos = restated(poses, clouds, (ES.CUT,), CS.MASK, v, carve=carve)
    same_as_restated(A, R, infos, rinfos)
    kept = kept_cells(A, v)
    B.closed_map_carve_configure(**carve)
    full_info = B.closed_map_carve()
    full = kept_cells(B, v)
    if name == "removed":
        assert not kept & ES.cells(box, v) and kept == ES.cells(wall, v)      # none of the box kept, the wall whole
    else:
        assert len(kept & ES.cells(box, v)) > len(full & ES.cells(box, v))    # strictly more of it than the full carve keeps
        assert (len(kept & ES.cells(box, v)), len(full & ES.cells(box, v))) == (17, 1)
        assert ES.cells(wall, v) <= kept
    # a full carve after the extend replaces the counts with the full semantics: B's
    assert A.closed_map_carve() == full_info
    same_map(A, B, hip_module)
    assert A.closed_map_save() == B.closed_map_save()
    A.close(); B.close()
    # never carved: the snapshot's bytes, localisations with their logs and a relocalisation are the full build's
    A, B, _ = pair(hip_module, poses, clouds, (ES.CUT,), voxel=v, cloud_mask=CS.MASK)
    same_map(A, B, hip_module)
    assert A.closed_map_save() == B.closed_map_save() and A.closed_map_save(clouds=True) == B.closed_map_save(clouds=True)
    _, _, scan, truth = LS.wall()
    assert queries(A, scan, truth) == queries(B, scan, truth)
    A.close(); B.close()


@pytest.fixture(scope="module")
def static():
    return RS.static()


def test_the_static_pass_split_4_and_4(hip_module, static):
    poses, clouds, scans, qs = static
    v = CS.STATIC["voxel"]
    A, B, infos = pair(hip_module, poses, clouds, (4,), scans=scans, place=RS.PLACE, voxel=v, cloud_mask=CS.MASK)
    info = A.closed_map_info()
    assert (info["n_points"], info["n_voxels"], infos[0]["new_voxels"]) == (152074, 11557, 11557 - 7808)
    same_map(A, B, hip_module)
    assert A.closed_map_save() == B.closed_map_save()
    scan, truth = qs["as_it_is"]
    assert queries(A, scan, truth) == queries(B, scan, truth)
    A.close(); B.close()


def test_the_static_pass_carved(hip_module, static):
    poses, clouds, scans, _ = static
    v, carve = CS.STATIC["voxel"], dict(max_range=CS.STATIC["max_range"])
    A, B, infos = pair(hip_module, poses, clouds, (4,), carve=carve, voxel=v, cloud_mask=CS.MASK)
    same_map(A, B, hip_module, carved=True)
    R, rinfos = restated(poses, clouds, (4,), CS.MASK, v, carve=carve)
    same_as_restated(A, R, infos, rinfos)
    assert A.closed_map_carve_info()["misses"] == 17589 and len(A.closed_map_read_carved()[1]) == 11125
    A.close(); B.close()


# ---- 2: sizes, masks and the keyframes that add nothing ------------------------------------------------------------------------
def cloud_in(rng, n, lo, hi):
    return rng.uniform(lo, hi, (n, 3))


def slots(*tgt):
    """target slots 0.. of a keyframe (mask 0xF0)"""
    t = [np.ascontiguousarray(c, np.float64).reshape(-1, 3) for c in tgt] + [NONE] * (4 - len(tgt))
    return [[NONE] * 4, t]


def pose_at(x, y, z, yaw=0.0):
    P = np.eye(4)
    P[:3, :3] = LS.rotation([0.0, 0.0, 1.0], yaw)
    P[:3, 3] = [x, y, z]
    return P


def check_pair(reg, poses, clouds, cuts, mask=0xF0, voxel=0.5, carve=None, surfels=True, **cfg):
    poses = np.array(poses)
    carve = dict(max_range=30.0) if carve is None else carve
    A, B, infos = pair(reg, poses, clouds, cuts, surfels=surfels, carve=carve, voxel=voxel, cloud_mask=mask, **cfg)
    same_map(A, B, reg, carved=True)
    R, rinfos = restated(poses, clouds, cuts, mask, voxel, surfels=surfels, carve=carve)
    same_as_restated(A, R, infos, rinfos)
    return A, B, infos


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_new_keyframes_of_every_size(hip_module, n):
    rng = np.random.default_rng(100 + n)
    poses = [pose_at(0.0, 0.0, 1.0), pose_at(1.0, 0.5, 1.0, 0.3)]
    clouds = [slots(cloud_in(rng, 700, -6.0, 6.0)), slots(cloud_in(rng, n, -8.0, 8.0))]
    A, B, infos = check_pair(hip_module, poses, clouds, (1,))
    assert infos[0]["points"] == n and infos[0]["rays"] == n
    A.close(); B.close()


def test_existing_voxels_fresh_voxels_and_runs_across_spans(hip_module):
    rng = np.random.default_rng(7)
    base = cloud_in(rng, 900, -5.0, 5.0)
    I = pose_at(0.0, 0.0, 0.0)
    # every new point in a voxel the map holds: the base's own points again
    A, B, infos = check_pair(hip_module, [I, I], [slots(base), slots(base[::-1])], (1,))
    assert infos[0]["new_voxels"] == 0 and infos[0]["touched_voxels"] == A.closed_map_info()["n_voxels"]
    A.close(); B.close()
    # every new point in a fresh voxel: far from the base
    A, B, infos = check_pair(hip_module, [I, I], [slots(base), slots(base + 40.0)], (1,))
    assert infos[0]["new_voxels"] == infos[0]["touched_voxels"] > 0
    A.close(); B.close()
    # mask 0xF0, four non-empty slots of sorted points: runs of equal keys cross spans and keyframes inside a wave
    line = np.stack([np.linspace(-3.0, 3.0, 50), np.full(50, 0.2), np.full(50, 0.3)], axis=1)
    four = slots(line[:13], line[13:14], line[14:40], line[40:])
    A, B, infos = check_pair(hip_module, [I, I, I, I], [slots(base), four, four, slots(line)], (1, 3))
    assert [i["n_keyframes"] for i in infos] == [2, 1] and infos[0]["points"] == 100
    A.close(); B.close()


def test_keyframes_that_add_nothing_and_points_that_are_left_out(hip_module):
    rng = np.random.default_rng(9)
    I = pose_at(0.0, 0.0, 0.0)
    good = cloud_in(rng, 300, -5.0, 5.0)
    far = np.concatenate([good[:100], [[6e5, 0.0, 0.0]], good[100:200]])      # v = 0.5: beyond the grid
    holes = good.copy()
    holes[5] = [np.nan, 0.0, 0.0]; holes[70] = [0.0, np.inf, 0.0]; holes[299] = [1.0, 1.0, -np.inf]
    clouds = [slots(good), slots(NONE), slots(far), slots(holes), slots(good + 0.25)]
    A, B, infos = check_pair(hip_module, [I] * 5, clouds, (1,))
    i = infos[0]
    assert (i["n_keyframes"], i["added_keyframes"], i["empty_keyframes"], i["overflow_keyframes"], i["points"]) == (4, 2, 1, 1, 597)
    info = A.closed_map_info()
    assert (info["n_keyframes"], info["added_keyframes"], info["empty_keyframes"], info["overflow_keyframes"]) == (5, 3, 1, 1)
    A.close(); B.close()


def test_the_rows_grow_inside_the_call(hip_module):
    poses, clouds, _, _ = ES.appeared()
    v, carve = CS.GHOST["voxel"], dict(max_range=CS.GHOST["max_range"])
    A, B, infos = pair(hip_module, poses, clouds, (1, 3), carve=carve, voxel=v, cloud_mask=CS.MASK, reserve_voxels=64)
    C, D, plain = pair(hip_module, poses, clouds, (1, 3), carve=carve, voxel=v, cloud_mask=CS.MASK)
    # (the build sized the rows for the first keyframe's 154 voxels; the wall's other 21 do not fit, the box's 27 then do)
    assert [i["grown"] for i in infos] == [1, 0] and [i["grown"] for i in plain] == [0, 0]
    assert A.closed_map_info()["capacity_voxels"] >= 202 > 64
    assert [{k: i[k] for k in COUNTED} for i in infos] == [{k: i[k] for k in COUNTED} for i in plain]
    assert [i["launches"] - p["launches"] for i, p in zip(infos, plain)] == [1, 0]   # the rehash
    same_map(A, B, hip_module, carved=True)
    got, want = map_bytes(A, hip_module), map_bytes(C, hip_module)
    assert all(got[k] == want[k] for k in want)
    assert A.closed_map_save() == C.closed_map_save()
    for H in (A, B, C, D):
        H.close()


def test_an_empty_map_grows(hip_module):
    """no row to copy or rehash: the launches are still those of a grown call"""
    rng = np.random.default_rng(21)
    I = pose_at(0.0, 0.0, 0.0)
    clouds = [slots(NONE), slots(cloud_in(rng, 900, -6.0, 6.0))]
    A, B, infos = check_pair(hip_module, [I, I], clouds, (1,), reserve_voxels=64)
    assert A.closed_map_info()["empty_keyframes"] == 1 and infos[0]["new_voxels"] == infos[0]["touched_voxels"] > 64
    assert infos[0]["grown"] == 1 and infos[0]["launches"] == 5 + 2 + 2 + 1
    A.close(); B.close()


def test_nothing_to_take_and_two_successive_extends(hip_module):
    poses, clouds, _, _ = CS.ghost_scene()
    v = CS.GHOST["voxel"]
    A, B, infos = pair(hip_module, poses, clouds, (2, 4), carve=dict(max_range=CS.GHOST["max_range"]), voxel=v, cloud_mask=CS.MASK)
    before = map_bytes(A, hip_module)
    blob = A.closed_map_save()
    for source, P in ((0, None), (2, np.zeros((0, 4, 4)))):
        info = A.closed_map_extend(source, P)
        assert (info["first_keyframe"], info["n_keyframes"], info["points"], info["launches"]) == (6, 0, 0, 0)
        assert info["solved_voxels"] == A.closed_map_surfel_info()["solved_voxels"]
        assert map_bytes(A, hip_module) == before and A.closed_map_save() == blob
    same_map(A, B, hip_module, carved=True)
    A.close(); B.close()


def test_the_stored_poses(hip_module):
    poses, clouds, _, _ = ES.removed()
    v = CS.GHOST["voxel"]
    A, B, _ = pair(hip_module, poses, clouds, (ES.CUT,), voxel=v, cloud_mask=CS.MASK, source=0)
    C, D, _ = pair(hip_module, poses, clouds, (ES.CUT,), voxel=v, cloud_mask=CS.MASK, source=2)
    same_map(A, B, hip_module)
    assert A.closed_map_info()["pose_source"] == 0 and C.closed_map_info()["pose_source"] == 2
    assert map_bytes(A, hip_module)["read"] == map_bytes(C, hip_module)["read"]
    for H in (A, B, C, D):
        H.close()


def test_the_corrected_poses(hip_module):
    """pose_source 1 is the build's rule: a keyframe behind the last optimise takes the last correction, a later optimise's
    corrected pose is used as it is"""
    poses, clouds, _, _ = ES.removed()
    v = CS.GHOST["voxel"]
    A, B = (new_context(hip_module, voxel=v, cloud_mask=CS.MASK) for _ in range(2))
    for H in (A, B):
        add(H, range(ES.CUT), poses, clouds)
        H.graph_optimize()
    A.closed_map_build(1)
    A.closed_map_surfels()
    for H in (A, B):
        add(H, range(ES.CUT, 5), poses, clouds)
    info = A.closed_map_extend(1)
    B.closed_map_build(1)
    B.closed_map_surfels()
    assert info["n_keyframes"] == 2 and A.closed_map_info()["pose_source"] == 1
    same_map(A, B, hip_module)
    stored = A.place_read_keyframes()["poses"]
    used = A.closed_map_poses()
    for k in range(ES.CUT, 5):
        assert bits(used[k]) == bits(A.graph_correct_pose(-1, stored[k])), k
    # after another optimise the new keyframe is one the graph covers
    add(A, [5], poses, clouds)
    A.graph_optimize()
    A.closed_map_extend(1)
    assert bits(A.closed_map_poses(5, 1)[0]) == bits(A.graph_poses()[5]) and bits(A.closed_map_poses(0, 5)) == bits(used)
    add(B, [5], poses, clouds)
    B.closed_map_build(2, A.closed_map_poses())
    B.closed_map_surfels()
    got, want = map_bytes(A, hip_module), map_bytes(B, hip_module)
    assert all(got[k] == want[k] for k in want if k != "info")
    A.close(); B.close()


# ---- 3: launches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("surfels,carved", [(False, False), (True, False), (False, True), (True, True)])
def test_the_launches_depend_on_the_sections_alone(hip_module, surfels, carved):
    rng = np.random.default_rng(3)
    I = pose_at(0.0, 0.0, 0.0)
    seen = []
    for n in (5, 3000):
        clouds = [slots(cloud_in(rng, 500, -5.0, 5.0)), slots(cloud_in(rng, n, -9.0, 9.0))]
        H = new_context(hip_module, voxel=0.5)
        add(H, [0], [I, I], clouds)
        H.closed_map_build(2, [I])
        if surfels:
            H.closed_map_surfels()
        if carved:
            H.closed_map_carve()
        add(H, [1], [I, I], clouds)
        info = H.closed_map_extend(2, [I])
        seen.append(info["launches"])
        assert info["points"] == n and H.closed_map_info()["launches"] == 4
        H.close()
    assert seen[0] == seen[1] == 5 + 2 * surfels + 2 * carved


# ---- 4: the other state -----------------------------------------------------------------------------------------------------
def test_the_records_go_stale_and_the_diff_counts_go(hip_module):
    poses, clouds, _, _ = CS.ghost_scene()
    _, _, scan, truth = LS.wall()
    H = new_context(hip_module, voxel=CS.GHOST["voxel"], cloud_mask=CS.MASK)
    add(H, range(3), poses, clouds)
    H.closed_map_build(2, poses[:3])
    H.closed_map_surfels()
    assert H.closed_map_localise(scan, truth)[1]["prepared"] == 1
    assert H.closed_map_localise(scan, truth)[1]["prepared"] == 0
    H.closed_map_diff(scan, truth)
    assert H.closed_map_diff_info()["scans"] == 1
    H.closed_map_diff_counts()
    place, loop, kf = H.place_info(), H.loop_info(), TSN.cat(v for _, v in sorted(H.place_read_keyframes().items()))
    add(H, range(3, 6), poses, clouds)
    H.closed_map_extend(2, poses[3:])
    assert H.closed_map_diff_info()["scans"] == 0
    with not_ready(hip_module):
        H.closed_map_diff_counts()
    assert H.closed_map_diff(scan, truth)[-1]["prepared"] == 1
    assert H.closed_map_localise(scan, truth)[1]["prepared"] == 0
    assert len(H.closed_map_poses()) == 6 and bits(H.closed_map_poses(3, 3)) == bits(poses[3:])
    assert H.place_info()["n_keyframes"] == place["n_keyframes"] + 3 and H.place_info()["n_loops"] == place["n_loops"]
    assert TSN.cat(v[:3] for _, v in sorted(H.place_read_keyframes().items())) == kf
    H.close()


def test_a_detached_map_extends(hip_module):
    poses, clouds, _, _ = ES.removed()
    v, carve = CS.GHOST["voxel"], dict(max_range=CS.GHOST["max_range"])
    A, B, _ = pair(hip_module, poses, clouds, (ES.CUT,), voxel=v, cloud_mask=CS.MASK)
    base = new_context(hip_module, voxel=v, cloud_mask=CS.MASK)
    add(base, range(ES.CUT), poses, clouds)
    base.closed_map_build(2, poses[:ES.CUT])
    base.closed_map_surfels()
    D = TSN.loaded(hip_module, base.closed_map_save())                            # without its clouds
    add(D, range(ES.CUT, 6), poses, clouds)
    info = D.closed_map_extend(2, poses[ES.CUT:])
    assert info["first_keyframe"] == ES.CUT and info["n_keyframes"] == 6 - ES.CUT
    same_map(D, B, hip_module)
    for call in (lambda: D.closed_map_build(2, poses), D.closed_map_carve, D.closed_map_surfels):
        with not_ready(hip_module):
            call()
    same_map(D, B, hip_module)
    blob = D.closed_map_save()
    assert blob == B.closed_map_save() == A.closed_map_save()
    E = TSN.loaded(hip_module, blob)
    same_map(E, B, hip_module)
    for H in (A, B, base, D, E):
        H.close()


def test_refusals_leave_every_byte(hip_module):
    reg = hip_module
    poses, clouds, _, _ = CS.ghost_scene()
    v = CS.GHOST["voxel"]
    H = new_context(reg, voxel=v, cloud_mask=CS.MASK)
    add(H, range(3), poses, clouds)
    with not_ready(reg):
        H.closed_map_extend(2, poses[:3])                       # no built map
    H.closed_map_build(2, poses[:3])
    H.closed_map_surfels()
    H.closed_map_carve()
    add(H, range(3, 6), poses, clouds)
    before, blob = map_bytes(H, reg), H.closed_map_save(clouds=True)
    bad = np.array(poses[3:])
    nan, shear = bad.copy(), bad.copy()
    nan[1, 0, 3] = np.nan
    shear[2, 0, 1] = 0.5
    for call in (lambda: H.closed_map_extend(3), lambda: H.closed_map_extend(-1), lambda: H.closed_map_extend(2, poses[3:5]),
                 lambda: H.closed_map_extend(2, poses), lambda: H.closed_map_extend(2), lambda: H.closed_map_extend(2, nan),
                 lambda: H.closed_map_extend(2, shear)):
        with invalid(reg):
            call()
        assert map_bytes(H, reg) == before and H.closed_map_save(clouds=True) == blob
    with not_ready(reg):
        H.closed_map_extend(1)                                   # no optimise
    assert map_bytes(H, reg) == before and H.closed_map_save(clouds=True) == blob
    assert H.closed_map_extend_info()["n_keyframes"] == 0
    info = H.closed_map_extend(2, poses[3:])
    assert info["n_keyframes"] == 3 and H.closed_map_info()["n_keyframes"] == 6
    H.close()
    # keyframe clouds off: there is nothing to extend from
    H = reg.HipRegistration()
    H.place_configure(enabled=1, exclude_recent=8)
    with invalid(reg):
        H.closed_map_extend(0)
    H.close()
    # single-GPU only
    H = reg.HipRegistration()
    H.comm_init_callback(0, 2, lambda dev, count, stream: 0)
    for call in (H.closed_map_extend, lambda: H.closed_map_extend(2, poses[3:]), H.closed_map_extend_info):
        with invalid(reg):
            call()
    H.close()
