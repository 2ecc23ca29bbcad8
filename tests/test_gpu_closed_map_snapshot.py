"""-m gpu: the closed map's snapshot (tl_snapshot.hip, tl_api_snapshot.hip): a context that loads a saved
closed map answers every read and every localisation with the bytes of the context that saved; the blob is the one the numpy
restatement (tests/closed_map_snapshot_np.py) packs; a blob that is not well-formed is refused and leaves the context as it was."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_snapshot_np as SN  # noqa: E402
import localise_scenes as LS  # noqa: E402
import relocalise_scenes as RS  # noqa: E402
import test_gpu_closed_map_localise as TL  # noqa: E402
import test_gpu_closed_map_relocalise as TR  # noqa: E402
import test_gpu_closed_map_surfel as TS  # noqa: E402
from tloam_amd import map_io  # noqa: E402

pytestmark = pytest.mark.gpu

bits, invalid, not_ready, log_bytes = TL.bits, TL.invalid, TL.not_ready, TL.log_bytes
BOX = dict(lo=[-30.0, -30.0, -5.0], hi=[30.0, 30.0, 5.0])
WORLD = dict(lo=[-1e7] * 3, hi=[1e7] * 3)


def cat(arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def less(info):
    return {k: v for k, v in info.items() if k != "capacity_voxels"}


def map_bytes(H, reg):
    """every getter of the closed map and the keyframe database, as bytes; a section that is not there is NOT_READY"""
    out = {"read": cat(H.closed_map_read()), "box": cat(H.closed_map_read_box(BOX["lo"], BOX["hi"], 2)),
           "poses": bits(H.closed_map_poses()), "info": less(H.closed_map_info())}
    kf = H.place_read_keyframes()
    out["keyframes"] = cat(kf[k] for k in sorted(kf))
    out["place"] = {k: v for k, v in H.place_info().items() if k != "capacity_keyframes"}
    out["carve_info"], out["surfel_info"] = H.closed_map_carve_info(), H.closed_map_surfel_info()
    try:
        out["misses"] = H.closed_map_misses().tobytes()
        out["carved"] = cat(H.closed_map_read_carved()) + cat(H.closed_map_read_carved(**BOX, min_count=2, min_miss=1, miss_ratio=0.5))
    except reg.TloamHipError as e:
        assert "TLOAM_E_NOT_READY" in str(e)
        out["misses"] = out["carved"] = None
    try:
        out["moments"] = H.closed_map_moments().tobytes()
        out["surfels"] = cat(H.closed_map_read_surfels())
        out["surfels_box"] = cat(H.closed_map_read_surfels_box()) + cat(H.closed_map_read_surfels_box(**TS.READS[1]))
    except reg.TloamHipError as e:
        assert "TLOAM_E_NOT_READY" in str(e)
        out["moments"] = out["surfels"] = out["surfels_box"] = None
    return out


def check_unpacked(H, blob):
    """the blob through the numpy reader against the context's own getters -> the dict"""
    d = SN.unpack(blob)
    cen, cnt = H.closed_map_read()
    assert cnt.tobytes() == d["N"].tobytes()
    assert bits(cen) == bits(SN.centroid(d["key"], d["N"], d["Q"], d["cmap"]["voxel"], d["cmap"]["origin"]))
    assert bits(H.closed_map_poses()) == bits(d["poses"])
    info = H.closed_map_info()
    assert less(info) == less(d["info"]) and d["info"]["capacity_voxels"] == 0
    kf = H.place_read_keyframes()
    assert kf["frames"].tobytes() == d["frames"].tobytes() and bits(kf["poses"]) == bits(d["kf_poses"])
    assert bits(kf["ring_keys"]) == bits(d["ring_keys"]) and bits(kf["sector_keys"]) == bits(d["sector_keys"])
    assert bits(kf["descriptors"]) == bits(d["descriptors"])
    if d["M"] is not None:
        assert H.closed_map_misses().tobytes() == d["M"].tobytes() and H.closed_map_carve_info() == d["carve_info"]
    if d["sums"] is not None:
        assert H.closed_map_moments().tobytes() == d["sums"].tobytes() and H.closed_map_surfel_info() == d["surfel_info"]
    for name in ("place", "loop", "cmap", "carve", "surfel"):
        assert d[name]["reserved0"] == 0
    assert d["place"]["reserve_keyframes"] == d["loop"]["reserve_points"] == d["cmap"]["reserve_voxels"] == 0
    assert SN.pack(d) == blob
    return d


def loaded(reg, blob):
    """a fresh context -- no configure call, nothing built -- with the blob loaded"""
    B = reg.HipRegistration()
    assert B.place_info() == dict(n_keyframes=0, n_loops=0, last_keyframe_frame=-1, capacity_keyframes=0)
    with not_ready(reg):
        B.closed_map_read()
    info = B.closed_map_load(blob)
    assert info == reg.closed_map_probe(blob) and info["bytes"] == len(blob)
    return B


# ---- the scenes, built once --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def static(hip_module):
    """A: the static pass built, carved and surfelled; its blob; B: a fresh context that loaded it"""
    poses, clouds, scans, queries = RS.static()
    A = TR.context(hip_module, poses, clouds, scans)
    A.closed_map_build(2, poses)
    A.closed_map_carve_configure(max_range=CS.STATIC["max_range"])
    A.closed_map_carve()
    A.closed_map_surfels()
    blob = A.closed_map_save()
    B = loaded(hip_module, blob)
    yield A, B, blob, poses, queries
    A.close(); B.close()


def corner_context(reg, carve=True, surfels=True):
    poses, clouds, scan, truth = LS.corner()
    H = TS.context(reg, poses, clouds, voxel=LS.CORNER["voxel"], origin=(0.0, 0.0, 0.0), cloud_mask=CS.MASK)
    H.closed_map_build(2, poses)
    if carve:
        H.closed_map_carve()
    if surfels:
        H.closed_map_surfels()
    return H, poses, clouds, scan, truth


@pytest.fixture(scope="module")
def corner(hip_module):
    H, poses, clouds, scan, truth = corner_context(hip_module)
    yield H, poses, scan, LS.offset(truth, *LS.CORNER_START)
    H.close()


# ---- 1: the round trip on the static pass ------------------------------------------------------------------------------------
def test_round_trip_on_the_static_pass(static, hip_module):
    A, B, blob, poses, _ = static
    info = A.closed_map_info()
    assert (info["n_keyframes"], info["n_voxels"]) == (CS.STATIC_KEYFRAMES, 11557)
    want, got = map_bytes(A, hip_module), map_bytes(B, hip_module)
    assert all(v is not None for v in want.values())
    for k in want:
        assert got[k] == want[k], k
    check_unpacked(A, blob)
    assert B.closed_map_save() == blob and A.closed_map_save() == blob
    probe = hip_module.closed_map_probe(blob)
    assert (probe["n_voxels"], probe["has_carve"], probe["has_surfels"], probe["has_clouds"]) == (11557, 1, 1, 0)


# ---- 2: localisation in the loaded map is the saver's ------------------------------------------------------------------------
def test_localisation_is_the_savers(static):
    A, B, blob, poses, queries = static
    scan, truth = queries["as_it_is"]
    starts = [LS.offset(truth, *s) for s in LS.STARTS]
    out = []
    for H in (A, B):
        r = []
        pose, info = H.closed_map_localise(scan, starts[0])
        for at, tau in ((starts[0], 1.0), (pose, 0.1)):
            lin = H.closed_map_linearise(scan, at, tau)
            r.append(cat([lin["ids"], lin["residuals"], lin["H"], lin["g"]]) + bits([lin["cost"]]) + repr((lin["matched"], lin["used"])).encode())
        for s in starts:
            pose, info = H.closed_map_localise(scan, s)
            r.append(bits(pose) + repr(info).encode() + log_bytes(H.closed_map_localise_log()))
        bposes, binfos, best = H.closed_map_localise_batch(scan, np.array(starts[:3]))
        r.append(bits(bposes) + repr((binfos, best)).encode() + b"".join(log_bytes(H.closed_map_localise_batch_log(h)) for h in range(3)))
        for name in RS.TURNS:
            pose, info = H.closed_map_relocalise(queries[name][0])
            hyps = H.closed_map_relocalise_hypotheses()
            r.append(bits(pose) + repr(info).encode() + repr([sorted((k, bits(v) if isinstance(v, np.ndarray) else v) for k, v in h.items())
                                                               for h in hyps]).encode() +
                     b"".join(log_bytes(H.closed_map_localise_batch_log(h)) for h in range(len(hyps))))
            assert info["status"] == 0 and info["n_hypotheses"] == 8
        out.append(r)
    assert len(out[0]) == 2 + 4 + 1 + 4
    for i, (a, b) in enumerate(zip(*out)):
        assert a == b, i


# ---- 3: the optional sections ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("carve,surfels", [(True, False), (False, True), (False, False)])
def test_absent_sections_stay_absent(hip_module, carve, surfels):
    A, poses, clouds, scan, truth = corner_context(hip_module, carve, surfels)
    blob = A.closed_map_save()
    n = hip_module.C.c_size_t(0)
    assert A.L.tloam_closed_map_save_size(A.h, 0, hip_module.C.byref(n)) == 0 and n.value == len(blob)
    B = loaded(hip_module, blob)
    want, got = map_bytes(A, hip_module), map_bytes(B, hip_module)
    assert (want["misses"] is not None, want["moments"] is not None) == (carve, surfels)
    assert got == want and B.closed_map_save() == blob
    d = check_unpacked(A, blob)
    assert (d["M"] is not None, d["sums"] is not None, d["clouds"]) == (carve, surfels, None)
    for H in (A, B):
        if not surfels:
            with not_ready(hip_module):
                H.closed_map_localise(scan, truth)
    A.close(); B.close()


def test_with_clouds_the_loaded_map_can_be_built_again(hip_module, corner):
    A, poses, scan, prior = corner
    blob = A.closed_map_save(clouds=True)
    n = hip_module.C.c_size_t(0)
    assert A.L.tloam_closed_map_save_size(A.h, 1, hip_module.C.byref(n)) == 0 and n.value == len(blob)
    d = check_unpacked(A, blob)
    B = loaded(hip_module, blob)
    want = map_bytes(A, hip_module)
    assert map_bytes(B, hip_module) == want and B.closed_map_save(clouds=True) == blob
    assert B.closed_map_save() == A.closed_map_save()
    for k in range(len(poses)):
        a, b = A.place_read_keyframe_clouds(k), B.place_read_keyframe_clouds(k)
        assert cat(c for side in a for c in side) == cat(c for side in b for c in side) == cat(d["clouds"][k])
    assert B.loop_info()["arena_points"] == A.loop_info()["arena_points"] == sum(len(c) for kf in d["clouds"] for c in kf) > 0
    # a rebuild, a carve and a surfel pass in the loaded context give the saver's bytes
    assert less(B.closed_map_build(2, poses)) == less(A.closed_map_info())
    with not_ready(hip_module):
        B.closed_map_misses()
    assert B.closed_map_carve() == A.closed_map_carve_info() and B.closed_map_surfels() == A.closed_map_surfel_info()
    assert map_bytes(B, hip_module) == want and B.closed_map_save(clouds=True) == blob
    B.close()


def test_without_clouds_the_loaded_map_is_detached(hip_module, corner):
    A, poses, scan, prior = corner
    B = loaded(hip_module, A.closed_map_save())
    want = map_bytes(A, hip_module)
    for call in (lambda: B.closed_map_build(2, poses), lambda: B.closed_map_build(0), B.closed_map_carve, B.closed_map_surfels):
        with not_ready(hip_module):
            call()
        assert map_bytes(B, hip_module) == want
    assert bits(B.closed_map_localise(scan, prior)[0]) == bits(A.closed_map_localise(scan, prior)[0])
    # a surfel configure drops the surfels and leaves the rows and the carve; the surfels cannot be gathered again
    B.closed_map_surfel_configure(min_points=5)
    got = map_bytes(B, hip_module)
    assert got["moments"] is None and got["surfels"] is None
    for k in ("read", "box", "poses", "info", "keyframes", "misses", "carved", "carve_info"):
        assert got[k] == want[k], k
    with not_ready(hip_module):
        B.closed_map_surfels()
    d = SN.unpack(B.closed_map_save())
    assert d["sums"] is None and d["M"] is not None
    # emptying the map ends the detached state: the closed map's own configure, then a build over the (cloudless) keyframes
    B.closed_map_configure(voxel=LS.CORNER["voxel"], cloud_mask=CS.MASK)
    with not_ready(hip_module):
        B.closed_map_read()
    info = B.closed_map_build(0)
    assert (info["n_keyframes"], info["empty_keyframes"], info["n_voxels"]) == (len(poses), len(poses), 0)
    B.close()


# ---- 4: the adversarial map ------------------------------------------------------------------------------------------------
def test_the_adversarial_map_round_trips(hip_module):
    voxel, origin = 0.3, (-0.37, 12.5, 0.11)
    poses, clouds = TS.adversarial_plus(voxel, origin)
    A, V = TS.built(hip_module, poses, clouds, 0x21, voxel, origin)
    A.closed_map_carve()
    A.closed_map_surfels()
    blob = A.closed_map_save()
    d = check_unpacked(A, blob)
    assert (SN.cell_of(d["key"]) < 0).any() and (d["Q"] == d["N"][:, None] << 24).any()   # negative cells, q = 2^24
    B = loaded(hip_module, blob)
    assert map_bytes(B, hip_module) == map_bytes(A, hip_module) and B.closed_map_save() == blob
    A.close(); B.close()


# ---- 5: exact sizes through the numpy packer ---------------------------------------------------------------------------------
def with_rows(base, nv, seed=11):
    """the corner's dict with nv seeded rows in place of its own, misses and sums to match"""
    small = SN.small_map(nv=nv, seed=seed)
    d = dict(base)
    for k in ("key", "N", "Q", "M", "sums"):
        d[k] = small[k]
    d["info"] = dict(base["info"], n_voxels=nv, n_points=int(small["N"].sum()))
    d["surfel_info"] = dict(base["surfel_info"], solved_voxels=int((small["N"] >= base["surfel"]["min_points"]).sum()))
    return d


@pytest.mark.parametrize("nv", [0, 1, 255, 256, 257, 1025])
def test_exact_sizes_through_the_numpy_packer(hip_module, corner, nv):
    base = SN.unpack(corner[0].closed_map_save())
    d = with_rows(base, nv)
    blob = SN.pack(d)
    B = hip_module.HipRegistration()
    assert B.closed_map_load(blob)["n_voxels"] == nv
    cen, cnt = B.closed_map_read()
    want = SN.centroid(d["key"], d["N"], d["Q"], d["cmap"]["voxel"], d["cmap"]["origin"])
    assert cnt.tobytes() == d["N"].tobytes() and bits(cen) == bits(want)
    bcen, bcnt = B.closed_map_read_box(WORLD["lo"], WORLD["hi"], 1)   # every voxel: every key is findable in the rebuilt table
    assert bits(bcen) == bits(want) and bcnt.tobytes() == d["N"].tobytes()
    assert B.closed_map_misses().tobytes() == d["M"].tobytes() and B.closed_map_moments().tobytes() == d["sums"].tobytes()
    assert B.closed_map_surfel_info()["solved_voxels"] == d["surfel_info"]["solved_voxels"]
    assert B.closed_map_save() == blob
    B.close()


def test_the_golden_blob_loads(hip_module):
    blob = open(os.path.join(HERE, "golden", "closed_map_snapshot_v1.bin"), "rb").read()
    B = hip_module.HipRegistration()
    assert B.closed_map_load(blob)["n_points"] == 1010
    check_unpacked(B, blob)
    n, e, c = B.closed_map_read_surfels()
    assert c.tolist() == [1, 2, 3, 4, 1000] and not n[:2].any() and np.allclose(np.linalg.norm(n[2:], axis=1), 1.0)
    assert B.closed_map_save() == blob
    B.close()


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------
def _rows(f):
    def corrupt(d):
        for k in ("key", "N", "Q", "M", "sums"):
            d[k] = d[k].copy()
        f(d)
    return corrupt


def _dup(a, b):
    return _rows(lambda d: d["key"].__setitem__(a, d["key"][b]))


def _sum_n(d):
    d["info"] = dict(d["info"], n_points=d["info"]["n_points"] + 1)


def _nan(d):
    d["descriptors"] = d["descriptors"].copy()
    d["descriptors"][-1, 3, 7] = np.nan


def _not_rigid(d):
    d["poses"] = d["poses"].copy()
    d["poses"][1, :3, :3] *= 1.001


def _more_poses(d):
    d["poses"] = np.concatenate([d["poses"], d["poses"][:1]])
    d["info"] = dict(d["info"], n_keyframes=len(d["poses"]), added_keyframes=d["info"]["added_keyframes"] + 1)


def _cloud_count(d):
    counts = np.array([[len(c) for c in kf] for kf in d["clouds"]], np.int64)
    counts[-1, 4] += 1
    d["cloud_counts"] = counts


# name -> (the corruption of the dict, the section the refusal names, whether the base carries the clouds)
SEALED = {
    "duplicate_key_first_last": (_dup(-1, 0), "rows", False),
    "duplicate_key_neighbours": (_dup(8, 7), "rows", False),
    "axis_field_0": (_rows(lambda d: d["key"].__setitem__(5, d["key"][5] & ~np.uint64(0x1fffff << 21))), "rows", False),
    "bit_63": (_rows(lambda d: d["key"].__setitem__(5, d["key"][5] | np.uint64(1 << 63))), "rows", False),
    "N_0": (_rows(lambda d: d["N"].__setitem__(3, 0)), "rows", False),
    "Q_above": (_rows(lambda d: d["Q"].__setitem__((4, 1), (int(d["N"][4]) << 24) + 1)), "rows", False),
    "Q_negative": (_rows(lambda d: d["Q"].__setitem__((4, 2), -1)), "rows", False),
    "M_negative": (_rows(lambda d: d["M"].__setitem__(-1, -1)), "misses", False),
    "Ns_negative": (_rows(lambda d: d["sums"].__setitem__((6, 0), -1)), "sums", False),
    "nan_in_a_descriptor": (_nan, "database", False),
    "non_rigid_build_pose": (_not_rigid, "poses", False),
    "K_above_n_kf": (_more_poses, "header", False),
    "cloud_count_one_more": (_cloud_count, "clouds", True),
    "sum_N_not_n_points": (_sum_n, "rows", False),
}
UNSEALED = ["header"] + list(SN.KINDS) + ["truncated_rows"]


@pytest.fixture(scope="module")
def refusal(hip_module, corner):
    """the target: a context that holds the corner's map, what it saves and localises to, and the two bases of the corruptions"""
    A, poses, scan, prior = corner
    T = loaded(hip_module, A.closed_map_save(clouds=True))
    blobs = {False: A.closed_map_save(), True: A.closed_map_save(clouds=True)}
    T.closed_map_localise(scan, prior)   # (the first call after a load prepares the voxel records and says so in its info)
    pose, info = T.closed_map_localise(scan, prior)
    assert info["prepared"] == 0
    before = (T.closed_map_save(clouds=True), bits(pose) + repr(info).encode() + log_bytes(T.closed_map_localise_log()))
    yield T, blobs, before, scan, prior
    T.close()


def refused(reg, T, blob, section, before, scan, prior):
    with pytest.raises(reg.TloamHipError, match=f"TLOAM_E_INVALID closed map snapshot: {section}: ") as e:
        T.closed_map_load(blob)
    print(e.value)
    assert T.closed_map_save(clouds=True) == before[0]
    pose, info = T.closed_map_localise(scan, prior)
    assert bits(pose) + repr(info).encode() + log_bytes(T.closed_map_localise_log()) == before[1]


@pytest.mark.parametrize("name", list(SEALED))
def test_a_corrupt_blob_with_good_checksums_is_refused(hip_module, refusal, name):
    T, blobs, before, scan, prior = refusal
    corrupt, section, clouds = SEALED[name]
    d = SN.unpack(blobs[clouds])
    assert len(d["key"]) > 8 and len(d["poses"]) == 2
    corrupt(d)
    blob = SN.pack(d)
    assert blob != blobs[clouds] and len(blob) >= len(blobs[clouds])
    refused(hip_module, T, blob, section, before, scan, prior)


@pytest.mark.parametrize("name", UNSEALED)
def test_a_damaged_blob_is_refused(hip_module, refusal, name):
    T, blobs, before, scan, prior = refusal
    good = blobs[True]
    where = dict([("header", (0, SN.HEADER_BYTES))] + [(k, (off, n)) for k, off, n in SN.sections_of(good)])
    if name == "truncated_rows":
        off, n = where["rows"]
        blob, section = good[:off + (n // 16) * 8], "rows"
    else:
        off, n = where[name]
        assert n > 0
        b = bytearray(good)
        b[off + n // 2] ^= 0x10
        blob, section = bytes(b), name
    refused(hip_module, T, blob, section, before, scan, prior)


def test_the_undamaged_blobs_still_load(hip_module, refusal):
    """the refusals above are the corruptions', not the packer's: the same bases, repacked untouched, load"""
    T, blobs, before, scan, prior = refusal
    for clouds in (False, True):
        assert SN.pack(SN.unpack(blobs[clouds])) == blobs[clouds]
    B = hip_module.HipRegistration()
    B.closed_map_load(SN.pack(SN.unpack(blobs[False])))
    B.closed_map_load(SN.pack(SN.unpack(blobs[True])))
    assert B.closed_map_save(clouds=True) == blobs[True]
    B.close()


# ---- 7: lifecycle ------------------------------------------------------------------------------------------------------------
def test_a_load_replaces_what_the_context_held(hip_module, static, tmp_path):
    A, _, blob, poses, queries = static
    H, cposes, clouds, scan, truth = corner_context(hip_module)
    assert H.place_info()["n_keyframes"] == 2
    path = str(tmp_path / "street.tlcm")
    assert map_io.save_closed_map(path, A) == len(blob) and open(path, "rb").read() == blob
    assert sorted(os.listdir(tmp_path)) == ["street.tlcm"]
    info = map_io.load_closed_map(path, H)
    assert info["n_keyframes_database"] == CS.STATIC_KEYFRAMES and H.closed_map_save() == blob
    assert map_bytes(H, hip_module) == map_bytes(A, hip_module)
    assert H.loop_info()["n_constraints"] == 0
    with not_ready(hip_module):
        H.graph_poses()
    # a scan added after the load is keyframe n_kf; the relocalisation still ranks the build's keyframes only
    q = queries["quarter"][0]
    H.closed_map_relocalise(q)   # (the first call after a load prepares the voxel records and says so in its info)
    pose, rinfo = H.closed_map_relocalise(q)
    hyps = H.closed_map_relocalise_hypotheses()
    assert H.place_add_scan(q, np.eye(4), 99) == CS.STATIC_KEYFRAMES
    assert H.place_info()["n_keyframes"] == CS.STATIC_KEYFRAMES + 1
    pose2, rinfo2 = H.closed_map_relocalise(q)
    assert bits(pose2) == bits(pose) and rinfo2 == rinfo
    assert [h["keyframe"] for h in H.closed_map_relocalise_hypotheses()] == [h["keyframe"] for h in hyps]
    assert max(h["keyframe"] for h in hyps) < CS.STATIC_KEYFRAMES
    assert SN.unpack(H.closed_map_save())["frames"].tolist() == list(range(CS.STATIC_KEYFRAMES)) + [99]
    # what empties the map empties a loaded one
    H.odometry_reset(None, TS.TC.odom_cfg(hip_module))
    assert H.place_info()["n_keyframes"] == 0 and H.closed_map_info()["n_voxels"] == 0
    with not_ready(hip_module):
        H.closed_map_save()
    H.closed_map_load(blob)
    H.place_configure(enabled=1, **RS.PLACE)
    assert H.place_info()["n_keyframes"] == 0
    with not_ready(hip_module):
        H.closed_map_read()
    H.closed_map_load(blob)
    H.loop_configure(enabled=1)
    with not_ready(hip_module):
        H.closed_map_read()
    H.close()


def test_save_refuses_what_it_must(hip_module, corner):
    A = corner[0]
    C = hip_module.C
    n = C.c_size_t(0)
    assert A.L.tloam_closed_map_save_size(A.h, 2, C.byref(n)) == -1
    blob = A.closed_map_save()
    buf = C.create_string_buffer(b"\x5a" * len(blob), len(blob))
    assert A.L.tloam_closed_map_save(A.h, 0, buf, len(blob) - 8, C.byref(n)) == -1
    assert n.value == len(blob) and buf.raw == b"\x5a" * len(blob)
    H = hip_module.HipRegistration()
    with not_ready(hip_module):
        H.closed_map_save()
    H.close()
