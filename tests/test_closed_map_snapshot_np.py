"""The closed map's snapshot format without a GPU: the numpy restatement (tests/closed_map_snapshot_np.py)
against itself, its checksum's properties, the library's host-only tloam_closed_map_probe on numpy-packed blobs, and the golden
blob that pins format version 1."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import closed_map_snapshot_np as SN  # noqa: E402
from tloam_amd import registration as reg  # noqa: E402

GOLDEN_PATH = os.path.join(HERE, "golden", "closed_map_snapshot_v1.bin")
SHAPES = [dict(nv=nv, carve=c, surfels=s, clouds=cl) for nv in (0, 1, 257) for c, s, cl in
          ((True, True, True), (False, True, False), (True, False, False), (False, False, True), (False, False, False))]


def refused():
    return pytest.raises(reg.TloamHipError, match="TLOAM_E_INVALID")


def golden_dict():
    """one keyframe, two rings by four sectors, five voxels with misses and surfel sums: every value a literal"""
    d = SN.configs(n_rings=2, n_sectors=4, voxel=0.5, origin=(0.25, -1.0, 2.0), cloud_mask=0x10, min_points=3)
    pose = np.array([[0.0, -1.0, 0.0, 1.5], [1.0, 0.0, 0.0, -2.25], [0.0, 0.0, 1.0, 0.125], [0.0, 0.0, 0.0, 1.0]])
    cells = [[0, 0, 0], [-1, 2, 0], [3, -4, 1], [1 - SN.LIMIT, SN.LIMIT - 1, 0], [7, 7, -7]]
    N = np.array([1, 2, 3, 4, 1000], np.int64)
    Q = np.array([[8388608, 8388608, 8388608], [0, 33554432, 1], [25165824, 12582912, 50331647], [4, 3, 2],
                  [8388608000, 16777216000, 0]], np.int64)
    R = Q >> 8
    sums = np.zeros((5, 13), np.int64)
    sums[:, 0] = N
    sums[:, 1:4] = R
    sums[:, 4:10] = [[1073741824, 1073741824, 1073741824, 1073741824, 1073741824, 1073741824],
                     [0, 0, 0, 8589934592, 0, 1], [3221225472, 1, 2, 805306368, 3, 12884901888], [4, 3, 2, 3, 2, 1],
                     [1073741824000, 5, -6, 4294967296000, 7, 0]]
    sums[:, 10:13] = [[256, -256, 0], [1, 2, 3], [-700, 0, 700], [0, 0, -1], [123456, -654321, 42]]
    d.update(flags=0, frames=np.array([42], np.int64), kf_poses=pose[None], poses=pose[None],
             ring_keys=np.array([[0.5, 1.25]]), sector_keys=np.array([[0.0, 2.5, 0.75, 1.0]]),
             descriptors=np.array([[[0.0, 1.5, 2.5, 0.0], [3.25, 0.0, 0.0, 4.0]]]), key=SN.key_of(cells), N=N, Q=Q,
             M=np.array([0, 1, 0, 7, 250], np.int64), sums=sums, clouds=None)
    d["info"] = dict(n_keyframes=1, added_keyframes=1, empty_keyframes=0, overflow_keyframes=0, n_voxels=5, n_points=1010,
                     capacity_voxels=0, pose_source=2, launches=4)
    d["carve_info"] = dict(n_keyframes=1, n_rays=1010, skipped_rays=2, steps=9000, tested=300, misses=258, voxels_missed=3,
                           launches=3, reserved0=0)
    d["surfel_info"] = dict(n_keyframes=1, n_points=1010, orphan_points=0, solved_voxels=3, launches=4, reserved0=0)
    return d


# ---- the restatement against itself --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(f"{k}{int(v)}" for k, v in s.items()))
def test_unpack_of_pack_is_the_dict(shape):
    d = SN.small_map(n_kf=3, n_rings=3, n_sectors=5, **shape)
    blob = SN.pack(d)
    u = SN.unpack(blob)
    d.pop("cloud_counts", None)
    assert SN.same({k: d[k] for k in u}, u)
    assert SN.pack(u) == blob and len(blob) % 8 == 0
    for _, off, n in SN.sections_of(blob):
        assert off % 8 == 0 and n % 8 == 0


def test_checksum_sees_every_bit_and_no_order():
    rng = np.random.default_rng(5)
    w = rng.integers(0, 2 ** 63, 512, dtype=np.int64).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, 512).astype(np.uint64)
    base = SN.checksum(w)
    assert SN.checksum(w.tobytes()) == base and SN.checksum(b"") == 0
    t = SN.terms(w)
    with np.errstate(over="ignore"):
        total = np.add.reduce(t, dtype=np.uint64)
        # any order of the sum: reversed, shuffled, by per-wave partials of 64
        assert int(np.add.reduce(t[::-1], dtype=np.uint64)) == base
        assert int(np.add.reduce(t[rng.permutation(512)], dtype=np.uint64)) == base
        assert int(np.add.reduce(np.add.reduce(t.reshape(8, 64), axis=1, dtype=np.uint64)[::-1], dtype=np.uint64)) == base
        # every single-bit flip of the 4 KiB section changes it: the flipped word's term changes, so the sum does
        idx = np.arange(512, dtype=np.uint64) + np.uint64(1)
        for bit in range(64):
            flipped = SN.mix64((w ^ (np.uint64(1) << np.uint64(bit))) + SN.GOLDEN * idx)
            sums = total - t + flipped   # the checksum of each of the 512 blobs with that bit of one word flipped
            assert not (sums == total).any(), bit
    # the position counts: two words swapped, and a word moved to the end, change it
    s = w.copy(); s[[3, 4]] = s[[4, 3]]
    assert SN.checksum(s) != base and SN.checksum(np.roll(w, 1)) != base
    # and against a plain-integer restatement of the definition
    M = (1 << 64) - 1

    def mix(x):
        x ^= x >> 30; x = (x * 0xbf58476d1ce4e5b9) & M
        x ^= x >> 27; x = (x * 0x94d049bb133111eb) & M
        return x ^ (x >> 31)
    assert sum(mix((int(v) + 0x9E3779B97F4A7C15 * (i + 1)) & M) for i, v in enumerate(w[:40])) & M == SN.checksum(w[:40])


# ---- the library's probe on numpy-packed blobs -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(f"{k}{int(v)}" for k, v in s.items()))
def test_probe_reports_the_packed_counts_and_refuses_truncation(shape):
    d = SN.small_map(n_kf=2, n_rings=3, n_sectors=5, **shape)
    blob = SN.pack(d)
    info = reg.closed_map_probe(blob)
    cp = sum(len(c) for kf in d["clouds"] for c in kf) if shape["clouds"] else 0
    assert info == dict(format_version=1, flags=int(shape["clouds"]), n_keyframes_database=2, n_keyframes_map=2,
                        n_voxels=shape["nv"], n_points=int(d["N"].sum()), has_carve=int(shape["carve"]),
                        has_surfels=int(shape["surfels"]), has_clouds=int(shape["clouds"]), n_rings=3, n_sectors=5, cloud_points=cp,
                        voxel=0.5, origin=(0.25, -1.0, 2.0), bytes=len(blob))
    cuts = {0, 8, SN.HEADER_BYTES - 1, SN.HEADER_BYTES, len(blob) - 1, len(blob) + 8}
    for _, off, n in SN.sections_of(blob):
        cuts |= {off, off - 1, off + n, off + n - 1}
    for cut in sorted(c for c in cuts if 0 <= c != len(blob)):
        with refused():
            reg.closed_map_probe((blob + b"\0" * 8)[:cut])


def test_probe_refuses_a_bad_header_and_a_bad_table():
    blob = SN.pack(SN.small_map(nv=257, n_kf=2, clouds=True))
    h = SN.header_of(blob)
    body = blob[SN.HEADER_BYTES:]
    assert reg.closed_map_probe(SN.reseal_header(h) + body)["n_voxels"] == 257

    def edited(**fields):
        g = h.copy()
        for k, v in fields.items():
            g[k] = v
        return SN.reseal_header(g) + body

    def table(k, **fields):
        g = h.copy()
        for name, v in fields.items():
            g["sec"][k][name] = v
        return SN.reseal_header(g) + body

    bad = dict(magic=edited(magic=b"TLCMSNP2"), version=edited(version=2), flags=edited(flags=3), bytes=edited(bytes=len(blob) + 8),
               clouds_flag=edited(has_clouds=0), K=edited(K=3), voxels=edited(n_voxels=(1 << 30) + 1), rings=edited(n_rings=0),
               voxel=edited(voxel=float("nan")), sections=edited(n_sections=8),
               past_the_end=table(8, offset=len(blob), bytes=int(h["sec"][8]["bytes"])),
               overlapping=table(6, offset=int(h["sec"][5]["offset"]) + 8),
               unaligned=table(5, offset=int(h["sec"][5]["offset"]) + 4), kind=table(2, kind=4),
               size=table(5, bytes=int(h["sec"][5]["bytes"]) - 8))
    for name, b in bad.items():
        with refused():
            reg.closed_map_probe(b)
    # a flipped bit anywhere in the header, its checksum left alone
    for byte in range(0, SN.HEADER_BYTES, 7):
        b = bytearray(blob)
        b[byte] ^= 1 << (byte % 8)
        with refused():
            reg.closed_map_probe(bytes(b))


# ---- format version 1, pinned ------------------------------------------------------------------------------------------------
def test_the_golden_blob_is_reproduced_byte_for_byte():
    d = golden_dict()
    blob = SN.pack(d)
    want = open(GOLDEN_PATH, "rb").read()
    assert len(want) < 16384 and blob == want
    assert SN.same({k: d[k] for k in SN.unpack(want)}, SN.unpack(want))
    info = reg.closed_map_probe(want)
    assert (info["n_voxels"], info["n_points"], info["n_keyframes_database"], info["n_rings"], info["n_sectors"]) == (5, 1010, 1, 2, 4)
    assert (info["has_carve"], info["has_surfels"], info["has_clouds"], info["bytes"]) == (1, 1, 0, len(want))
