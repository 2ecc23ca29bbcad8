"""The closed map's snapshot, format version 1, restated in numpy: the checksum, the header, the section
table and the nine sections, as `pack(dict) -> bytes` and `unpack(bytes) -> dict`.  It shares nothing with the C code: the
layouts are written out here as numpy dtypes, from the format table.

The dict:
  flags                      TLOAM_SNAPSHOT_* (bit 0: clouds)
  place, loop, cmap, carve, surfel   the five configurations, {field: value} (loop["coarse"] is the TLS configuration's dict)
  info, carve_info, surfel_info      the three infos, {field: int}; carve_info / surfel_info None when that section is absent
  frames (n_kf,) int64, kf_poses (n_kf, 4, 4)                              the host's keyframe table
  ring_keys (n_kf, R), sector_keys (n_kf, S), descriptors (n_kf, R, S)     the device's database
  poses (K, 4, 4)            the build's poses
  key (nv,) uint64, N (nv,) int64, Q (nv, 3) int64                         the rows in id order
  M (nv,) int64 or None, sums (nv, 13) int64 or None
  clouds                     None, or per keyframe a list of eight (n, 3) arrays in slot order
  cloud_counts               optional, (n_kf, 8): written instead of the clouds' own lengths (for the refusal tests)
"""
from __future__ import annotations

import numpy as np

MAGIC = b"TLCMSNP1"
VERSION = 1
CLOUDS = 1
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
HEADER_BYTES = 416
KINDS = ("configs", "infos", "keyframes", "poses", "database", "rows", "misses", "sums", "clouds")   # kinds 1 .. 9
QSCALE = 16777216.0   # 2^24
LIMIT = 1 << 20

TLS = np.dtype([("k_corr", "<i4"), ("factor_num", "<i4"), ("edge_dist_thres", "<f8"), ("edge_dir_thres", "<f8"),
                ("edge_maxnum", "<i4"), ("sphere_maxnum", "<i4"), ("sphere_dist_thres", "<f8"), ("planar_dist_thres", "<f8"),
                ("planar_maxnum", "<i4"), ("ground_maxnum", "<i4"), ("ground_dist_thres", "<f8"), ("max_iterations", "<i4"),
                ("reserved0", "<i4"), ("cost_threshold", "<f8"), ("gnc_factor", "<f8"), ("noise_bound", "<f8"),
                ("fitness_thres", "<f8")])
PLACE = np.dtype([("enabled", "<i4"), ("n_rings", "<i4"), ("n_sectors", "<i4"), ("num_candidates", "<i4"),
                  ("exclude_recent", "<i4"), ("reserved0", "<i4"), ("max_radius", "<f8"), ("height_offset", "<f8"),
                  ("kf_dist", "<f8"), ("kf_angle", "<f8"), ("dist_thres", "<f8"), ("reserve_keyframes", "<i8")])
LOOP = np.dtype([("enabled", "<i4"), ("window", "<i4"), ("init_mode", "<i4"), ("reserved0", "<i4"), ("inlier_dist", "<f8"),
                 ("min_overlap", "<f8"), ("max_rmse", "<f8"), ("reserve_points", "<i8"), ("coarse", TLS)])
CMAP = np.dtype([("voxel", "<f8"), ("origin", "<f8", (3,)), ("cloud_mask", "<i4"), ("reserved0", "<i4"), ("reserve_voxels", "<i8")])
CARVE = np.dtype([("max_range", "<f8"), ("end_margin", "<f8"), ("radius", "<f8"), ("ray_mask", "<i4"), ("reserved0", "<i4")])
SURFEL = np.dtype([("min_points", "<i4"), ("reserved0", "<i4")])
INFO = np.dtype([("n_keyframes", "<i8"), ("added_keyframes", "<i8"), ("empty_keyframes", "<i8"), ("overflow_keyframes", "<i8"),
                 ("n_voxels", "<i8"), ("n_points", "<i8"), ("capacity_voxels", "<i8"), ("pose_source", "<i4"), ("launches", "<i4")])
CARVE_INFO = np.dtype([("n_keyframes", "<i8"), ("n_rays", "<i8"), ("skipped_rays", "<i8"), ("steps", "<i8"), ("tested", "<i8"),
                       ("misses", "<i8"), ("voxels_missed", "<i8"), ("launches", "<i4"), ("reserved0", "<i4")])
SURFEL_INFO = np.dtype([("n_keyframes", "<i8"), ("n_points", "<i8"), ("orphan_points", "<i8"), ("solved_voxels", "<i8"),
                        ("launches", "<i4"), ("reserved0", "<i4")])
ENTRY = np.dtype([("kind", "<u4"), ("reserved0", "<u4"), ("offset", "<u8"), ("bytes", "<u8"), ("checksum", "<u8")])
HEADER = np.dtype([("magic", "S8"), ("version", "<u4"), ("flags", "<u4"), ("bytes", "<u8"), ("checksum", "<u8"),
                   ("n_kf", "<i8"), ("K", "<i8"), ("n_voxels", "<i8"), ("n_points", "<i8"), ("cloud_points", "<i8"),
                   ("n_rings", "<i4"), ("n_sectors", "<i4"), ("has_carve", "<i4"), ("has_surfels", "<i4"), ("has_clouds", "<i4"),
                   ("n_sections", "<i4"), ("voxel", "<f8"), ("origin", "<f8", (3,)), ("sec", ENTRY, (9,))])
assert HEADER.itemsize == HEADER_BYTES and TLS.itemsize == 104
assert (PLACE.itemsize, LOOP.itemsize, CMAP.itemsize, CARVE.itemsize, SURFEL.itemsize) == (72, 152, 48, 32, 8)
assert (INFO.itemsize, CARVE_INFO.itemsize, SURFEL_INFO.itemsize) == (64, 64, 40)


# ---- the checksum --------------------------------------------------------------------------------------------------------------
def mix64(x):
    """the splitmix64 finaliser on uint64 arrays (arithmetic mod 2^64)"""
    x = np.asarray(x, np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30); x *= np.uint64(0xbf58476d1ce4e5b9)
        x ^= x >> np.uint64(27); x *= np.uint64(0x94d049bb133111eb)
        x ^= x >> np.uint64(31)
    return x


def terms(words):
    """the checksum's summands: mix64(w_i + GOLDEN * (i + 1))"""
    w = np.asarray(words, np.uint64)
    with np.errstate(over="ignore"):
        return mix64(w + GOLDEN * (np.arange(len(w), dtype=np.uint64) + np.uint64(1)))


def checksum(data) -> int:
    """of a section given as bytes (a multiple of 8) or as an array of 64-bit words"""
    w = np.frombuffer(data, "<u8") if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data, np.uint64)
    with np.errstate(over="ignore"):
        return int(np.add.reduce(terms(w), dtype=np.uint64)) if len(w) else 0


# ---- the voxel map's arithmetic the tests need --------------------------------------------------------------
def key_of(i):
    """i + 2^20 of each axis in 21 bits -> uint64"""
    u = (np.asarray(i, np.int64).reshape(-1, 3) + LIMIT).astype(np.uint64)
    return u[:, 0] | (u[:, 1] << np.uint64(21)) | (u[:, 2] << np.uint64(42))


def cell_of(key):
    k = np.asarray(key, np.uint64)
    return np.stack([((k >> np.uint64(21 * a)) & np.uint64(0x1fffff)).astype(np.int64) - LIMIT for a in range(3)], axis=1)


def centroid(key, N, Q, voxel, origin):
    """c = o + v * ((double) i + ((double) Q / (double) N) * 2^-24), in that order"""
    i = cell_of(key).astype(np.float64)
    q = np.asarray(Q, np.int64).astype(np.float64) / np.asarray(N, np.int64).astype(np.float64)[:, None]
    return np.asarray(origin, np.float64) + float(voxel) * (i + q * (1.0 / QSCALE))


# ---- pack / unpack -------------------------------------------------------------------------------------------------------------
def _record(dtype, values):
    r = np.zeros((), dtype)
    for name in dtype.names:
        if dtype[name].names:
            r[name] = _record(dtype[name], values[name])
        elif name in values:
            r[name] = values[name]
    return r


def _plain(r):
    out = {}
    for name in r.dtype.names:
        v = r[name]
        out[name] = _plain(v) if v.dtype.names else (tuple(v.tolist()) if v.shape else v.item())
    return out


def _colmajor(T):
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    return np.ascontiguousarray(T.transpose(0, 2, 1)).astype("<f8").tobytes()


def _matrices(raw, n):
    return np.frombuffer(raw, "<f8").reshape(n, 4, 4).transpose(0, 2, 1).copy()


def section_bytes(d):
    """the nine sections of the dict as bytes, and the header's counts"""
    frames = np.asarray(d["frames"], "<i8").reshape(-1)
    nk, K = len(frames), len(np.asarray(d["poses"], np.float64).reshape(-1, 4, 4))
    rk = np.asarray(d["ring_keys"], "<f8").reshape(nk, -1)
    sk = np.asarray(d["sector_keys"], "<f8").reshape(nk, -1)
    R, S = int(d["place"]["n_rings"]), int(d["place"]["n_sectors"])
    key, N, Q = np.asarray(d["key"], "<u8"), np.asarray(d["N"], "<i8"), np.asarray(d["Q"], "<i8").reshape(-1, 3)
    nv = len(key)
    sec = [b""] * 9
    sec[0] = b"".join(_record(t, d[k]).tobytes() for t, k in ((PLACE, "place"), (LOOP, "loop"), (CMAP, "cmap"), (CARVE, "carve"),
                                                              (SURFEL, "surfel")))
    sec[1] = _record(INFO, d["info"]).tobytes()
    if d.get("carve_info") is not None:
        sec[1] += _record(CARVE_INFO, d["carve_info"]).tobytes()
    if d.get("surfel_info") is not None:
        sec[1] += _record(SURFEL_INFO, d["surfel_info"]).tobytes()
    sec[2] = frames.tobytes() + _colmajor(d["kf_poses"])
    sec[3] = _colmajor(d["poses"])
    sec[4] = rk.tobytes() + sk.tobytes() + np.asarray(d["descriptors"], "<f8").reshape(nk, -1).tobytes()
    sec[5] = key.tobytes() + N.tobytes() + b"".join(np.ascontiguousarray(Q[:, a]).tobytes() for a in range(3))
    if d.get("M") is not None:
        sec[6] = np.asarray(d["M"], "<i8").tobytes()
    if d.get("sums") is not None:
        sec[7] = np.asarray(d["sums"], "<i8").reshape(nv, 13).tobytes()
    cloud_points = 0
    if d.get("clouds") is not None:
        clouds = [[np.asarray(c, "<f8").reshape(-1, 3) for c in kf] for kf in d["clouds"]]
        counts = np.array([[len(c) for c in kf] for kf in clouds], "<i8").reshape(nk, 8)
        cloud_points = int(counts.sum())
        if d.get("cloud_counts") is not None:
            counts = np.asarray(d["cloud_counts"], "<i8").reshape(nk, 8)
        sec[8] = counts.tobytes() + b"".join(c.tobytes() for kf in clouds for c in kf)
    counts = dict(n_kf=nk, K=K, n_voxels=nv, n_points=int(d["info"]["n_points"]), cloud_points=cloud_points, n_rings=R,
                  n_sectors=S, has_carve=int(d.get("M") is not None), has_surfels=int(d.get("sums") is not None),
                  has_clouds=int(d.get("clouds") is not None), voxel=d["cmap"]["voxel"], origin=d["cmap"]["origin"])
    return sec, counts


def seal(header, sections) -> bytes:
    """the blob of a header record and nine sections: offsets, sizes and every checksum filled in"""
    h = header.copy()
    at = HEADER_BYTES
    for k, s in enumerate(sections):
        h["sec"][k] = (k + 1, 0, at, len(s), checksum(s))
        at += len(s)
    h["bytes"] = at
    h["n_sections"] = 9
    h["checksum"] = 0
    h["checksum"] = checksum(h.tobytes())
    return h.tobytes() + b"".join(sections)


def pack(d) -> bytes:
    sec, counts = section_bytes(d)
    h = np.zeros((), HEADER)
    h["magic"], h["version"], h["flags"] = MAGIC, VERSION, int(d.get("flags", CLOUDS if d.get("clouds") is not None else 0))
    for k, v in counts.items():
        h[k] = v
    return seal(h, sec)


def header_of(blob):
    return np.frombuffer(blob[:HEADER_BYTES], HEADER)[0].copy()


def reseal_header(h) -> bytes:
    """a header record's bytes with its own checksum recomputed (the table as it stands)"""
    h = h.copy()
    h["checksum"] = 0
    h["checksum"] = checksum(h.tobytes())
    return h.tobytes()


def sections_of(blob):
    """[(name, offset, bytes)] of the table"""
    h = header_of(blob)
    return [(KINDS[k], int(h["sec"][k]["offset"]), int(h["sec"][k]["bytes"])) for k in range(9)]


def unpack(blob) -> dict:
    """the dict of a well-formed blob; every checksum is verified (ValueError otherwise)"""
    blob = bytes(blob)
    h = header_of(blob)
    if bytes(h["magic"]) != MAGIC or int(h["version"]) != VERSION or int(h["bytes"]) != len(blob):
        raise ValueError("header")
    z = h.copy()
    z["checksum"] = 0
    if checksum(z.tobytes()) != int(h["checksum"]):
        raise ValueError("header checksum")
    raw = []
    for k in range(9):
        e = h["sec"][k]
        s = blob[int(e["offset"]):int(e["offset"]) + int(e["bytes"])]
        if int(e["kind"]) != k + 1 or len(s) != int(e["bytes"]) or checksum(s) != int(e["checksum"]):
            raise ValueError(KINDS[k])
        raw.append(s)
    nk, K, nv, R, S = (int(h[k]) for k in ("n_kf", "K", "n_voxels", "n_rings", "n_sectors"))
    d = dict(flags=int(h["flags"]))
    at = 0
    for t, name in ((PLACE, "place"), (LOOP, "loop"), (CMAP, "cmap"), (CARVE, "carve"), (SURFEL, "surfel")):
        d[name] = _plain(np.frombuffer(raw[0][at:at + t.itemsize], t)[0])
        at += t.itemsize
    d["info"] = _plain(np.frombuffer(raw[1][:64], INFO)[0])
    at = 64
    d["carve_info"] = d["surfel_info"] = None
    if h["has_carve"]:
        d["carve_info"] = _plain(np.frombuffer(raw[1][at:at + 64], CARVE_INFO)[0])
        at += 64
    if h["has_surfels"]:
        d["surfel_info"] = _plain(np.frombuffer(raw[1][at:at + 40], SURFEL_INFO)[0])
    d["frames"] = np.frombuffer(raw[2][:8 * nk], "<i8").copy()
    d["kf_poses"] = _matrices(raw[2][8 * nk:], nk)
    d["poses"] = _matrices(raw[3], K)
    db = np.frombuffer(raw[4], "<f8")
    d["ring_keys"] = db[:nk * R].reshape(nk, R).copy()
    d["sector_keys"] = db[nk * R:nk * (R + S)].reshape(nk, S).copy()
    d["descriptors"] = db[nk * (R + S):].reshape(nk, R, S).copy()
    rows = np.frombuffer(raw[5], "<u8").reshape(5, nv)
    d["key"] = rows[0].copy()
    d["N"] = rows[1].astype(np.int64)
    d["Q"] = np.ascontiguousarray(rows[2:5].astype(np.int64).T)
    d["M"] = np.frombuffer(raw[6], "<i8").copy() if h["has_carve"] else None
    d["sums"] = np.frombuffer(raw[7], "<i8").reshape(nv, 13).copy() if h["has_surfels"] else None
    d["clouds"] = None
    if h["has_clouds"]:
        counts = np.frombuffer(raw[8][:64 * nk], "<i8").reshape(nk, 8)
        pts = np.frombuffer(raw[8][64 * nk:], "<f8").reshape(-1, 3)
        ends = np.concatenate([[0], np.cumsum(counts.reshape(-1))])
        d["clouds"] = [[pts[ends[8 * k + j]:ends[8 * k + j + 1]].copy() for j in range(8)] for k in range(nk)]
    return d


def same(a, b) -> bool:
    """two dicts of this module hold the same bytes"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    x, y = np.asarray(a), np.asarray(b)
    return x.shape == y.shape and x.dtype.kind == y.dtype.kind and x.tobytes() == y.astype(x.dtype).tobytes()


# ---- a small valid map from literals: what the CPU tests and the golden blob pack ---------------------------------------------
TLS_DEFAULT = dict(k_corr=10, factor_num=4, edge_dist_thres=2.0, edge_dir_thres=0.85, edge_maxnum=1200, sphere_maxnum=200,
                   sphere_dist_thres=1.0, planar_dist_thres=1.0, planar_maxnum=2500, ground_maxnum=2000, ground_dist_thres=1.0,
                   max_iterations=8, reserved0=0, cost_threshold=5e-9, gnc_factor=11.8, noise_bound=0.01, fitness_thres=0.02)


def configs(n_rings=20, n_sectors=60, voxel=1.0, origin=(0.0, 0.0, 0.0), cloud_mask=0xF0, min_points=5):
    return dict(
        place=dict(enabled=1, n_rings=n_rings, n_sectors=n_sectors, num_candidates=10, exclude_recent=50, reserved0=0,
                   max_radius=80.0, height_offset=2.0, kf_dist=1.0, kf_angle=0.2, dist_thres=0.30, reserve_keyframes=0),
        loop=dict(enabled=1, window=2, init_mode=0, reserved0=0, inlier_dist=0.3, min_overlap=0.6, max_rmse=0.2, reserve_points=0,
                  coarse=dict(TLS_DEFAULT)),
        cmap=dict(voxel=voxel, origin=tuple(origin), cloud_mask=cloud_mask, reserved0=0, reserve_voxels=0),
        carve=dict(max_range=60.0, end_margin=1.0, radius=0.25, ray_mask=0, reserved0=0),
        surfel=dict(min_points=min_points, reserved0=0))


def random_rows(nv, seed, voxel=1.0):
    """nv valid rows with distinct seeded keys, the extreme axis fields 1 and 2^21 - 1 among them -> key, N, Q"""
    rng = np.random.default_rng(seed)
    cells = set()
    if nv >= 1:
        cells.add((1 - LIMIT, LIMIT - 1, 0))
    if nv >= 2:
        cells.add((LIMIT - 1, 1 - LIMIT, 1 - LIMIT))
    while len(cells) < nv:
        cells.add(tuple(int(v) for v in rng.integers(-400, 400, 3)))
    i = np.array(sorted(cells), np.int64).reshape(-1, 3)
    i = i[rng.permutation(nv)] if nv else i
    N = rng.integers(1, 50, nv).astype(np.int64)
    Q = np.stack([rng.integers(0, N * (1 << 24) + 1) for _ in range(3)], axis=1).astype(np.int64) if nv else np.zeros((0, 3), np.int64)
    return key_of(i), N, Q


def small_map(nv=5, n_kf=1, n_rings=2, n_sectors=4, carve=True, surfels=True, clouds=False, seed=3):
    """a well-formed dict of nv voxels and n_kf keyframes, every value seeded"""
    rng = np.random.default_rng(seed)
    key, N, Q = random_rows(nv, seed)
    d = configs(n_rings, n_sectors, voxel=0.5, origin=(0.25, -1.0, 2.0), cloud_mask=0x10)
    poses = np.tile(np.eye(4), (n_kf, 1, 1))
    poses[:, :3, 3] = rng.uniform(-5.0, 5.0, (n_kf, 3))
    d.update(flags=CLOUDS if clouds else 0, frames=np.arange(n_kf, dtype=np.int64) * 3, kf_poses=poses.copy(), poses=poses,
             ring_keys=rng.uniform(0.0, 3.0, (n_kf, n_rings)), sector_keys=rng.uniform(0.0, 3.0, (n_kf, n_sectors)),
             descriptors=rng.uniform(0.0, 5.0, (n_kf, n_rings, n_sectors)), key=key, N=N, Q=Q)
    d["info"] = dict(n_keyframes=n_kf, added_keyframes=n_kf, empty_keyframes=0, overflow_keyframes=0, n_voxels=nv,
                     n_points=int(N.sum()), capacity_voxels=0, pose_source=2, launches=4)
    d["M"] = rng.integers(0, 9, nv).astype(np.int64) if carve else None
    d["carve_info"] = dict(n_keyframes=n_kf, n_rays=int(N.sum()), skipped_rays=0, steps=17, tested=9, misses=int(d["M"].sum()),
                           voxels_missed=int((d["M"] > 0).sum()), launches=3, reserved0=0) if carve else None
    if surfels:
        S = np.zeros((nv, 13), np.int64)
        S[:, 0] = N
        S[:, 1:4] = Q >> 8
        S[:, [4, 7, 9]] = (Q >> 8) ** 2 // np.maximum(N, 1)[:, None] + rng.integers(0, 1000, (nv, 3))
        S[:, 10:13] = rng.integers(-500, 500, (nv, 3))
        d["sums"] = S
        d["surfel_info"] = dict(n_keyframes=n_kf, n_points=int(N.sum()), orphan_points=0,
                                solved_voxels=int((N >= d["surfel"]["min_points"]).sum()), launches=4, reserved0=0)
    else:
        d["sums"], d["surfel_info"] = None, None
    d["clouds"] = [[rng.uniform(-3.0, 3.0, (int(rng.integers(0, 4)), 3)) for _ in range(8)] for _ in range(n_kf)] if clouds else None
    return d
