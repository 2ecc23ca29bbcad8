"""PCD export of the global map, of the merged voxel map (section 14), of the carved closed map
(section 21), of the closed map's surfels (section 22), of a diffed scan with its labels (section 26) and of the free cells of
the free-space grid (section 29); and the closed map's snapshot as a file (section 25): the one form that loses nothing and is
read back.

The reference declares a `saveMap` service (srv/saveMap.srv) and never serves it; this is the file a user of the map needs.
PCD v0.7 (the Point Cloud Library's format), fields `x y z`, each `F 8` (float64), so the device's doubles are written and
read back bit for bit.  `DATA binary` by default; `ascii=True` writes every value with 17 significant digits (also exact).
"""
from __future__ import annotations

import os

import numpy as np

_FIELDS = ("x", "y", "z")


def write_pcd(path: str, xyz, ascii: bool = False) -> None:
    """Writes an (n, 3) cloud as PCD v0.7 with float64 x y z."""
    a = np.ascontiguousarray(np.asarray(xyz, dtype="<f8").reshape(-1, 3))
    n = len(a)
    header = ("# .PCD v0.7 - Point Cloud Data file format\n"
              "VERSION 0.7\n"
              "FIELDS x y z\n"
              "SIZE 8 8 8\n"
              "TYPE F F F\n"
              "COUNT 1 1 1\n"
              f"WIDTH {n}\n"
              "HEIGHT 1\n"
              "VIEWPOINT 0 0 0 1 0 0 0\n"
              f"POINTS {n}\n"
              f"DATA {'ascii' if ascii else 'binary'}\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        if ascii:
            fh.write("".join(f"{x:.17g} {y:.17g} {z:.17g}\n" for x, y, z in a.tolist()).encode("ascii"))
        else:
            fh.write(a.tobytes())


def read_pcd(path: str) -> np.ndarray:
    """Reads a PCD v0.7 file whose fields are x y z, float64 (`F 8`), DATA ascii or binary -> (n, 3) float64."""
    with open(path, "rb") as fh:
        raw = fh.read()
    head, pos = {}, 0
    while True:
        end = raw.index(b"\n", pos)
        line = raw[pos:end].decode("ascii").strip()
        pos = end + 1
        if not line or line.startswith("#"):
            continue
        key, _, val = line.partition(" ")
        head[key.upper()] = val.split()
        if key.upper() == "DATA":
            break
    if tuple(head.get("FIELDS", ())) != _FIELDS or head.get("SIZE") != ["8"] * 3 or head.get("TYPE") != ["F"] * 3 \
            or head.get("COUNT", ["1"] * 3) != ["1"] * 3:
        raise ValueError(f"{path}: only FIELDS x y z with SIZE 8 / TYPE F / COUNT 1 are read")
    n = int(head["POINTS"][0])
    kind = head["DATA"][0]
    if kind == "binary":
        body = raw[pos: pos + 24 * n]
        if len(body) != 24 * n:
            raise ValueError(f"{path}: {len(body)} bytes of data for {n} points")
        return np.frombuffer(body, dtype="<f8").reshape(n, 3).astype(np.float64)
    if kind == "ascii":
        vals = np.array(raw[pos:].split(), dtype=np.float64)
        if len(vals) != 3 * n:
            raise ValueError(f"{path}: {len(vals)} values for {n} points")
        return vals.reshape(n, 3)
    raise ValueError(f"{path}: DATA {kind} is not supported")


# ---- the merged voxel map: centroids and the count of returns behind each
_VOX_FIELDS = ("x", "y", "z", "count")
_VOX_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("count", "<i8")])


def write_voxel_pcd(path: str, centroids, counts, ascii: bool = False) -> None:
    """Writes the voxel map's (n, 3) centroids and (n,) counts as PCD v0.7: x y z float64 (`F 8`), count int64 (`I 8`)."""
    c = np.asarray(centroids, dtype="<f8").reshape(-1, 3)
    k = np.asarray(counts, dtype="<i8").reshape(-1)
    if len(c) != len(k):
        raise ValueError(f"{len(c)} centroids, {len(k)} counts")
    n = len(c)
    rec = np.empty(n, _VOX_DTYPE)
    rec["x"], rec["y"], rec["z"], rec["count"] = c[:, 0], c[:, 1], c[:, 2], k
    header = ("# .PCD v0.7 - Point Cloud Data file format\n"
              "VERSION 0.7\n"
              "FIELDS x y z count\n"
              "SIZE 8 8 8 8\n"
              "TYPE F F F I\n"
              "COUNT 1 1 1 1\n"
              f"WIDTH {n}\n"
              "HEIGHT 1\n"
              "VIEWPOINT 0 0 0 1 0 0 0\n"
              f"POINTS {n}\n"
              f"DATA {'ascii' if ascii else 'binary'}\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        if ascii:
            fh.write("".join(f"{x:.17g} {y:.17g} {z:.17g} {int(m)}\n"
                             for (x, y, z), m in zip(c.tolist(), k.tolist())).encode("ascii"))
        else:
            fh.write(rec.tobytes())


def read_voxel_pcd(path: str):
    """Reads a file of write_voxel_pcd (DATA ascii or binary) -> (centroids (n, 3) float64, counts (n,) int64)."""
    with open(path, "rb") as fh:
        raw = fh.read()
    head, pos = {}, 0
    while True:
        end = raw.index(b"\n", pos)
        line = raw[pos:end].decode("ascii").strip()
        pos = end + 1
        if not line or line.startswith("#"):
            continue
        key, _, val = line.partition(" ")
        head[key.upper()] = val.split()
        if key.upper() == "DATA":
            break
    if tuple(head.get("FIELDS", ())) != _VOX_FIELDS or head.get("SIZE") != ["8"] * 4 \
            or head.get("TYPE") != ["F", "F", "F", "I"] or head.get("COUNT", ["1"] * 4) != ["1"] * 4:
        raise ValueError(f"{path}: only FIELDS x y z count with SIZE 8 / TYPE F F F I / COUNT 1 are read")
    n = int(head["POINTS"][0])
    kind = head["DATA"][0]
    if kind == "binary":
        body = raw[pos: pos + 32 * n]
        if len(body) != 32 * n:
            raise ValueError(f"{path}: {len(body)} bytes of data for {n} voxels")
        rec = np.frombuffer(body, dtype=_VOX_DTYPE)
        return np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float64), rec["count"].astype(np.int64)
    if kind == "ascii":
        rows = raw[pos:].split()
        if len(rows) != 4 * n:
            raise ValueError(f"{path}: {len(rows)} values for {n} voxels")
        cols = [rows[i::4] for i in range(4)]
        cen = np.array(cols[:3], dtype=np.float64).T.reshape(n, 3)
        return np.ascontiguousarray(cen), np.array([int(v) for v in cols[3]], dtype=np.int64)
    raise ValueError(f"{path}: DATA {kind} is not supported")


# ---- the carved closed map: the voxels that were not seen through
def write_carved_closed_map_pcd(path: str, H, lo=None, hi=None, min_count=1, min_miss=3, miss_ratio=1.0, ascii: bool = False) -> int:
    """Writes what `H.closed_map_read_carved` keeps of a carved closed map (a HipRegistration after closed_map_build and
    closed_map_carve) as a file of write_voxel_pcd: centroids and counts N -> the voxels written."""
    cen, cnt, _ = H.closed_map_read_carved(lo, hi, min_count, min_miss, miss_ratio)
    write_voxel_pcd(path, cen, cnt, ascii=ascii)
    return len(cnt)


# ---- the closed map's surfels: centroids, unit normals and the count of points behind each
_SURFEL_FIELDS = ("x", "y", "z", "normal_x", "normal_y", "normal_z", "count")
_SURFEL_DTYPE = np.dtype([(f, "<f8") for f in _SURFEL_FIELDS[:6]] + [("count", "<i8")])


def write_surfel_pcd(path: str, centroids, normals, counts, ascii: bool = False) -> None:
    """Writes (n, 3) centroids, (n, 3) normals and (n,) counts as PCD v0.7: x y z normal_x normal_y normal_z float64 (`F 8`),
    count int64 (`I 8`)."""
    c = np.asarray(centroids, dtype="<f8").reshape(-1, 3)
    m = np.asarray(normals, dtype="<f8").reshape(-1, 3)
    k = np.asarray(counts, dtype="<i8").reshape(-1)
    if not len(c) == len(m) == len(k):
        raise ValueError(f"{len(c)} centroids, {len(m)} normals, {len(k)} counts")
    n = len(c)
    rec = np.empty(n, _SURFEL_DTYPE)
    for a in range(3):
        rec[_SURFEL_FIELDS[a]], rec[_SURFEL_FIELDS[3 + a]] = c[:, a], m[:, a]
    rec["count"] = k
    header = ("# .PCD v0.7 - Point Cloud Data file format\n"
              "VERSION 0.7\n"
              f"FIELDS {' '.join(_SURFEL_FIELDS)}\n"
              "SIZE 8 8 8 8 8 8 8\n"
              "TYPE F F F F F F I\n"
              "COUNT 1 1 1 1 1 1 1\n"
              f"WIDTH {n}\n"
              "HEIGHT 1\n"
              "VIEWPOINT 0 0 0 1 0 0 0\n"
              f"POINTS {n}\n"
              f"DATA {'ascii' if ascii else 'binary'}\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        if ascii:
            fh.write("".join(" ".join(f"{v:.17g}" for v in (*p, *q)) + f" {int(j)}\n"
                             for p, q, j in zip(c.tolist(), m.tolist(), k.tolist())).encode("ascii"))
        else:
            fh.write(rec.tobytes())


def read_surfel_pcd(path: str):
    """Reads a file of write_surfel_pcd (DATA ascii or binary) -> (centroids (n, 3), normals (n, 3) float64, counts (n,) int64)."""
    with open(path, "rb") as fh:
        raw = fh.read()
    head, pos = {}, 0
    while True:
        end = raw.index(b"\n", pos)
        line = raw[pos:end].decode("ascii").strip()
        pos = end + 1
        if not line or line.startswith("#"):
            continue
        key, _, val = line.partition(" ")
        head[key.upper()] = val.split()
        if key.upper() == "DATA":
            break
    if tuple(head.get("FIELDS", ())) != _SURFEL_FIELDS or head.get("SIZE") != ["8"] * 7 \
            or head.get("TYPE") != ["F"] * 6 + ["I"] or head.get("COUNT", ["1"] * 7) != ["1"] * 7:
        raise ValueError(f"{path}: only FIELDS {' '.join(_SURFEL_FIELDS)} with SIZE 8 / TYPE F F F F F F I / COUNT 1 are read")
    n = int(head["POINTS"][0])
    kind = head["DATA"][0]
    if kind == "binary":
        body = raw[pos: pos + 56 * n]
        if len(body) != 56 * n:
            raise ValueError(f"{path}: {len(body)} bytes of data for {n} surfels")
        rec = np.frombuffer(body, dtype=_SURFEL_DTYPE)
        cols = [rec[f].astype(np.float64) for f in _SURFEL_FIELDS[:6]]
        return np.stack(cols[:3], axis=1), np.stack(cols[3:], axis=1), rec["count"].astype(np.int64)
    if kind == "ascii":
        rows = raw[pos:].split()
        if len(rows) != 7 * n:
            raise ValueError(f"{path}: {len(rows)} values for {n} surfels")
        vals = np.array([rows[i::7] for i in range(6)], dtype=np.float64).T.reshape(n, 6)
        return (np.ascontiguousarray(vals[:, :3]), np.ascontiguousarray(vals[:, 3:]),
                np.array([int(v) for v in rows[6::7]], dtype=np.int64))
    raise ValueError(f"{path}: DATA {kind} is not supported")


def write_closed_map_surfel_pcd(path: str, H, lo=None, hi=None, min_count=1, max_sigma=float("inf"), min_planarity=0.05,
                                ascii: bool = False) -> int:
    """Writes what `H.closed_map_read_surfels_box` keeps (a HipRegistration after closed_map_build and closed_map_surfels) as a
    file of write_surfel_pcd -> the surfels written."""
    cen, nrm, _, cnt = H.closed_map_read_surfels_box(lo, hi, min_count, max_sigma, min_planarity)
    write_surfel_pcd(path, cen, nrm, cnt, ascii=ascii)
    return len(cnt)


def _write_renamed(path: str, blob: bytes) -> None:
    """`blob` written to a temporary name beside `path` and renamed, so a reader never sees half a file."""
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        with open(tmp, "wb") as fh:
            fh.write(blob)
            fh.flush()
            os.fsync(fh.fileno())
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def save_closed_map(path: str, H, clouds: bool = False) -> int:
    """Writes H's closed map snapshot (H.closed_map_save(clouds)) to `path` -> the bytes written.  Written to a temporary
    name beside it and renamed, so a reader never sees half a file."""
    blob = H.closed_map_save(clouds=clouds)
    _write_renamed(path, blob)
    return len(blob)


def load_closed_map(path: str, H) -> dict:
    """Loads the snapshot file at `path` into H (H.closed_map_load) -> what it held."""
    with open(path, "rb") as fh:
        return H.closed_map_load(fh.read())


# ---- a scan diffed against the closed map: the scan in the map's frame with its labels
_LABEL_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("label", "u1")])


def write_labelled_scan_pcd(path: str, points_world, labels) -> int:
    """Writes a diffed scan as one PCD v0.7, DATA binary: x y z float64 (`F 8`) in the map's frame (the scan under the pose it
    was diffed at) and `label` uint8 (`U 1`: 0 INVALID, 1 SURFACE, 2 OCCUPIED, 3 NEW, H.closed_map_diff's) -> the points
    written.  Written to a temporary name beside `path` and renamed."""
    p = np.asarray(points_world, dtype="<f8").reshape(-1, 3)
    k = np.asarray(labels, dtype="u1").reshape(-1)
    if len(p) != len(k):
        raise ValueError(f"{len(p)} points, {len(k)} labels")
    n = len(p)
    rec = np.empty(n, _LABEL_DTYPE)
    rec["x"], rec["y"], rec["z"], rec["label"] = p[:, 0], p[:, 1], p[:, 2], k
    header = ("# .PCD v0.7 - Point Cloud Data file format\n"
              "VERSION 0.7\n"
              "FIELDS x y z label\n"
              "SIZE 8 8 8 1\n"
              "TYPE F F F U\n"
              "COUNT 1 1 1 1\n"
              f"WIDTH {n}\n"
              "HEIGHT 1\n"
              "VIEWPOINT 0 0 0 1 0 0 0\n"
              f"POINTS {n}\n"
              "DATA binary\n")
    _write_renamed(path, header.encode("ascii") + rec.tobytes())
    return n


# ---- the closed map ray-cast: where the cast rays met the map
_HIT_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("status", "u1")])


def write_raycast_pcd(path: str, pose, ends, status, ranges) -> int:
    """Writes the hit points of a ray-cast (H.closed_map_raycast(ends, pose) -> status, ranges) as one PCD v0.7, DATA binary:
    x y z float64 (`F 8`) in the map's frame -- the point `range` along the segment from the pose's translation to the end under
    the pose -- and `status` uint8 (`U 1`: 2 HIT_CENTROID, 3 HIT_PLANE).  Rays without a hit are left out -> the points written.
    Written to a temporary name beside `path` and renamed."""
    P = np.asarray(pose, dtype=np.float64).reshape(4, 4)
    e = np.asarray(ends, dtype=np.float64).reshape(-1, 3)
    k = np.asarray(status, dtype="u1").reshape(-1)
    r = np.asarray(ranges, dtype=np.float64).reshape(-1)
    if not len(e) == len(k) == len(r):
        raise ValueError(f"{len(e)} ends, {len(k)} statuses, {len(r)} ranges")
    hit = k >= 2
    D = e[hit] @ P[:3, :3].T                          # E - O
    L = np.sqrt((D * D).sum(axis=1))
    X = P[:3, 3] + D * (r[hit] / L)[:, None]
    n = int(hit.sum())
    rec = np.empty(n, _HIT_DTYPE)
    rec["x"], rec["y"], rec["z"], rec["status"] = X[:, 0], X[:, 1], X[:, 2], k[hit]
    header = ("# .PCD v0.7 - Point Cloud Data file format\n"
              "VERSION 0.7\n"
              "FIELDS x y z status\n"
              "SIZE 8 8 8 1\n"
              "TYPE F F F U\n"
              "COUNT 1 1 1 1\n"
              f"WIDTH {n}\n"
              "HEIGHT 1\n"
              "VIEWPOINT 0 0 0 1 0 0 0\n"
              f"POINTS {n}\n"
              "DATA binary\n")
    _write_renamed(path, header.encode("ascii") + rec.tobytes())
    return n


# ---- the closed map's free space: the centres of the cells rays saw through
def write_free_pcd(path: str, H, lo=None, hi=None, ascii: bool = False) -> int:
    """Writes what `H.closed_map_free_cells` reads of a free-space grid (a HipRegistration after closed_map_free_build) as a
    file of write_pcd: the centres of the free cells, brick by brick -> the cells written."""
    cen = H.closed_map_free_cells(lo, hi)
    write_pcd(path, cen, ascii=ascii)
    return len(cen)


# ---- the closed map's clearance: the free cells with their distance to the nearest obstacle
_CLEAR_FIELDS = ("x", "y", "z", "distance")


def write_clearance_pcd(path: str, H, lo=None, hi=None, ascii: bool = False) -> int:
    """Writes the centres `H.closed_map_free_cells` reads (a HipRegistration after closed_map_clearance_build) with
    voxel * sqrt(d2) of each as a fourth field, `distance` (inf beyond the field's radius), as PCD v0.7, four float64 (`F 8`)
    -> the cells written."""
    cen = H.closed_map_free_cells(lo, hi)
    n = len(cen)
    dist = H.closed_map_clearance_points(cen)[2] if n else np.zeros(0)
    rec = np.ascontiguousarray(np.concatenate([cen.reshape(n, 3), dist.reshape(n, 1)], axis=1), dtype="<f8")
    header = ("# .PCD v0.7 - Point Cloud Data file format\n"
              "VERSION 0.7\n"
              "FIELDS x y z distance\n"
              "SIZE 8 8 8 8\n"
              "TYPE F F F F\n"
              "COUNT 1 1 1 1\n"
              f"WIDTH {n}\n"
              "HEIGHT 1\n"
              "VIEWPOINT 0 0 0 1 0 0 0\n"
              f"POINTS {n}\n"
              f"DATA {'ascii' if ascii else 'binary'}\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        if ascii:
            fh.write("".join(" ".join(f"{v:.17g}" for v in row) + "\n" for row in rec.tolist()).encode("ascii"))
        else:
            fh.write(rec.tobytes())
    return n


def read_clearance_pcd(path: str):
    """Reads a file of write_clearance_pcd (DATA ascii or binary) -> (centres (n, 3) float64, distance (n,) float64)."""
    with open(path, "rb") as fh:
        raw = fh.read()
    head, pos = {}, 0
    while True:
        end = raw.index(b"\n", pos)
        line = raw[pos:end].decode("ascii").strip()
        pos = end + 1
        if not line or line.startswith("#"):
            continue
        key, _, val = line.partition(" ")
        head[key.upper()] = val.split()
        if key.upper() == "DATA":
            break
    if tuple(head.get("FIELDS", ())) != _CLEAR_FIELDS or head.get("SIZE") != ["8"] * 4 or head.get("TYPE") != ["F"] * 4:
        raise ValueError(f"{path}: only FIELDS x y z distance with SIZE 8 / TYPE F are read")
    n = int(head["POINTS"][0])
    kind = head["DATA"][0]
    if kind == "binary":
        body = raw[pos: pos + 32 * n]
        if len(body) != 32 * n:
            raise ValueError(f"{path}: {len(body)} bytes of data for {n} cells")
        rec = np.frombuffer(body, dtype="<f8").reshape(n, 4)
    elif kind == "ascii":
        rows = raw[pos:].split()
        if len(rows) != 4 * n:
            raise ValueError(f"{path}: {len(rows)} values for {n} cells")
        rec = np.array([float(v) for v in rows], dtype=np.float64).reshape(n, 4)
    else:
        raise ValueError(f"{path}: DATA {kind} is not supported")
    return np.ascontiguousarray(rec[:, :3]), np.ascontiguousarray(rec[:, 3])


# ---- the route through the closed map: the reached free cells with their cost-to-go, and descended paths
def _write_xyz_and_one(path: str, name: str, rec, ascii: bool) -> None:
    """rows of x y z and one more float64 field `name` as PCD v0.7 (`F 8` each), DATA binary or ascii (17 significant digits)"""
    n = len(rec)
    header = ("# .PCD v0.7 - Point Cloud Data file format\n"
              "VERSION 0.7\n"
              f"FIELDS x y z {name}\n"
              "SIZE 8 8 8 8\n"
              "TYPE F F F F\n"
              "COUNT 1 1 1 1\n"
              f"WIDTH {n}\n"
              "HEIGHT 1\n"
              "VIEWPOINT 0 0 0 1 0 0 0\n"
              f"POINTS {n}\n"
              f"DATA {'ascii' if ascii else 'binary'}\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        if ascii:
            fh.write("".join(" ".join(f"{v:.17g}" for v in row) + "\n" for row in rec.tolist()).encode("ascii"))
        else:
            fh.write(rec.tobytes())


def _read_xyz_and_one(path: str, name: str):
    """a file of _write_xyz_and_one -> (n, 4) float64"""
    with open(path, "rb") as fh:
        raw = fh.read()
    head, pos = {}, 0
    while True:
        end = raw.index(b"\n", pos)
        line = raw[pos:end].decode("ascii").strip()
        pos = end + 1
        if not line or line.startswith("#"):
            continue
        key, _, val = line.partition(" ")
        head[key.upper()] = val.split()
        if key.upper() == "DATA":
            break
    if head.get("FIELDS") != ["x", "y", "z", name] or head.get("SIZE") != ["8"] * 4 or head.get("TYPE") != ["F"] * 4:
        raise ValueError(f"{path}: only FIELDS x y z {name} with SIZE 8 / TYPE F are read")
    n = int(head["POINTS"][0])
    kind = head["DATA"][0]
    if kind == "binary":
        body = raw[pos: pos + 32 * n]
        if len(body) != 32 * n:
            raise ValueError(f"{path}: {len(body)} bytes of data for {n} points")
        return np.frombuffer(body, dtype="<f8").reshape(n, 4)
    if kind == "ascii":
        rows = raw[pos:].split()
        if len(rows) != 4 * n:
            raise ValueError(f"{path}: {len(rows)} values for {n} points")
        return np.array([float(v) for v in rows], dtype=np.float64).reshape(n, 4)
    raise ValueError(f"{path}: DATA {kind} is not supported")


def write_route_pcd(path: str, H, lo=None, hi=None, ascii: bool = False) -> int:
    """Writes the centres `H.closed_map_free_cells` reads (a HipRegistration after closed_map_route_build) that a goal reaches,
    with voxel * cost / 3 of each as a fourth field, `route` (metres to the nearest goal along the 3-4-5 chamfer), as PCD v0.7,
    four float64 (`F 8`) -> the cells written."""
    cen = H.closed_map_free_cells(lo, hi)
    dist = H.closed_map_route_points(cen)[1] if len(cen) else np.zeros(0)
    keep = np.isfinite(dist)
    rec = np.ascontiguousarray(np.concatenate([cen.reshape(-1, 3)[keep], dist[keep].reshape(-1, 1)], axis=1), dtype="<f8")
    _write_xyz_and_one(path, "route", rec, ascii)
    return len(rec)


def read_route_pcd(path: str):
    """Reads a file of write_route_pcd (DATA ascii or binary) -> (centres (n, 3) float64, route (n,) float64)."""
    rec = _read_xyz_and_one(path, "route")
    return np.ascontiguousarray(rec[:, :3]), np.ascontiguousarray(rec[:, 3])


def write_route_paths_pcd(path: str, H, starts, max_cells: int, pose=None, ascii: bool = False) -> int:
    """Writes the waypoints of `H.closed_map_route_paths(starts, max_cells, pose)`, path after path, each with the index of its
    start as a fourth field, `path` (float64 like the rest: `F 8`); a start without a path writes nothing -> the waypoints
    written."""
    _, count, _, centres = H.closed_map_route_paths(starts, max_cells, pose)
    rows = [np.concatenate([centres[i, :count[i]], np.full((count[i], 1), float(i))], axis=1) for i in range(len(count)) if count[i]]
    rec = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 4)), dtype="<f8")
    _write_xyz_and_one(path, "path", rec, ascii)
    return len(rec)


def read_route_paths_pcd(path: str):
    """Reads a file of write_route_paths_pcd -> (waypoints (n, 3) float64, path index (n,) int64)."""
    rec = _read_xyz_and_one(path, "path")
    return np.ascontiguousarray(rec[:, :3]), rec[:, 3].astype(np.int64)


# ---- the frontiers of the closed map: the kept clusters' cells with their cluster index, and the clusters
def _write_xyz_and_fields(path: str, names, rec, ascii: bool) -> None:
    """rows of x y z and the float64 fields `names` as PCD v0.7 (`F 8` each), DATA binary or ascii (17 significant digits)"""
    n, k = len(rec), 3 + len(names)
    header = ("# .PCD v0.7 - Point Cloud Data file format\n"
              "VERSION 0.7\n"
              f"FIELDS x y z {' '.join(names)}\n"
              f"SIZE {' '.join(['8'] * k)}\n"
              f"TYPE {' '.join(['F'] * k)}\n"
              f"COUNT {' '.join(['1'] * k)}\n"
              f"WIDTH {n}\n"
              "HEIGHT 1\n"
              "VIEWPOINT 0 0 0 1 0 0 0\n"
              f"POINTS {n}\n"
              f"DATA {'ascii' if ascii else 'binary'}\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        if ascii:
            fh.write("".join(" ".join(f"{v:.17g}" for v in row) + "\n" for row in rec.tolist()).encode("ascii"))
        else:
            fh.write(rec.tobytes())


def _read_xyz_and_fields(path: str, names):
    """a file of _write_xyz_and_fields -> (n, 3 + len(names)) float64"""
    with open(path, "rb") as fh:
        raw = fh.read()
    head, pos, k = {}, 0, 3 + len(names)
    while True:
        end = raw.index(b"\n", pos)
        line = raw[pos:end].decode("ascii").strip()
        pos = end + 1
        if not line or line.startswith("#"):
            continue
        key, _, val = line.partition(" ")
        head[key.upper()] = val.split()
        if key.upper() == "DATA":
            break
    if head.get("FIELDS") != ["x", "y", "z", *names] or head.get("SIZE") != ["8"] * k or head.get("TYPE") != ["F"] * k:
        raise ValueError(f"{path}: only FIELDS x y z {' '.join(names)} with SIZE 8 / TYPE F are read")
    n = int(head["POINTS"][0])
    kind = head["DATA"][0]
    if kind == "binary":
        body = raw[pos: pos + 8 * k * n]
        if len(body) != 8 * k * n:
            raise ValueError(f"{path}: {len(body)} bytes of data for {n} points")
        return np.frombuffer(body, dtype="<f8").reshape(n, k)
    if kind == "ascii":
        rows = raw[pos:].split()
        if len(rows) != k * n:
            raise ValueError(f"{path}: {len(rows)} values for {n} points")
        return np.array([float(v) for v in rows], dtype=np.float64).reshape(n, k)
    raise ValueError(f"{path}: DATA {kind} is not supported")


def write_frontier_pcd(path: str, H, ascii: bool = False) -> int:
    """Writes the centres of the frontier cells of the kept clusters (a HipRegistration after closed_map_frontier_build), ascending
    in linear index, each with the index of its cluster in the kept list as a fourth field, `cluster` (float64 like the rest:
    `F 8`), as PCD v0.7 -> the cells written."""
    cen, roots = H.closed_map_frontier_cells()
    kept = H.closed_map_frontier_clusters()[0]["root"]
    index = np.searchsorted(kept, roots).astype(np.float64)
    rec = np.ascontiguousarray(np.concatenate([cen.reshape(-1, 3), index.reshape(-1, 1)], axis=1), dtype="<f8")
    _write_xyz_and_fields(path, ["cluster"], rec, ascii)
    return len(rec)


def read_frontier_pcd(path: str):
    """Reads a file of write_frontier_pcd (DATA ascii or binary) -> (centres (n, 3) float64, cluster index (n,) int64)."""
    rec = _read_xyz_and_fields(path, ["cluster"])
    return np.ascontiguousarray(rec[:, :3]), rec[:, 3].astype(np.int64)


def write_frontier_clusters_pcd(path: str, H, with_cost: bool = True, ascii: bool = False) -> int:
    """Writes the centroids of the kept clusters with `cells`, `unknown_faces` and `cost` (closed_map_frontier_costs' -- it needs a
    built route field --, or with_cost False: NaN) as PCD v0.7, six float64 (`F 8`) -> the clusters written."""
    rec, cen = H.closed_map_frontier_clusters()
    cost = H.closed_map_frontier_costs()[0].astype(np.float64) if with_cost else np.full(len(rec), np.nan)
    rows = np.concatenate([cen.reshape(-1, 3), rec["cells"].astype(np.float64).reshape(-1, 1),
                           rec["unknown_faces"].astype(np.float64).reshape(-1, 1), cost.reshape(-1, 1)], axis=1)
    _write_xyz_and_fields(path, ["cells", "unknown_faces", "cost"], np.ascontiguousarray(rows, dtype="<f8"), ascii)
    return len(rows)


def read_frontier_clusters_pcd(path: str):
    """Reads a file of write_frontier_clusters_pcd -> (centroids (k, 3) float64, cells (k,) int64, unknown_faces (k,) int64,
    cost (k,) float64)."""
    rec = _read_xyz_and_fields(path, ["cells", "unknown_faces", "cost"])
    return np.ascontiguousarray(rec[:, :3]), rec[:, 3].astype(np.int64), rec[:, 4].astype(np.int64), np.ascontiguousarray(rec[:, 5])


def write_view_pcd(path: str, H, pose, ends, ascii: bool = False) -> int:
    """Writes the centres of the distinct UNKNOWN cells one view sees (a HipRegistration after closed_map_frontier_build; `pose`
    4 x 4, `ends` (r, 3) in the sensor frame: closed_map_view_cells), ascending in window bit index, as PCD v0.7 -> the cells
    written: the view's gain."""
    cen, _ = H.closed_map_view_cells(pose, ends)
    write_pcd(path, cen, ascii=ascii)
    return len(cen)


def read_view_pcd(path: str) -> np.ndarray:
    """Reads a file of write_view_pcd (DATA ascii or binary) -> centres (n, 3) float64."""
    return read_pcd(path)
