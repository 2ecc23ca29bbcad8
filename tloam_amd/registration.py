"""Host-side mirror of the reference's registration plugin, bound to the C ABI (include/tloam_hip.h).

`HipRegistration` follows tloam::RegistrationInterface
(include/tloam/models/registration/registration_interface.hpp:40-48):

    setInputSource(Frame&)            -> set_input_source(frame)
    setInputTarget(Frame&)            -> set_input_target(frame)
    scanMatching(out, predict, pose)  -> scan_matching(predict, ...)  -> (ok, result_pose)
    getFitnessScore()                 -> get_fitness_score()

and is selected the way FrontEnd::initRegistraton selects "TLS" (front_end.cpp:155-167): see
`make_registration("TLS_HIP", cfg)`.  All computation happens in libtloam_hip.so (hand-written HIP
kernels for gfx950); this module only marshals numpy arrays into the C ABI through ctypes.  There is
no CPU fallback: a missing library or a missing GPU raises.
"""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from .abi import *  # noqa: F401,F403 -- the constants, the structures, SIGNATURES, load_library: this module's public names too


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _lp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64))


def _u8p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))


def _u16p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint16))


def _u32p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))


def _per_point(n, want_ids):
    """the per-point outputs of a scan query, never empty -> (bytes (max(n, 1),) uint8, ids (max(n, 1),) int32 or None, cut);
    cut(a): the first n of `a` as the caller's own copy (None stays None)"""
    return (np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int32) if want_ids else None,
            lambda a: None if a is None else a[:n].copy())


def _box(lo, hi):
    """the two corners of a box read, both or neither -> ((3,) float64, (3,) float64) or (None, None)"""
    if (lo is None) != (hi is None):
        raise ValueError("lo and hi go together")
    if lo is None:
        return None, None
    return np.ascontiguousarray(lo, dtype=np.float64).reshape(3), np.ascontiguousarray(hi, dtype=np.float64).reshape(3)


def _aos(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, 3))


def _colmajor(T):
    return np.ascontiguousarray(np.asarray(T, dtype=np.float64).T).reshape(-1)


def _id_range(first, count, total):
    """ids [first, first + count) of a list of total() entries (asked only when count is None: to the end) -> (first, count)"""
    first = int(first)
    return first, int(max(total() - first, 0) if count is None else count)


def _double3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


# every configuration struct: the C function that fills in its defaults, and what an override of a field passes through
_CONFIGS = {
    TlsConfig: ("tloam_default_config", {}),
    SubmapConfig: ("tloam_submap_default_config", {}),
    FeatureConfig: ("tloam_feature_default_config", {}),
    SegConfig: ("tloam_seg_default_config", {}),
    OdomConfig: ("tloam_odom_default_config", {}),
    MapConfig: ("tloam_map_default_config", {}),
    VoxelMapConfig: ("tloam_voxel_map_default_config", {"origin": _double3}),
    DeskewConfig: ("tloam_deskew_default_config", {}),
    PlaceConfig: ("tloam_place_default_config", {}),
    LoopConfig: ("tloam_loop_default_config", {}),
    GraphConfig: ("tloam_graph_default_config", {}),
    GraphRobustConfig: ("tloam_graph_robust_default_config", {}),
    ClosedMapConfig: ("tloam_closed_map_default_config", {"origin": _double3}),
    ClosedMapCarveConfig: ("tloam_closed_map_carve_default_config", {}),
    ClosedMapSurfelConfig: ("tloam_closed_map_surfel_default_config", {}),
    ClosedMapLocaliseConfig: ("tloam_closed_map_localise_default_config", {}),
    ClosedMapRelocaliseConfig: ("tloam_closed_map_relocalise_default_config", {}),
    ClosedMapDiffConfig: ("tloam_closed_map_diff_default_config", {}),
    ClosedMapRaycastConfig: ("tloam_closed_map_raycast_default_config", {}),
    FreeConfig: ("tloam_closed_map_free_default_config", {}),
    ClearanceConfig: ("tloam_closed_map_clearance_default_config", {}),
    RouteConfig: ("tloam_closed_map_route_default_config", {}),
    FrontierConfig: ("tloam_closed_map_frontier_default_config", {}),
    ViewConfig: ("tloam_closed_map_view_default_config", {}),
}


def _default(cls, over):
    """`cls` as the library's default function fills it, then the keyword overrides (passed through the table's coercion where
    the field has one); `<sub>__<field>` names a field of the nested struct `<sub>`.  A name the struct does not have raises
    KeyError."""
    default_fn, coerce = _CONFIGS[cls]
    cfg = cls()
    getattr(load_library(), default_fn)(C.byref(cfg))
    for k, v in over.items():
        sub, sep, field = k.rpartition("__")   # (no "__": field is k)
        target = getattr(cfg, sub, None) if sep else cfg
        if not isinstance(target, C.Structure) or not hasattr(target, field):
            raise KeyError(k)
        setattr(target, field, coerce[k](v) if k in coerce else v)
    return cfg


def default_config(**over) -> TlsConfig:
    return _default(TlsConfig, over)


def shard_range(n, rank, nranks):
    lo, hi = C.c_size_t(0), C.c_size_t(0)
    load_library().tloam_shard_range(C.c_size_t(n), int(rank), int(nranks), C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def shard_ranges_frame(n4, rank, nranks):
    """[(lo, hi)] x 4: the blocks of a whole Frame a sharded context keeps (tloam_shard_ranges_frame)."""
    n = (C.c_size_t * 4)(*[int(v) for v in n4])
    lo, hi = (C.c_size_t * 4)(), (C.c_size_t * 4)()
    load_library().tloam_shard_ranges_frame(n, int(rank), int(nranks), lo, hi)
    return [(int(lo[k]), int(hi[k])) for k in range(4)]


def closed_map_probe(blob) -> dict:
    """what a closed map snapshot says it holds, from its header and section table alone (host only: no context, no GPU);
    raises TloamHipError when they do not hold"""
    blob = bytes(blob)
    info = ClosedMapSnapshotInfo()
    rc = load_library().tloam_closed_map_probe(blob, len(blob), C.byref(info))
    if rc:
        raise TloamHipError(f"tloam_closed_map_probe: {STATUS.get(rc, rc)}")
    return info.as_dict()


def se3_exp(x):
    T = np.zeros(16)
    rc = load_library().tloam_se3_exp(_dp(np.ascontiguousarray(x, float)), _dp(T))
    if rc:
        raise TloamHipError(STATUS.get(rc, rc))
    return T.reshape(4, 4).T.copy()


def se3_log(T):
    x = np.zeros(6)
    rc = load_library().tloam_se3_log(_dp(_colmajor(T)), _dp(x))
    if rc:
        raise TloamHipError(STATUS.get(rc, rc))
    return x


def se3_plus(x, delta):
    o = np.zeros(6)
    load_library().tloam_se3_plus(_dp(np.ascontiguousarray(x, float)), _dp(np.ascontiguousarray(delta, float)), _dp(o))
    return o


class HipRegistration:
    """MI355X-native drop-in for tloam::LocalRegistration behind RegistrationInterface."""

    def __init__(self, cfg: TlsConfig | None = None, device: int = 0):
        self.L = load_library()
        self.cfg = cfg if cfg is not None else default_config()
        self.h = C.c_void_p()
        rc = self.L.tloam_create(C.byref(self.cfg), int(device), C.byref(self.h))
        if rc != 0:
            raise TloamHipError(f"tloam_create: {STATUS.get(rc, rc)} -- a gfx950 (MI355X) device is required; "
                                "this path has no CPU fallback")
        self._n = {}
        self._cb = None
        # marshalling buffers of scan_match (column-major 4x4 in / out), allocated once: the binding adds ~3 us per
        # call instead of ~10
        self._pred_buf, self._res_buf = (C.c_double * 16)(), (C.c_double * 16)()
        self._pred_view = np.frombuffer(self._pred_buf).reshape(4, 4).T
        self._res_view = np.frombuffer(self._res_buf).reshape(4, 4).T

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.L.tloam_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self.L.tloam_last_error(self.h)
            raise TloamHipError(f"{what}: {STATUS.get(rc, rc)} {msg.decode() if msg else ''}")

    # ---- RegistrationInterface ------------------------------------------------------------
    def _note(self, rc, what):
        """entry points whose status the caller inspects (they do not raise): a HIP / exchange failure leaves its text on stderr"""
        if rc in (-4, -5):
            sys.stderr.write(f"[tloam_amd] {what}: {STATUS.get(rc, rc)}: {self.L.tloam_last_error(self.h).decode(errors='replace')}\n")
        return rc

    def _call(self, name, *args):
        """the entry point `name` on this context, its status checked under that name"""
        rc = getattr(self.L, name)(self.h, *args)
        self._check(rc, name)
        return rc

    def _configure(self, cls, name, cfg, over):
        """a configure entry point: `cfg`, or `cls`'s defaults with the overrides when it is None -> the struct that was set"""
        cfg = cfg if cfg is not None else _default(cls, over)
        self._call(name, C.byref(cfg))
        return cfg

    def _info(self, cls, name, *head):
        """an entry point whose last argument is an info struct it fills -> its dict"""
        info = cls()
        self._call(name, *head, C.byref(info))
        return info.as_dict()

    def _read_list(self, name, rec_type, *head):
        """a list getter's two calls, name(ctx, *head, capacity, n, records): the count, then the records -> [dict]"""
        n = C.c_size_t(0)
        self._call(name, *head, 0, C.byref(n), None)
        if not n.value:
            return []
        rec = (rec_type * n.value)()
        self._call(name, *head, n.value, C.byref(n), rec)
        return [r.as_dict() for r in rec[: n.value]]

    def _read_box(self, name, head, columns):
        """a box read's two calls, name(ctx, *head, capacity, n, *columns): the probe for the count (a short capacity, -1, with
        n > 0 is its answer), then the columns -- (width, or None for a vector; dtype float64 or int64) each -- fetched and trimmed"""
        n = C.c_size_t(0)
        rc = getattr(self.L, name)(self.h, *head, 0, C.byref(n), *[None] * len(columns))
        if rc not in (0, -1) or (rc == -1 and n.value == 0):
            self._check(rc, name)
        m = n.value
        cols = [np.zeros((max(m, 1), w) if w else max(m, 1), dt) for w, dt in columns]
        if m:
            self._call(name, *head, m, C.byref(n), *[_dp(a) if a.dtype == np.float64 else _lp(a) for a in cols])
        return tuple(a[: n.value].copy() for a in cols)

    def _frame_call(self, fn, name, tag, frame):
        clouds = [_aos(frame.cloud(k)) for k in range(4)]
        ptrs = (C.POINTER(C.c_double) * 4)(*[_dp(a) for a in clouds])
        ns = (C.c_size_t * 4)(*[len(a) for a in clouds])
        for k in range(4):
            self._n[(tag, k)] = len(clouds[k])
        self._check(fn(self.h, ptrs, ns), name)
        return True

    def set_input_source(self, frame) -> bool:
        """setInputSource (registration.cpp:232-239): the four clouds of the Frame in one call."""
        return self._frame_call(self.L.tloam_set_source_frame, "tloam_set_source_frame", "s", frame)

    def set_input_target(self, frame) -> bool:
        """setInputTarget (registration.cpp:241-248)."""
        return self._frame_call(self.L.tloam_set_target_frame, "tloam_set_target_frame", "t", frame)

    def scan_matching(self, predict_pose, omega_perturb=None, scan_cloud=None):
        """scanMatching (registration.cpp:879-1133) -> (True, result_pose 4x4).  `scan_cloud`
        ((n,3) float64, C-contiguous) is transformed in place like out_result_.scan_cloud."""
        rc, T, st = self.scan_match(predict_pose, omega_perturb, scan_cloud)
        self._check(rc, "tloam_scan_match")
        self.last_stats = st
        return True, T

    def get_fitness_score(self):
        """getFitnessScore (registration.cpp:257-296)."""
        f, r = C.c_double(0), C.c_double(0)
        self._call("tloam_fitness", C.byref(f), C.byref(r))
        return f.value, r.value

    # ---- C ABI, one to one --------------------------------------------------------------------
    def set_source(self, kind, xyz):
        a = _aos(xyz)
        self._n[("s", kind)] = len(a)
        return self._call("tloam_set_source", int(kind), _dp(a), len(a))

    def set_target(self, kind, xyz):
        a = _aos(xyz)
        self._n[("t", kind)] = len(a)
        return self._call("tloam_set_target", int(kind), _dp(a), len(a))

    def set_frames(self, source, target):
        self.set_input_source(source)
        self.set_input_target(target)

    def frame_stash(self, slot):
        """tloam_frame_stash: the registered clouds move into slot `slot` of the HBM frame store."""
        self._call("tloam_frame_stash", int(slot))

    def frame_select(self, slot):
        """tloam_frame_select: the clouds of `slot` become the registered ones (-1: the context's own); O(1)."""
        self._call("tloam_frame_select", int(slot))

    def scan_match(self, predict, omega=None, scan=None):
        self._pred_view[...] = predict
        self._res_view[...] = 0.0
        st = Stats()
        om = None if omega is None else np.ascontiguousarray(omega, float)
        if scan is not None:
            assert scan.dtype == np.float64 and scan.flags.c_contiguous
        rc = self.L.tloam_scan_match(self.h, self._pred_buf, _dp(om), self._res_buf, _dp(scan),
                                     0 if scan is None else len(scan), C.byref(st))
        self._note(rc, "tloam_scan_match")
        return rc, self._res_view.copy(), st.as_dict()

    def sm_begin(self, predict, omega=None):
        om = None if omega is None else np.ascontiguousarray(omega, float)
        return self._note(self.L.tloam_sm_begin(self.h, _dp(_colmajor(predict)), _dp(om)), "tloam_sm_begin")

    def sm_outer(self):
        done = C.c_int(0)
        st = Stats()
        rc = self._note(self.L.tloam_sm_outer(self.h, C.byref(done), C.byref(st)), "tloam_sm_outer")
        return rc, bool(done.value), st.as_dict()

    def sm_end(self):
        res = np.zeros(16)
        st = Stats()
        rc = self._note(self.L.tloam_sm_end(self.h, _dp(res), C.byref(st)), "tloam_sm_end")
        return rc, res.reshape(4, 4).T.copy(), st.as_dict()

    # ---- device-resident submap (FrontEnd::updateSubmap, front_end.cpp:201-275 / :283-304)
    def submap_init(self, planar, sphere, edge, ground, cfg: SubmapConfig | None = None):
        cl = [_aos(x) for x in (planar, sphere, edge, ground)]
        args = []
        for a in cl:
            args += [_dp(a), len(a)]
        return self._call("tloam_submap_init", C.byref(cfg) if cfg is not None else None, *args)

    def submap_update(self, pose, planar, sphere, edge, ground):
        m = np.ascontiguousarray(np.asarray(pose, float).reshape(4, 4).T.ravel())  # column-major
        cl = [_aos(x) for x in (planar, sphere, edge, ground)]
        args = []
        for a in cl:
            args += [_dp(a), len(a)]
        return self._call("tloam_submap_update", _dp(m), *args)

    def get_target(self, kind):
        n = C.c_size_t(0)
        self.L.tloam_get_target(self.h, int(kind), 0, C.byref(n), None)
        out = np.zeros((max(n.value, 1), 3))
        if n.value:
            self._call("tloam_get_target", int(kind), n.value, C.byref(n), _dp(out))
        self._n[("t", kind)] = n.value
        return out[: n.value].copy()

    # ---- PCA feature extraction (featureExtract::calculatePCAInfo / extractPlanarSphere)
    def pca_info(self, xyz, cfg: FeatureConfig | None = None):
        cfg = cfg or default_feature_config()
        a = _aos(xyz)
        n, K = len(a), cfg.K
        out = dict(flatness=np.zeros(n), cvr=np.zeros(n), sphericity=np.zeros(n), normal=np.zeros((max(n, 1), 3)),
                   num_sum=np.zeros(n, np.int32), neigh=np.zeros((max(n, 1), K), np.int32))
        self._call("tloam_pca_info", C.byref(cfg), _dp(a), n, _dp(out["flatness"]), _dp(out["cvr"]), _dp(out["sphericity"]),
                   _dp(out["normal"]), _ip(out["num_sum"]), _ip(out["neigh"]))
        out["normal"] = out["normal"][:n]
        out["neigh"] = out["neigh"][:n]
        return out

    def extract_planar_sphere(self, xyz, cfg: FeatureConfig | None = None):
        """-> (planar_scan_index, planar_submap_index, sphere_scan_index, sphere_submap_index)"""
        cfg = cfg or default_feature_config()
        a = _aos(xyz)
        n = len(a)
        lists = [np.zeros(max(n, 1), np.int32) for _ in range(4)]
        cnt = [C.c_size_t(0) for _ in range(4)]
        args = []
        for l, k in zip(lists, cnt):
            args += [_ip(l), C.byref(k)]
        self._call("tloam_extract_planar_sphere", C.byref(cfg), _dp(a), n, *args)
        return tuple(l[: k.value].copy() for l, k in zip(lists, cnt))

    # ---- segmentation node (Segmentation::spinOnce, segmentation.cpp:40-93)
    def segment(self, xyz, cfg: SegConfig | None = None):
        """one raw scan -> dict: status (0, or -2 when the node publishes nothing), ring (per input point, -1 filtered),
        ground, object, segmented + label, edge, general (index lists into `xyz`), boxes (clusters x 6).  Raises on
        any other status."""
        cfg = cfg or default_seg_config()
        a = _aos(xyz)
        n = len(a)
        m = max(n, 1)
        ring = np.zeros(m, np.int32)
        lists = {k: np.zeros(m, np.int32) for k in ("ground", "object", "segmented", "label", "edge", "general")}
        boxes = np.zeros((m, 6))
        cnt = {k: C.c_size_t(0) for k in ("ground", "object", "segmented", "edge", "general", "boxes")}
        rc = self.L.tloam_segment(self.h, C.byref(cfg), _dp(a), n, _ip(ring), _ip(lists["ground"]), C.byref(cnt["ground"]),
                                  _ip(lists["object"]), C.byref(cnt["object"]), _ip(lists["segmented"]), _ip(lists["label"]),
                                  C.byref(cnt["segmented"]), _ip(lists["edge"]), C.byref(cnt["edge"]), _ip(lists["general"]),
                                  C.byref(cnt["general"]), _dp(boxes), m, C.byref(cnt["boxes"]))
        if rc not in (0, -2):
            self._check(rc, "tloam_segment")
        out = {"status": rc, "ring": ring[:n].copy()}
        for k in ("ground", "object", "segmented", "edge", "general"):
            out[k] = lists[k][: cnt[k].value].copy()
        out["label"] = lists["label"][: cnt["segmented"].value].copy()
        out["boxes"] = boxes[: cnt["boxes"].value].copy()
        return out

    # ---- per-scan voxel grid and the whole odometry frame (FrontEnd::updateLidarOdometry, front_end.cpp:278-337)
    def voxel_down_sample(self, xyz, voxel):
        """PointCloud2::VoxelDownSample on the device: voxel means in order of first occurrence.  Raises on
        TLOAM_E_INVALID (voxel <= 0, voxel too small)."""
        a = _aos(xyz)
        out = np.zeros((max(len(a), 1), 3))
        n = C.c_size_t(0)
        self._call("tloam_voxel_down_sample", float(voxel), _dp(a), len(a), _dp(out), len(out), C.byref(n))
        return out[: n.value].copy()

    def odometry_reset(self, init_pose=None, cfg: OdomConfig | None = None):
        """FrontEnd::setInitPose + a fresh odometry state (the next frame is the first one)."""
        T = None if init_pose is None else _colmajor(init_pose)
        self._call("tloam_odometry_reset", C.byref(cfg) if cfg is not None else None, _dp(T))

    def odometry_frame(self, xyz, times=None):
        """one raw scan -> (rc, pose 4x4, stats dict).  rc: 0, -2 (TLOAM_E_TOO_FEW_POINTS: the frame is skipped) or
        -7 (TLOAM_E_WEIGHT_RANGE: pose written, as scan_match); raises on any other status.  times: per-point seconds relative
        to the pose's instant -- tloam_odometry_frame_timed (deskew configured with time_source 1)."""
        a = _aos(xyz)
        T = np.zeros(16)
        st = OdomStats()
        if times is None:
            rc = self.L.tloam_odometry_frame(self.h, _dp(a), len(a), _dp(T), C.byref(st))
        else:
            t = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
            if len(t) != len(a):
                raise ValueError(f"{len(t)} times for {len(a)} points")
            rc = self.L.tloam_odometry_frame_timed(self.h, _dp(a), _dp(t), len(a), _dp(T), C.byref(st))
        if rc not in (0, -2, -7):
            self._check(rc, "tloam_odometry_frame_timed" if times is not None else "tloam_odometry_frame")
        if rc != -2 and st.frame > 0:   # the getters' capacities: this frame's source clouds, in kind order
            for k, m in enumerate((st.n_planar_scan, st.n_ground_ds, st.n_edge_ds, st.n_sphere_scan)):
                self._n[("s", k)] = int(m)
        return rc, T.reshape(4, 4).T.copy(), st.as_dict()

    # ---- the global map and the registered scan (FrontEnd::spinOnce :84-92, updateSubmap :269-274)
    def map_configure(self, cfg: MapConfig | None = None, **over):
        """mapping on / off (default_map_config(**over) when cfg is None); empties the map.  Kept across odometry_reset."""
        self._configure(MapConfig, "tloam_map_configure", cfg, over)

    def map_info(self) -> dict:
        return self._info(MapInfo, "tloam_map_get_info")

    def map_read(self, first=0, count=None):
        """points [first, first + count) of the global map as an (m, 3) float64 array (count None: to the end)"""
        first, m = _id_range(first, count, lambda: self.map_info()["n_points"])
        out = np.zeros((max(m, 1), 3))
        self._call("tloam_map_read", first, m, _dp(out))
        return out[:m].copy()

    def registered_scan(self):
        """the last accepted frame's raw scan transformed by its pose (/raw_cloud, front_end.cpp:84-86) as (n, 3)"""
        n = C.c_size_t(0)
        rc = self.L.tloam_registered_scan(self.h, 0, C.byref(n), None)
        if rc not in (0, -1) or (rc == -1 and n.value == 0):
            self._check(rc, "tloam_registered_scan")
        out = np.zeros((max(n.value, 1), 3))
        self._call("tloam_registered_scan", n.value, C.byref(n), _dp(out))
        return out[: n.value].copy()

    # ---- the merged voxel map
    def voxel_map_configure(self, cfg: VoxelMapConfig | None = None, **over):
        """voxel map on / off (default_voxel_map_config(**over) when cfg is None); empties it.  Kept across odometry_reset."""
        self._configure(VoxelMapConfig, "tloam_voxel_map_configure", cfg, over)

    def voxel_map_info(self) -> dict:
        return self._info(VoxelMapInfo, "tloam_voxel_map_get_info")

    def voxel_map_read(self, first=0, count=None):
        """voxels [first, first + count) in id order -> (centroids (m, 3) float64, counts (m,) int64); count None: to the end"""
        first, m = _id_range(first, count, lambda: self.voxel_map_info()["n_voxels"])
        cen, cnt = np.zeros((max(m, 1), 3)), np.zeros(max(m, 1), np.int64)
        self._call("tloam_voxel_map_read", int(first), m, _dp(cen), _lp(cnt))
        return cen[:m].copy(), cnt[:m].copy()

    def voxel_map_read_box(self, lo, hi, min_count=1):
        """the voxels whose centroid lies in [lo, hi] (inclusive, every axis) with N >= min_count, in id order ->
        (centroids (m, 3), counts (m,))"""
        lo = np.ascontiguousarray(lo, dtype=np.float64).reshape(3)
        hi = np.ascontiguousarray(hi, dtype=np.float64).reshape(3)
        return self._read_box("tloam_voxel_map_read_box", (_dp(lo), _dp(hi), int(min_count)), [(3, np.float64), (None, np.int64)])

    # ---- deskew of the frame's scan under constant velocity
    def deskew_configure(self, cfg: DeskewConfig | None = None, **over):
        """deskew on / off (default_deskew_config(**over) when cfg is None).  Kept across odometry_reset."""
        self._configure(DeskewConfig, "tloam_deskew_configure", cfg, over)

    def deskew_info(self) -> dict:
        return self._info(DeskewInfo, "tloam_deskew_get_info")

    def deskew_scan(self, xyz, motion, cfg: DeskewConfig | None = None, scan_period=0.1, times=None):
        """the correction alone, on the device: (n, 3) scan, motion = the step (4x4 rigid), times in seconds (timed mode) ->
        the deskewed (n, 3) scan"""
        cfg = cfg if cfg is not None else default_deskew_config(enabled=1, time_source=0 if times is None else 1)
        a = _aos(xyz)
        t = None if times is None else np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
        if t is not None and len(t) != len(a):
            raise ValueError(f"{len(t)} times for {len(a)} points")
        out = np.zeros((max(len(a), 1), 3))
        M = _colmajor(motion)
        self._call("tloam_deskew_scan", C.byref(cfg), float(scan_period), _dp(M), _dp(a), _dp(t), len(a), _dp(out))
        return out[: len(a)].copy()

    # ---- place recognition: Scan Context keyframes and loop search
    def place_configure(self, cfg: PlaceConfig | None = None, **over):
        """place recognition on / off (default_place_config(**over) when cfg is None); empties the keyframe database.  Kept
        across odometry_reset (which empties the database too)."""
        self._place_cfg = self._configure(PlaceConfig, "tloam_place_configure", cfg, over)

    def _place_grid(self):
        cfg = getattr(self, "_place_cfg", None) or default_place_config()
        return int(cfg.n_rings), int(cfg.n_sectors)

    def place_info(self) -> dict:
        """keyframes, loops (this waits for the device's work in flight), the last keyframe's frame, capacity"""
        return self._info(PlaceInfo, "tloam_place_get_info")

    def place_add_scan(self, xyz, pose, frame_id=-1) -> int:
        """one scan (sensor frame) with the caller's pose (4x4), added as a keyframe and searched -> its keyframe id"""
        a = _aos(xyz)
        M = _colmajor(pose)
        kf = C.c_int64(-1)
        self._call("tloam_place_add_scan", _dp(a), len(a), _dp(M), int(frame_id), C.byref(kf))
        return int(kf.value)

    def place_describe(self, xyz, cfg: PlaceConfig | None = None):
        """the Scan Context of one scan -> (descriptor (n_rings, n_sectors), ring_key, sector_key); cfg None: the context's"""
        R, S = (int(cfg.n_rings), int(cfg.n_sectors)) if cfg is not None else self._place_grid()
        a = _aos(xyz)
        d, rk, sk = np.zeros((R, S)), np.zeros(R), np.zeros(S)
        self._call("tloam_place_describe", C.byref(cfg) if cfg is not None else None, _dp(a), len(a), _dp(d), _dp(rk), _dp(sk))
        return d, rk, sk

    def place_read_keyframes(self, first=0, count=None) -> dict:
        """keyframes [first, first + count) -> frames (m,), poses (m, 4, 4), ring_keys (m, R), sector_keys (m, S),
        descriptors (m, R, S)"""
        R, S = self._place_grid()
        first, m = _id_range(first, count, lambda: self.place_info()["n_keyframes"])
        fr, P = np.zeros(max(m, 1), np.int64), np.zeros((max(m, 1), 16))
        rk, sk, d = np.zeros((max(m, 1), R)), np.zeros((max(m, 1), S)), np.zeros((max(m, 1), R, S))
        self._call("tloam_place_read_keyframes", int(first), m, _lp(fr), _dp(P), _dp(rk), _dp(sk), _dp(d))
        return {"frames": fr[:m].copy(), "poses": P[:m].reshape(m, 4, 4).transpose(0, 2, 1).copy(), "ring_keys": rk[:m].copy(),
                "sector_keys": sk[:m].copy(), "descriptors": d[:m].copy()}

    def place_loops(self, first=0, count=None) -> list:
        """loop records [first, first + count) in the order they were found, as dicts"""
        first, m = _id_range(first, count, lambda: self.place_info()["n_loops"])
        buf = (PlaceLoop * max(m, 1))()
        self._call("tloam_place_read_loops", int(first), m, buf)
        return [buf[i].as_dict() for i in range(m)]

    # ---- loop verification: keyframe clouds and a two-stage TLS match
    def loop_configure(self, cfg: LoopConfig | None = None, **over):
        """loop verification on / off (default_loop_config(**over) when cfg is None); empties the keyframe database, its clouds
        and the constraints.  Kept across odometry_reset (which empties them too)."""
        self._configure(LoopConfig, "tloam_loop_configure", cfg, over)

    def loop_info(self) -> dict:
        """constraints, accepted ones, the points the keyframe clouds take and the arena's capacity"""
        return self._info(LoopInfo, "tloam_loop_get_info")

    def place_set_keyframe_clouds(self, keyframe, src=None, tgt=None):
        """a keyframe's clouds from the caller: src / tgt are four (n, 3) clouds by kind, or None to leave that side"""
        def side(clouds):
            if clouds is None:
                return None, None, []
            a = [_aos(x) for x in clouds]
            assert len(a) == 4
            return (dp * 4)(*[_dp(x) for x in a]), (C.c_size_t * 4)(*[len(x) for x in a]), a
        dp = C.POINTER(C.c_double)
        sp, sn, keep_s = side(src)
        tp, tn, keep_t = side(tgt)
        self._call("tloam_place_set_keyframe_clouds", int(keyframe), sp, sn, tp, tn)
        del keep_s, keep_t

    def place_read_keyframe_clouds(self, keyframe, side=None, kind=None):
        """one stored cloud (side 0 source / 1 target, kind TLOAM_KIND_*) as (n, 3); side None: [[4 source], [4 target]]"""
        if side is None:
            return [[self.place_read_keyframe_clouds(keyframe, s, k) for k in range(4)] for s in range(2)]
        n = C.c_size_t(0)
        self._call("tloam_place_read_keyframe_clouds", int(keyframe), int(side), int(kind), 0, C.byref(n), None)
        out = np.zeros((max(n.value, 1), 3))
        self._call("tloam_place_read_keyframe_clouds", int(keyframe), int(side), int(kind), n.value, C.byref(n), _dp(out))
        return out[: n.value].copy()

    def loop_verify_pending(self) -> int:
        """verifies every loop record not verified yet (one constraint each) -> how many"""
        n = C.c_int64(0)
        self._call("tloam_loop_verify_pending", C.byref(n))
        return int(n.value)

    def loop_verify_pair(self, query, match, init=None) -> dict:
        """one pair from the caller's initial guess (4x4; None: rigid_inverse(P_m) P_q); not appended"""
        M = None if init is None else _colmajor(init)
        return self._info(LoopConstraint, "tloam_loop_verify_pair", int(query), int(match), _dp(M))

    def loop_constraints(self, first=0, count=None) -> list:
        """constraints [first, first + count) as dicts"""
        first, m = _id_range(first, count, lambda: self.loop_info()["n_constraints"])
        buf = (LoopConstraint * max(m, 1))()
        self._call("tloam_loop_read_constraints", int(first), m, buf)
        return [buf[i].as_dict() for i in range(m)]

    # ---- pose-graph optimisation of the keyframes
    def graph_configure(self, cfg: GraphConfig | None = None, **over):
        """the context's graph configuration (default_graph_config(**over) when cfg is None); drops the corrected poses.  Kept
        across odometry_reset."""
        self._configure(GraphConfig, "tloam_graph_configure", cfg, over)

    @staticmethod
    def _graph_arrays(poses, i, j, Z, w):
        """-> (poses column-major (n, 4, 4), number of edges, the tloam_graph_edge array)"""
        P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1))
        Zc = np.asarray(Z, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1).reshape(-1, 16)
        wv = np.asarray(w, np.float64).reshape(-1, 6)
        m = len(Zc)
        edges = (GraphEdge * max(m, 1))()
        if m:
            rec = np.frombuffer(edges, dtype=np.dtype([("i", np.int64), ("j", np.int64), ("Z", np.float64, 16),
                                                       ("w", np.float64, 6)]), count=m)
            rec["i"], rec["j"], rec["Z"], rec["w"] = np.asarray(i, np.int64), np.asarray(j, np.int64), Zc, wv
        return P, m, edges

    def graph_solve(self, poses, i, j, Z, w, cfg: GraphConfig | None = None):
        """the caller's graph: poses (n, 4, 4); edges i, j (m,), Z (m, 4, 4), w (m, 6), the first n - 1 the chain ->
        (poses (n, 4, 4), info dict); cfg None: the context's configuration"""
        P, m, edges = self._graph_arrays(poses, i, j, Z, w)
        out = np.zeros_like(P)
        info = GraphInfo()
        self._call("tloam_graph_solve", C.byref(cfg) if cfg is not None else None, len(P), _dp(P), m, edges, _dp(out), C.byref(info))
        return out.transpose(0, 2, 1).copy(), info.as_dict()

    # ---- its robust mode: GNC-TLS on the loop edges
    def graph_robust_configure(self, cfg: GraphRobustConfig | None = None, **over):
        """the context's robust configuration (default_graph_robust_config(**over) when cfg is None: off unless enabled=1);
        drops the corrected poses.  Kept across odometry_reset."""
        self._configure(GraphRobustConfig, "tloam_graph_robust_configure", cfg, over)

    def graph_solve_robust(self, poses, i, j, Z, w, cfg: GraphConfig | None = None, rcfg: GraphRobustConfig | None = None):
        """graph_solve with the robust mode -> (poses (n, 4, 4), info dict of the last inner solve, robust info dict, the loop
        edges' scales (m - (n - 1),), their statistics r); cfg / rcfg None: the context's configurations"""
        P, m, edges = self._graph_arrays(poses, i, j, Z, w)
        nl = max(m - (len(P) - 1), 0)
        out = np.zeros_like(P)
        scale, chi2 = np.zeros(max(nl, 1)), np.zeros(max(nl, 1))
        info, rinfo = GraphInfo(), GraphRobustInfo()
        self._call("tloam_graph_solve_robust", C.byref(cfg) if cfg is not None else None,
                   C.byref(rcfg) if rcfg is not None else None, len(P), _dp(P), m, edges, _dp(out), C.byref(info), C.byref(rinfo),
                   _dp(scale), _dp(chi2))
        return out.transpose(0, 2, 1).copy(), info.as_dict(), rinfo.as_dict(), scale[:nl].copy(), chi2[:nl].copy()

    def graph_read_loop_scales(self, first=0, count=None):
        """the loop edges [first, first + count) of the last graph_optimize -> (constraint indices as loop_constraints numbers
        them, scales, statistics r); count None: all of them"""
        first, m = _id_range(first, count, lambda: getattr(self, "_graph_loops", 0))
        idx, scale, chi2 = np.zeros(max(m, 1), np.int64), np.zeros(max(m, 1)), np.zeros(max(m, 1))
        self._call("tloam_graph_read_loop_scales", int(first), m, _lp(idx), _dp(scale), _dp(chi2))
        return idx[:m].copy(), scale[:m].copy(), chi2[:m].copy()

    def graph_robust_info(self) -> dict:
        """tloam_graph_get_robust_info: the robust mode's report of the last graph_optimize"""
        return self._info(GraphRobustInfo, "tloam_graph_get_robust_info")

    def graph_optimize(self) -> dict:
        """optimises the context's graph (keyframe poses, odometry chain, accepted constraints) -> info dict"""
        info = GraphInfo()
        self._call("tloam_graph_optimize", C.byref(info))
        self._graph_n = int(info.n_nodes)   # (how many corrected poses graph_poses reads by default)
        self._graph_loops = int(info.n_loop_edges)
        return info.as_dict()

    def graph_poses(self, first=0, count=None):
        """corrected keyframe poses [first, first + count) of the last graph_optimize, (m, 4, 4); count None: all of them"""
        first, m = _id_range(first, count, lambda: getattr(self, "_graph_n", 0))
        out = np.zeros((max(m, 1), 16))
        self._call("tloam_graph_read_poses", int(first), m, _dp(out))
        return out[:m].reshape(m, 4, 4).transpose(0, 2, 1).copy()

    def graph_correct_pose(self, keyframe, pose):
        """P'_k rigid_inverse(P_k) pose for a pose taken near keyframe k (-1: the last corrected one)"""
        out = np.zeros(16)
        self._call("tloam_graph_correct_pose", int(keyframe), _dp(_colmajor(pose)), _dp(out))
        return out.reshape(4, 4).T.copy()

    # ---- the closed map: the keyframe clouds merged under corrected poses
    def closed_map_configure(self, cfg: ClosedMapConfig | None = None, **over):
        """the closed map's configuration (default_closed_map_config(**over) when cfg is None); empties it.  Kept across
        odometry_reset."""
        self._cmap_cfg = self._configure(ClosedMapConfig, "tloam_closed_map_configure", cfg, over)

    def closed_map_build(self, pose_source=1, poses=None) -> dict:
        """builds the closed map from every keyframe's stored clouds, replacing the previous one -> info dict.  pose_source 0: the
        stored keyframe poses, 1: the corrected poses of the last graph_optimize, 2: `poses` (K, 4, 4)"""
        P, n = None, 0
        if poses is not None:
            P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1))
            n = len(P)
        return self._info(ClosedMapInfo, "tloam_closed_map_build", int(pose_source), _dp(P), n)

    def closed_map_info(self) -> dict:
        return self._info(ClosedMapInfo, "tloam_closed_map_get_info")

    def closed_map_read(self, first=0, count=None):
        """voxels [first, first + count) in id order -> (centroids (m, 3) float64, counts (m,) int64); count None: to the end"""
        first, m = _id_range(first, count, lambda: self.closed_map_info()["n_voxels"])
        cen, cnt = np.zeros((max(m, 1), 3)), np.zeros(max(m, 1), np.int64)
        self._call("tloam_closed_map_read", int(first), m, _dp(cen), _lp(cnt))
        return cen[:m].copy(), cnt[:m].copy()

    def closed_map_read_box(self, lo, hi, min_count=1):
        """the voxels whose centroid lies in [lo, hi] (inclusive, every axis) with N >= min_count, in id order ->
        (centroids (m, 3), counts (m,))"""
        lo = np.ascontiguousarray(lo, dtype=np.float64).reshape(3)
        hi = np.ascontiguousarray(hi, dtype=np.float64).reshape(3)
        return self._read_box("tloam_closed_map_read_box", (_dp(lo), _dp(hi), int(min_count)), [(3, np.float64), (None, np.int64)])

    def closed_map_poses(self, first=0, count=None):
        """the poses keyframes [first, first + count) were built with, (m, 4, 4); count None: to the end"""
        first, m = _id_range(first, count, lambda: self.closed_map_info()["n_keyframes"])
        out = np.zeros((max(m, 1), 16))
        self._call("tloam_closed_map_read_poses", int(first), m, _dp(out))
        return out[:m].reshape(m, 4, 4).transpose(0, 2, 1).copy()

    # ---- the closed map extended in place by the keyframes added since its build
    def closed_map_extend(self, pose_source=0, poses=None) -> dict:
        """adds the keyframes [info.n_keyframes, n_kf) -- the ones added since the build, the load or the last extend -- to the
        built closed map in place, its surfels and its carve following -> info dict.  pose_source 0: their stored poses, 1: the
        build's rule (corrected poses), 2: `poses` (n_kf - K, 4, 4), of the new keyframes only"""
        P, n = None, 0
        if poses is not None:
            P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1))
            n = len(P)
        return self._info(ClosedMapExtendInfo, "tloam_closed_map_extend", int(pose_source), _dp(P), n)

    def closed_map_extend_info(self) -> dict:
        return self._info(ClosedMapExtendInfo, "tloam_closed_map_get_extend_info")

    # ---- the closed map's snapshot: out of this context, into a fresh one
    def closed_map_save(self, clouds=False) -> bytes:
        """the built closed map, its carve and surfels when they exist, the keyframe database and the configurations as one
        blob; clouds: also the keyframes' stored clouds, so that the loaded map can be built, carved and surfelled again"""
        flags = SNAPSHOT_CLOUDS if clouds else 0
        n = C.c_size_t(0)
        self._call("tloam_closed_map_save_size", flags, C.byref(n))
        buf = C.create_string_buffer(max(n.value, 1))
        self._call("tloam_closed_map_save", flags, buf, n.value, C.byref(n))
        return buf.raw[:n.value]

    def closed_map_load(self, blob) -> dict:
        """replaces this context's keyframes, loop constraints, corrected poses and closed map by the snapshot's -> what it
        held (closed_map_probe's dict).  A refused blob raises TloamHipError and leaves the context as it was"""
        blob = bytes(blob)
        info = ClosedMapSnapshotInfo()
        self._call("tloam_closed_map_load", blob, len(blob), C.byref(info))
        # (the keyframe getters size their outputs by the place configuration's layout, which is now the snapshot's)
        self._place_cfg = default_place_config(enabled=1, n_rings=int(info.n_rings), n_sectors=int(info.n_sectors))
        # (... and the frontier clusters' centroids are formed from the grid, which is now the snapshot's too)
        self._cmap_cfg = default_closed_map_config(voxel=float(info.voxel), origin=tuple(float(v) for v in info.origin))
        return info.as_dict()

    # ---- the carve of the closed map: per voxel, the rays that passed through it
    def closed_map_carve_configure(self, cfg: ClosedMapCarveConfig | None = None, **over):
        """the carve's configuration (default_closed_map_carve_config(**over) when cfg is None); drops the counts, not the closed
        map.  Kept across odometry_reset."""
        self._configure(ClosedMapCarveConfig, "tloam_closed_map_carve_configure", cfg, over)

    def closed_map_carve(self) -> dict:
        """counts, per voxel of the built closed map, the keyframe rays that passed through it -> info dict"""
        return self._info(ClosedMapCarveInfo, "tloam_closed_map_carve")

    def closed_map_carve_info(self) -> dict:
        return self._info(ClosedMapCarveInfo, "tloam_closed_map_get_carve_info")

    def closed_map_misses(self, first=0, count=None):
        """M of voxels [first, first + count) in id order, (m,) int64; count None: to the end"""
        first, m = _id_range(first, count, lambda: self.closed_map_info()["n_voxels"])
        out = np.zeros(max(m, 1), np.int64)
        self._call("tloam_closed_map_read_misses", int(first), m, _lp(out))
        return out[:m].copy()

    def closed_map_read_carved(self, lo=None, hi=None, min_count=1, min_miss=3, miss_ratio=1.0):
        """closed_map_read_box's voxels (lo and hi None: the whole map) without those seen through -- M >= min_miss and
        M > miss_ratio * N -- in id order -> (centroids (m, 3), counts (m,), misses (m,))"""
        lo, hi = _box(lo, hi)
        head = (_dp(lo), _dp(hi), int(min_count), int(min_miss), float(miss_ratio))
        return self._read_box("tloam_closed_map_read_carved", head, [(3, np.float64), (None, np.int64), (None, np.int64)])

    # ---- the surfels of the closed map: per voxel a normal and three variances
    def closed_map_surfel_configure(self, cfg: ClosedMapSurfelConfig | None = None, **over):
        """the surfels' configuration (default_closed_map_surfel_config(**over) when cfg is None); drops the surfels, not the
        closed map or the carve's counts.  Kept across odometry_reset."""
        self._configure(ClosedMapSurfelConfig, "tloam_closed_map_surfel_configure", cfg, over)

    def closed_map_surfels(self) -> dict:
        """gathers, per voxel of the built closed map, the second moments of its points and solves them -> info dict"""
        return self._info(ClosedMapSurfelInfo, "tloam_closed_map_surfels")

    def closed_map_surfel_info(self) -> dict:
        return self._info(ClosedMapSurfelInfo, "tloam_closed_map_get_surfel_info")

    def closed_map_moments(self, first=0, count=None):
        """the thirteen sums (Ns, R, S xx xy xz yy yz zz, W) of voxels [first, first + count) in id order, (m, 13) int64;
        count None: to the end"""
        first, m = _id_range(first, count, lambda: self.closed_map_info()["n_voxels"])
        out = np.zeros((max(m, 1), 13), np.int64)
        self._call("tloam_closed_map_read_moments", int(first), m, _lp(out))
        return out[:m].copy()

    def closed_map_read_surfels(self, first=0, count=None):
        """voxels [first, first + count) in id order -> (normals (m, 3), variances ascending (m, 3) in m^2, Ns (m,) int64);
        count None: to the end.  An unsolved voxel's normal and variances are zero"""
        first, m = _id_range(first, count, lambda: self.closed_map_info()["n_voxels"])
        nrm, ev, cnt = np.zeros((max(m, 1), 3)), np.zeros((max(m, 1), 3)), np.zeros(max(m, 1), np.int64)
        self._call("tloam_closed_map_read_surfels", int(first), m, _dp(nrm), _dp(ev), _lp(cnt))
        return nrm[:m].copy(), ev[:m].copy(), cnt[:m].copy()

    def closed_map_read_surfels_box(self, lo=None, hi=None, min_count=1, max_sigma=float("inf"), min_planarity=0.05):
        """closed_map_read_box's voxels (lo and hi None: the whole map) whose surfel is solved with ev2 > 0,
        ev0 <= max_sigma^2 and ev1 - ev0 >= min_planarity * ev2, in id order ->
        (centroids (m, 3), normals (m, 3), variances (m, 3), Ns (m,))"""
        lo, hi = _box(lo, hi)
        head = (_dp(lo), _dp(hi), int(min_count), float(max_sigma), float(min_planarity))
        return self._read_box("tloam_closed_map_read_surfels_box", head,
                              [(3, np.float64), (3, np.float64), (3, np.float64), (None, np.int64)])

    # ---- localisation of a scan in the closed map: point-to-plane Gauss-Newton on the surfels
    def closed_map_localise_configure(self, cfg: ClosedMapLocaliseConfig | None = None, **over):
        """the localisation's configuration (default_closed_map_localise_config(**over) when cfg is None).  Kept across
        odometry_reset; a refused configuration leaves the old one."""
        self._configure(ClosedMapLocaliseConfig, "tloam_closed_map_localise_configure", cfg, over)

    def closed_map_localise(self, points, prior):
        """the scan `points` (n, 3; sensor frame) registered against the closed map's surfels from the pose `prior` (4 x 4)
        -> (pose (4, 4), info dict).  A DEGENERATE status returns the prior"""
        pts = _aos(points)
        pr, out = _colmajor(prior), np.zeros(16)
        info = self._info(ClosedMapLocaliseInfo, "tloam_closed_map_localise", _dp(pts), len(pts), _dp(pr), _dp(out))
        return out.reshape(4, 4).T.copy(), info

    def closed_map_localise_log(self) -> list:
        """the executed iterations of the last closed_map_localise: dicts of pose (before the step), tau, cost, d, matched, used"""
        return self._read_list("tloam_closed_map_localise_log", ClosedMapLocaliseRecord)

    def closed_map_linearise(self, points, pose, tau) -> dict:
        """one sweep at `pose` (4 x 4) with truncation `tau`, no step -> dict(ids (n,) int32, -1 unmatched; residuals (n,);
        H (21,) upper triangle by rows; g (6,); cost; matched; used)"""
        pts = _aos(points)
        ids, res = np.zeros(max(len(pts), 1), np.int32), np.zeros(max(len(pts), 1))
        out, cnt = np.zeros(28), np.zeros(2, np.int64)
        self._call("tloam_closed_map_linearise", _dp(pts), len(pts), _dp(_colmajor(pose)), float(tau), _ip(ids), _dp(res),
                   _dp(out), _lp(cnt))
        return {"ids": ids[: len(pts)].copy(), "residuals": res[: len(pts)].copy(), "H": out[:21].copy(), "g": out[21:27].copy(),
                "cost": float(out[27]), "matched": int(cnt[0]), "used": int(cnt[1])}

    # ---- several hypotheses of one scan, and relocalisation without a prior
    def closed_map_localise_batch(self, points, priors):
        """the scan `points` registered from every pose of `priors` (B, 4, 4; B in 1 .. 32) in one set of launches
        -> (poses (B, 4, 4), [info dict] * B, best).  Hypothesis h has the bits of closed_map_localise(points, priors[h]);
        best is -1 when every hypothesis is DEGENERATE"""
        pts = _aos(points)
        priors = np.asarray(priors, np.float64)
        if priors.ndim != 3 or priors.shape[1:] != (4, 4):
            raise ValueError("priors: (B, 4, 4)")
        B = len(priors)
        pr = np.ascontiguousarray(priors.transpose(0, 2, 1)).reshape(-1)   # column-major, hypothesis by hypothesis
        out = np.zeros(16 * max(B, 1))
        infos = (ClosedMapLocaliseInfo * max(B, 1))()
        best = C.c_int32(-1)
        self._call("tloam_closed_map_localise_batch", _dp(pts), len(pts), _dp(pr), B, _dp(out), infos, C.byref(best))
        poses = out[: 16 * B].reshape(B, 4, 4).transpose(0, 2, 1).copy()
        return poses, [infos[h].as_dict() for h in range(B)], int(best.value)

    def closed_map_localise_batch_log(self, h) -> list:
        """the executed iterations of hypothesis h of the last closed_map_localise_batch (or closed_map_relocalise)"""
        return self._read_list("tloam_closed_map_localise_batch_log", ClosedMapLocaliseRecord, int(h))

    def closed_map_relocalise_configure(self, cfg: ClosedMapRelocaliseConfig | None = None, **over):
        """the relocalisation's configuration (default_closed_map_relocalise_config(**over) when cfg is None).  Kept across
        odometry_reset; a refused configuration leaves the old one."""
        self._configure(ClosedMapRelocaliseConfig, "tloam_closed_map_relocalise_configure", cfg, over)

    def closed_map_relocalise(self, points):
        """the scan `points` (n, 3; sensor frame) localised in the closed map without a prior: place recognition's candidates,
        a hypothesis from each, the batched localiser, the pick -> (pose (4, 4) or None when NOT_FOUND, info dict)"""
        pts = _aos(points)
        out = np.zeros(16)
        info = ClosedMapRelocaliseInfo()
        self._call("tloam_closed_map_relocalise", _dp(pts), len(pts), _dp(out), C.byref(info))
        pose = out.reshape(4, 4).T.copy() if info.status == RELOCALISE_FOUND else None
        return pose, info.as_dict()

    def closed_map_relocalise_hypotheses(self) -> list:
        """the hypotheses of the last closed_map_relocalise, in candidate order: dicts of keyframe, shift, skipped, dist, yaw,
        prior, pose and the localise info"""
        return self._read_list("tloam_closed_map_relocalise_hypotheses", ClosedMapRelocaliseHypothesis)

    # ---- a scan diffed against the closed map: new points, voxels seen through
    def closed_map_diff_configure(self, cfg: ClosedMapDiffConfig | None = None, **over):
        """the diff's configuration (default_closed_map_diff_config(**over) when cfg is None); drops the counts, not the closed
        map.  Kept across odometry_reset; a refused configuration leaves the old one."""
        self._configure(ClosedMapDiffConfig, "tloam_closed_map_diff_configure", cfg, over)

    def closed_map_diff(self, points, pose, accumulate=False, want_ids=False):
        """the scan `points` (n, 3; sensor frame) at `pose` (4 x 4) against the closed map -> (labels (n,) uint8: DIFF_INVALID,
        DIFF_SURFACE, DIFF_OCCUPIED, DIFF_NEW; ids (n,) int32 of the voxel that explained each point, -1 for none, or None
        without want_ids; info dict).  accumulate: the per-voxel counts are added to the stored ones instead of replacing them"""
        pts = _aos(points)
        labels, ids, cut = _per_point(len(pts), want_ids)
        info = self._info(ClosedMapDiffInfo, "tloam_closed_map_diff", _dp(pts), len(pts), _dp(_colmajor(pose)),
                          DIFF_ACCUMULATE if accumulate else 0, _u8p(labels), _ip(ids))
        return cut(labels), cut(ids), info

    def closed_map_diff_info(self) -> dict:
        return self._info(ClosedMapDiffInfo, "tloam_closed_map_get_diff_info")

    def closed_map_diff_counts(self, first=0, count=None):
        """through and hits of voxels [first, first + count) in id order -> ((m,) int64, (m,) int64); count None: to the end"""
        first, m = _id_range(first, count, lambda: self.closed_map_info()["n_voxels"])
        through, hits = np.zeros(max(m, 1), np.int64), np.zeros(max(m, 1), np.int64)
        self._call("tloam_closed_map_read_diff", int(first), m, _lp(through), _lp(hits))
        return through[:m].copy(), hits[:m].copy()

    def closed_map_read_gone(self, lo=None, hi=None, min_through=3, gone_ratio=1.0):
        """the voxels (lo and hi None: of the whole map; else with their centroid in [lo, hi]) the diffed scans saw through --
        through >= min_through and through > gone_ratio * hits -- in id order ->
        (centroids (m, 3), counts (m,), through (m,), hits (m,))"""
        lo, hi = _box(lo, hi)
        head = (_dp(lo), _dp(hi), int(min_through), float(gone_ratio))
        return self._read_box("tloam_closed_map_read_gone", head,
                              [(3, np.float64), (None, np.int64), (None, np.int64), (None, np.int64)])

    # ---- the closed map ray-cast: predicted ranges along segments from a pose
    def closed_map_raycast_configure(self, cfg: ClosedMapRaycastConfig | None = None, **over):
        """the ray-cast's configuration (default_closed_map_raycast_config(**over) when cfg is None); clears the last info, not
        the closed map.  Kept across odometry_reset; a refused configuration leaves the old one."""
        self._configure(ClosedMapRaycastConfig, "tloam_closed_map_raycast_configure", cfg, over)

    def closed_map_raycast(self, ends, pose, want_ids=False):
        """the segments from `pose`'s translation to `ends` (n, 3; sensor frame) under `pose` (4 x 4) through the closed map ->
        (status (n,) uint8: RAYCAST_SKIPPED, RAYCAST_MISS, RAYCAST_HIT_CENTROID, RAYCAST_HIT_PLANE; ranges (n,) float64, metres
        along the segment to the first hit, -1.0 without one; ids (n,) int32 of the voxel hit, -1 for none, or None without
        want_ids; info dict)"""
        e = _aos(ends)
        status, ids, cut = _per_point(len(e), want_ids)
        ranges = np.zeros(max(len(e), 1), np.float64)
        info = self._info(ClosedMapRaycastInfo, "tloam_closed_map_raycast", _dp(e), len(e), _dp(_colmajor(pose)), _u8p(status),
                          _dp(ranges), _ip(ids))
        return cut(status), cut(ranges), cut(ids), info

    def closed_map_raycast_info(self) -> dict:
        return self._info(ClosedMapRaycastInfo, "tloam_closed_map_get_raycast_info")

    # ---- free space for the closed map: an occupancy grid from the rays
    def closed_map_free_configure(self, cfg: FreeConfig | None = None, **over):
        """the free space's configuration (default_closed_map_free_config(**over) when cfg is None); drops the grid, not the
        closed map.  Kept across odometry_reset; a refused configuration leaves the old one."""
        self._configure(FreeConfig, "tloam_closed_map_free_configure", cfg, over)

    def closed_map_free_info(self) -> dict:
        return self._info(FreeInfo, "tloam_closed_map_get_free_info")

    def closed_map_free_reset(self, lo_cells=None, hi_cells=None) -> dict:
        """allocates and zeroes the grid over the cells [lo_cells, hi_cells] (inclusive, rounded out to bricks); both None: the
        auto box around the closed map's poses -> info dict"""
        if (lo_cells is None) != (hi_cells is None):
            raise ValueError("lo_cells and hi_cells go together")
        lo = hi = None
        if lo_cells is not None:
            lo = np.ascontiguousarray(lo_cells, dtype=np.int64).reshape(3)
            hi = np.ascontiguousarray(hi_cells, dtype=np.int64).reshape(3)
        self._call("tloam_closed_map_free_reset", _lp(lo), _lp(hi))
        return self.closed_map_free_info()

    def closed_map_free_add_keyframes(self) -> dict:
        """walks the rays of the keyframes the grid has not seen (all of the map's after a reset, the new ones after an extend)
        -> info dict"""
        return self._info(FreeInfo, "tloam_closed_map_free_add_keyframes")

    def closed_map_free_add_scan(self, points, pose) -> dict:
        """walks the rays of the scan `points` (n, 3; sensor frame) at `pose` (4 x 4) -> info dict"""
        pts = _aos(points)
        return self._info(FreeInfo, "tloam_closed_map_free_add_scan", _dp(pts), len(pts), _dp(_colmajor(pose)))

    def closed_map_free_build(self, lo_cells=None, hi_cells=None) -> dict:
        """closed_map_free_reset, then closed_map_free_add_keyframes -> info dict"""
        self.closed_map_free_reset(lo_cells, hi_cells)
        return self.closed_map_free_add_keyframes()

    def closed_map_free_words(self, first=0, count=None):
        """the grid's words [first, first + count) -> (m,) uint64; count None: to the end"""
        def total():
            nb = self.closed_map_free_info()["n_bricks"]
            return nb[0] * nb[1] * nb[2]
        first, m = _id_range(first, count, total)
        words = np.zeros(max(m, 1), np.uint64)
        self._call("tloam_closed_map_read_free_words", int(first), m, words.ctypes.data_as(C.POINTER(C.c_uint64)))
        return words[:m].copy()

    def closed_map_occupancy(self, points, pose=None, want_ids=False):
        """the state of `points` (n, 3; in the map frame, or with `pose` (4 x 4) in its sensor frame) -> (states (n,) uint8:
        OCCUPANCY_INVALID, OCCUPANCY_UNKNOWN, OCCUPANCY_FREE, OCCUPANCY_OCCUPIED; ids (n,) int32 of the voxel of an OCCUPIED
        point, -1 otherwise, or None without want_ids; counts (4,) int64 of points per state)"""
        pts = _aos(points)
        state, ids, cut = _per_point(len(pts), want_ids)
        counts = np.zeros(4, np.int64)
        self._call("tloam_closed_map_occupancy", _dp(pts), len(pts), None if pose is None else _dp(_colmajor(pose)), _u8p(state),
                   _ip(ids), _lp(counts))
        return cut(state), cut(ids), counts

    def closed_map_free_cells(self, lo=None, hi=None):
        """the centres (m, 3) of the FREE cells (lo and hi None: of the whole grid; else with their centre in [lo, hi]), brick
        index ascending, then bit ascending"""
        lo, hi = _box(lo, hi)
        return self._read_box("tloam_closed_map_read_free", (_dp(lo), _dp(hi)), [(3, np.float64)])[0]

    def closed_map_free_columns(self, z_lo, z_hi, min_free=1):
        """the navigation grid (ny, nx) uint8 over the box's x-y footprint for the band of cells between heights z_lo and z_hi:
        OCCUPANCY_OCCUPIED, OCCUPANCY_FREE (at least min_free free band cells) or OCCUPANCY_UNKNOWN per column"""
        info = self.closed_map_free_info()
        nx, ny = C.c_size_t(0), C.c_size_t(0)
        out = np.zeros(max(16 * info["n_bricks"][0] * info["n_bricks"][1], 1), np.uint8)
        self._call("tloam_closed_map_free_columns", float(z_lo), float(z_hi), int(min_free), _u8p(out), len(out), C.byref(nx),
                   C.byref(ny))
        return out[: nx.value * ny.value].reshape(ny.value, nx.value).copy()

    # ---- clearance for the closed map: a truncated distance field over the free-space box, and path checks
    def closed_map_clearance_configure(self, cfg: ClearanceConfig | None = None, **over):
        """the clearance's configuration (default_closed_map_clearance_config(**over) when cfg is None); drops the field, not the
        free-space grid.  Kept across odometry_reset; a refused configuration leaves the old one."""
        self._configure(ClearanceConfig, "tloam_closed_map_clearance_configure", cfg, over)

    def closed_map_clearance_build(self) -> dict:
        """builds the field over the free-space grid's box from the occupancy as it stands -> info dict"""
        return self._info(ClearanceInfo, "tloam_closed_map_clearance_build")

    def closed_map_clearance_info(self) -> dict:
        return self._info(ClearanceInfo, "tloam_closed_map_get_clearance_info")

    def closed_map_clearance_field(self):
        """the whole field -> (nz, ny, nx) uint16: d2 in cells, CLEARANCE_BEYOND beyond radius_cells"""
        nx, ny, nz = self.closed_map_clearance_info()["n_cells"]
        d2 = np.zeros(max(nx * ny * nz, 1), np.uint16)
        self._call("tloam_closed_map_read_clearance", 0, nx * ny * nz, _u16p(d2))
        return d2[: nx * ny * nz].reshape(nz, ny, nx).copy()

    def closed_map_clearance_points(self, points, pose=None, want_distance=True):
        """the clearance of `points` (n, 3; in the map frame, or with `pose` (4 x 4) in its sensor frame) -> (states (n,) uint8 as
        closed_map_occupancy, d2 (n,) uint16, distance (n,) float64 = voxel * sqrt(d2) -- inf for CLEARANCE_BEYOND, NaN for
        CLEARANCE_OUTSIDE -- or None without want_distance, counts (4,) int64 of points per state)"""
        pts = _aos(points)
        n = len(pts)
        state, _, cut = _per_point(n, False)
        d2 = np.zeros(max(n, 1), np.uint16)
        dist = np.zeros(max(n, 1), np.float64) if want_distance else None
        counts = np.zeros(4, np.int64)
        self._call("tloam_closed_map_clearance_points", _dp(pts), n, None if pose is None else _dp(_colmajor(pose)), _u8p(state),
                   _u16p(d2), _dp(dist), _lp(counts))
        return cut(state), cut(d2), cut(dist), counts

    def closed_map_clearance_segments(self, starts, ends, radius, pose=None):
        """is each segment starts[i] -> ends[i] ((n, 3) each; map frame, or the sensor frame of `pose`) clear for a body of
        `radius` metres? -> (status (n,) uint8: CLEARANCE_SKIPPED, _CLEAR, _BLOCKED, _LEFT_BOX; min_d2 (n,) uint16 over the cells
        walked; t_block (n,) float64, the parameter along the segment where the walk stopped, -1 when it did not; counts (4,)
        int64 of segments per status).  radius 0 never blocks: min_d2 is then the path's clearance."""
        a, b = _aos(starts), _aos(ends)
        if len(a) != len(b):
            raise ValueError(f"{len(a)} starts, {len(b)} ends")
        n = len(a)
        status, _, cut = _per_point(n, False)
        d2 = np.zeros(max(n, 1), np.uint16)
        t = np.zeros(max(n, 1), np.float64)
        counts = np.zeros(4, np.int64)
        self._call("tloam_closed_map_clearance_segments", _dp(a), _dp(b), n, None if pose is None else _dp(_colmajor(pose)),
                   float(radius), _u8p(status), _u16p(d2), _dp(t), _lp(counts))
        return cut(status), cut(d2), cut(t), counts

    def closed_map_clearance_columns(self, z_lo, z_hi, min_free=1):
        """the 2-D field over closed_map_free_columns' grid -> (states (ny, nx) uint8, d2 (ny, nx) uint16 in cells to the nearest
        obstacle column); computed per call from the free-space grid"""
        nb = self.closed_map_free_info()["n_bricks"]
        nx, ny = C.c_size_t(0), C.c_size_t(0)
        m = max(16 * nb[0] * nb[1], 1)
        state, d2 = np.zeros(m, np.uint8), np.zeros(m, np.uint16)
        self._call("tloam_closed_map_clearance_columns", float(z_lo), float(z_hi), int(min_free), _u8p(state), _u16p(d2), m,
                   C.byref(nx), C.byref(ny))
        shape = (ny.value, nx.value)
        return state[: shape[0] * shape[1]].reshape(shape).copy(), d2[: shape[0] * shape[1]].reshape(shape).copy()

    # ---- the route through the closed map: a cost-to-go field from goals over the clearance field, and paths
    def closed_map_route_configure(self, cfg: RouteConfig | None = None, **over):
        """the route's configuration (default_closed_map_route_config(**over) when cfg is None); drops the route field only.
        Kept across odometry_reset; a refused configuration leaves the old one."""
        self._configure(RouteConfig, "tloam_closed_map_route_configure", cfg, over)

    def closed_map_route_build(self, goals, radius=0.0, pose=None) -> dict:
        """builds the cost-to-go field towards `goals` ((n, 3); map frame, or the sensor frame of `pose`) over the cells a body
        of `radius` metres may occupy -> info dict (its ROUTE_DIAGNOSTICS fields may differ from run to run)"""
        pts = _aos(goals)
        info = RouteInfo()
        self._call("tloam_closed_map_route_build", _dp(pts), len(pts), None if pose is None else _dp(_colmajor(pose)),
                   float(radius), C.byref(info))
        return info.as_dict()

    def closed_map_route_info(self) -> dict:
        return self._info(RouteInfo, "tloam_closed_map_get_route_info")

    def closed_map_route_field(self):
        """the whole field -> (nz, ny, nx) uint32: the 3-4-5 chamfer cost to the nearest accepted goal, ROUTE_UNREACHED,
        ROUTE_BLOCKED; voxel * cost / 3.0 is metres"""
        nx, ny, nz = self.closed_map_route_info()["n_cells"]
        cost = np.zeros(max(nx * ny * nz, 1), np.uint32)
        self._call("tloam_closed_map_read_route", 0, nx * ny * nz, _u32p(cost))
        return cost[: nx * ny * nz].reshape(nz, ny, nx).copy()

    def closed_map_route_points(self, points, pose=None, want_distance=True):
        """the cost-to-go of `points` (n, 3; map frame, or the sensor frame of `pose`) -> (cost (n,) uint32 -- ROUTE_OUTSIDE for a
        cell outside the box or an invalid point --, distance (n,) float64 = voxel * cost / 3.0 -- inf for ROUTE_UNREACHED, NaN
        for ROUTE_BLOCKED and ROUTE_OUTSIDE -- or None without want_distance, counts (4,) int64: reached, unreached, blocked,
        outside)"""
        pts = _aos(points)
        n = len(pts)
        cost = np.zeros(max(n, 1), np.uint32)
        dist = np.zeros(max(n, 1), np.float64) if want_distance else None
        counts = np.zeros(4, np.int64)
        self._call("tloam_closed_map_route_points", _dp(pts), n, None if pose is None else _dp(_colmajor(pose)), _u32p(cost),
                   _dp(dist), _lp(counts))
        return cost[:n].copy(), None if dist is None else dist[:n].copy(), counts

    def closed_map_route_paths(self, starts, max_cells, pose=None):
        """a path per start ((n, 3); map frame, or the sensor frame of `pose`) descended from the field -> (status (n,) uint8:
        ROUTE_PATH_*; n_cells (n,) int32 waypoints written; cost (n,) uint32 of the start's cell; centres (n, max_cells, 3)
        float64, the cell centres, zero past n_cells).  A whole path has at most cost // 3 + 1 cells."""
        pts = _aos(starts)
        n, m = len(pts), int(max_cells)
        status, _, cut = _per_point(n, False)
        cells, cost = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint32)
        centres = np.zeros((max(n, 1), max(m, 1), 3), np.float64)
        self._call("tloam_closed_map_route_paths", _dp(pts), n, None if pose is None else _dp(_colmajor(pose)), m, _u8p(status),
                   _ip(cells), _u32p(cost), _dp(centres))
        return cut(status), cut(cells), cut(cost), centres[:n].copy()

    def closed_map_route_columns(self, z_lo, z_hi, goals, radius=0.0, min_free=1, pose=None):
        """the 2-D cost-to-go over closed_map_clearance_columns' layer, 8-connected with weights 3 and 4, goals placed by x and y
        -> (states (ny, nx) uint8, d2 (ny, nx) uint16, cost (ny, nx) uint32, info dict); computed per call, not stored"""
        pts = _aos(goals)
        nb = self.closed_map_free_info()["n_bricks"]
        nx, ny = C.c_size_t(0), C.c_size_t(0)
        m = max(16 * nb[0] * nb[1], 1)
        state, d2, cost = np.zeros(m, np.uint8), np.zeros(m, np.uint16), np.zeros(m, np.uint32)
        info = RouteInfo()
        self._call("tloam_closed_map_route_columns", float(z_lo), float(z_hi), int(min_free), _dp(pts), len(pts),
                   None if pose is None else _dp(_colmajor(pose)), float(radius), _u8p(state), _u16p(d2), _u32p(cost), m,
                   C.byref(nx), C.byref(ny), C.byref(info))
        shape = (ny.value, nx.value)
        k = shape[0] * shape[1]
        return state[:k].reshape(shape).copy(), d2[:k].reshape(shape).copy(), cost[:k].reshape(shape).copy(), info.as_dict()

    # ---- the frontiers of the closed map: where free space meets the unknown, clustered
    def closed_map_frontier_configure(self, cfg: FrontierConfig | None = None, **over):
        """the frontiers' configuration (default_closed_map_frontier_config(**over) when cfg is None); drops the frontier field
        only.  Kept across odometry_reset; a refused configuration leaves the old one."""
        self._configure(FrontierConfig, "tloam_closed_map_frontier_configure", cfg, over)

    def closed_map_frontier_build(self) -> dict:
        """labels the frontier cells of the free-space grid's box by cluster and gathers the clusters -> info dict (its
        FRONTIER_DIAGNOSTICS fields may differ from run to run)"""
        return self._info(FrontierInfo, "tloam_closed_map_frontier_build")

    def closed_map_frontier_info(self) -> dict:
        return self._info(FrontierInfo, "tloam_closed_map_get_frontier_info")

    def closed_map_frontier_field(self):
        """the whole field -> (nz, ny, nx) uint32: a frontier cell's cluster root, else FRONTIER_FREE, FRONTIER_UNKNOWN or
        FRONTIER_OCCUPIED"""
        nx, ny, nz = self.closed_map_frontier_info()["n_cells"]
        label = np.zeros(max(nx * ny * nz, 1), np.uint32)
        self._call("tloam_closed_map_read_frontier", 0, nx * ny * nz, _u32p(label))
        return label[: nx * ny * nz].reshape(nz, ny, nx).copy()

    def _probe_count(self, name, *args):
        """the first of a capacity-convention getter's two calls: capacity 0 and no outputs -> the count (a short capacity, -1,
        with n > 0 is its answer)"""
        n = C.c_size_t(0)
        rc = getattr(self.L, name)(self.h, *args, C.byref(n))
        if rc not in (0, -1) or (rc == -1 and n.value == 0):
            self._check(rc, name)
        return n.value

    def _frontier_centroids(self, rec, box_lo):
        """o + (lo_cells + sum / cells + 0.5) * v per axis, in double, in that order"""
        cfg = getattr(self, "_cmap_cfg", None) or default_closed_map_config()
        o, v = np.array(list(cfg.origin), np.float64), np.float64(cfg.voxel)
        mean = rec["sum"].astype(np.float64) / rec["cells"].astype(np.float64)[:, None]
        return o + ((np.asarray(box_lo, np.int64).astype(np.float64) + mean) + 0.5) * v

    def closed_map_frontier_clusters(self):
        """the kept clusters in ascending root -> (records (k,) of FRONTIER_CLUSTER_DTYPE, centroids (k, 3) float64)"""
        m = self._probe_count("tloam_closed_map_frontier_clusters", 0, None)
        rec = np.zeros(max(m, 1), FRONTIER_CLUSTER_DTYPE)
        if m:
            n = C.c_size_t(0)
            self._call("tloam_closed_map_frontier_clusters", m, rec.ctypes.data, C.byref(n))
        rec = rec[:m].copy()
        return rec, self._frontier_centroids(rec, self.closed_map_frontier_info()["lo_cells"])

    def closed_map_frontier_cells(self, root=FRONTIER_ALL):
        """the frontier cells of the kept cluster of root `root` (FRONTIER_ALL: of every kept cluster), ascending in linear index
        -> (centres (m, 3) float64, roots (m,) uint32); a root that is no kept cluster's gives none"""
        m = self._probe_count("tloam_closed_map_read_frontier_cells", int(root), 0, None, None)
        cen, roots = np.zeros((max(m, 1), 3), np.float64), np.zeros(max(m, 1), np.uint32)
        if m:
            n = C.c_size_t(0)
            self._call("tloam_closed_map_read_frontier_cells", int(root), m, _dp(cen), _u32p(roots), C.byref(n))
        return cen[:m].copy(), roots[:m].copy()

    def closed_map_frontier_points(self, points, pose=None):
        """the frontier field at `points` (n, 3; map frame, or the sensor frame of `pose`) -> (label (n,) uint32 --
        FRONTIER_OUTSIDE for a cell outside the box or an invalid point --, cluster (n,) int32: the index in the kept list or -1,
        counts (5,) int64: frontier, free, unknown, occupied, outside)"""
        pts = _aos(points)
        n = len(pts)
        label, cluster = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.int32)
        counts = np.zeros(5, np.int64)
        self._call("tloam_closed_map_frontier_points", _dp(pts), n, None if pose is None else _dp(_colmajor(pose)), _u32p(label),
                   _ip(cluster), _lp(counts))
        return label[:n].copy(), cluster[:n].copy(), counts

    def closed_map_frontier_costs(self):
        """the join with the built route field -> (cost (k,) uint32 per kept cluster: the least route cost within `reach` cells
        of its cells, ROUTE_UNREACHED without one; approach (k, 3) float64: the centre of that cell, NaN without one).  A route
        built from the robot's cell as the one goal gives the robot's cost to every cluster: the route's moves are symmetric."""
        m = self._probe_count("tloam_closed_map_frontier_costs", 0, None, None)
        cost, approach = np.zeros(max(m, 1), np.uint32), np.zeros((max(m, 1), 3), np.float64)
        if m:
            n = C.c_size_t(0)
            self._call("tloam_closed_map_frontier_costs", m, _u32p(cost), _dp(approach), C.byref(n))
        return cost[:m].copy(), approach[:m].copy()

    def closed_map_frontier_columns(self, z_lo, z_hi, min_free=1):
        """the 2-D frontiers over closed_map_free_columns' layer, 4 face neighbours and 8-connectivity -> (label (ny, nx) uint32,
        kept records, centroids (k, 3) -- their z the box's lowest layer of cells --, info dict); computed per call, not stored"""
        nb = self.closed_map_free_info()["n_bricks"]
        nx, ny = 4 * nb[0], 4 * nb[1]
        label = np.zeros(max(nx * ny, 1), np.uint32)
        info, n = FrontierInfo(), C.c_size_t(0)
        args = (float(z_lo), float(z_hi), int(min_free))
        rc = self.L.tloam_closed_map_frontier_columns(self.h, *args, _u32p(label), 0, None, C.byref(n), C.byref(info))
        if rc not in (0, -1) or (rc == -1 and n.value == 0):
            self._check(rc, "tloam_closed_map_frontier_columns")
        m = n.value
        rec = np.zeros(max(m, 1), FRONTIER_CLUSTER_DTYPE)
        if m:
            self._call("tloam_closed_map_frontier_columns", *args, _u32p(label), m, rec.ctypes.data, C.byref(n), C.byref(info))
        rec = rec[:m].copy()
        return label[: nx * ny].reshape(ny, nx).copy(), rec, self._frontier_centroids(rec, info.as_dict()["lo_cells"]), info.as_dict()

    # ---- the view gain of the closed map: the unknown cells seen from candidate poses
    def closed_map_view_configure(self, cfg: ViewConfig | None = None, **over):
        """the view gain's configuration (default_closed_map_view_config(**over) when cfg is None); clears the last info only.
        Kept across odometry_reset; a refused configuration leaves the old one."""
        self._configure(ViewConfig, "tloam_closed_map_view_configure", cfg, over)

    def closed_map_view_gain(self, poses, ends):
        """the gain of the views at `poses` ((v, 4, 4) or one 4 x 4) under the shared segment ends `ends` ((r, 3), sensor frame)
        against the built frontier field -> records (v,) of VIEW_GAIN_DTYPE: `unknown_cells` is the gain, the distinct UNKNOWN
        cells the view's rays cross before an OCCUPIED cell or the box stops them"""
        P = np.asarray(poses, np.float64).reshape(-1, 4, 4)
        flat = np.ascontiguousarray(P.transpose(0, 2, 1)).reshape(-1)
        e = _aos(ends)
        rec = np.zeros(max(len(P), 1), VIEW_GAIN_DTYPE)
        self._call("tloam_closed_map_view_gain", _dp(flat), len(P), _dp(e), len(e), rec.ctypes.data, None)
        return rec[: len(P)].copy()

    def closed_map_view_cells(self, pose, ends):
        """one view's seen cells -> (centres (m, 3) float64 of the distinct UNKNOWN cells, ascending in window bit index, the
        view's record (1,) of VIEW_GAIN_DTYPE)"""
        flat, e = _colmajor(pose), _aos(ends)
        rec = np.zeros(1, VIEW_GAIN_DTYPE)
        n = C.c_size_t(0)
        rc = self.L.tloam_closed_map_view_cells(self.h, _dp(flat), _dp(e), len(e), 0, None, C.byref(n), rec.ctypes.data)
        if rc not in (0, -1) or (rc == -1 and n.value == 0):
            self._check(rc, "tloam_closed_map_view_cells")
        m = n.value
        cen = np.zeros((max(m, 1), 3), np.float64)
        if m:
            self._call("tloam_closed_map_view_cells", _dp(flat), _dp(e), len(e), m, _dp(cen), C.byref(n), rec.ctypes.data)
        return cen[:m].copy(), rec

    def closed_map_frontier_gains(self, ends):
        """the explorer's one call: per kept cluster the view gain at its approach point (identity rotation) beside
        closed_map_frontier_costs' cost and approach point -> (records (k,) of VIEW_GAIN_DTYPE, cost (k,) uint32, approach (k, 3)
        float64); a cluster without an approach point has every ray skipped"""
        e = _aos(ends)
        m = self._probe_count("tloam_closed_map_frontier_gains", _dp(e), len(e), 0, None, None, None)
        rec, cost, approach = np.zeros(max(m, 1), VIEW_GAIN_DTYPE), np.zeros(max(m, 1), np.uint32), np.zeros((max(m, 1), 3), np.float64)
        if m:
            n = C.c_size_t(0)
            self._call("tloam_closed_map_frontier_gains", _dp(e), len(e), m, rec.ctypes.data, _u32p(cost), _dp(approach), C.byref(n))
        return rec[:m].copy(), cost[:m].copy(), approach[:m].copy()

    def closed_map_view_info(self) -> dict:
        """of the last view call (its VIEW_DIAGNOSTICS fields depend on the form that ran); all zero when there has been none
        since the frontier field was last dropped"""
        return self._info(ViewInfo, "tloam_closed_map_get_view_info")

    def fitness(self):
        f, r = C.c_double(0), C.c_double(0)

        rc = self.L.tloam_fitness(self.h, C.byref(f), C.byref(r))
        return rc, f.value, r.value

    def get_correspondences(self, kind, capacity=None):
        cap = int(capacity or max(self._n.get(("s", kind), 0), self._n.get(("c", kind), 0), 1))
        n = C.c_size_t(0)
        idx = np.zeros(cap, np.int32); a = np.zeros((cap, 3)); b = np.zeros((cap, 3))
        d = np.zeros(cap); w = np.zeros(cap); cost = np.zeros(cap)
        self._call("tloam_get_correspondences", int(kind), cap, C.byref(n), _ip(idx), _dp(a), _dp(b), _dp(d), _dp(w), _dp(cost))
        m = n.value
        return dict(idx=idx[:m], a=a[:m], b=b[:m], d=d[:m], w=w[:m], cost=cost[:m])

    def get_weights(self, kind):
        cap = max(self._n.get(("s", kind), 0), 1)
        n = C.c_size_t(0)
        w = np.zeros(cap)
        self._call("tloam_get_weights", int(kind), cap, C.byref(n), _dp(w))
        return w[:n.value]

    def knn(self, kind, queries, radius, k):
        q = _aos(queries)
        idx = np.zeros((len(q), k), np.int32); d2 = np.zeros((len(q), k)); cnt = np.zeros(len(q), np.int32)
        self._call("tloam_knn", int(kind), _dp(q), len(q), float(radius), int(k), _ip(idx), _dp(d2), _ip(cnt))
        return idx, d2, cnt

    def set_correspondences(self, res_type, p, a, b=None, d=None, w=None):
        p = _aos(p); a = _aos(a)
        b = None if b is None else _aos(b)
        d = None if d is None else np.ascontiguousarray(d, float)
        w = np.ones(len(p)) if w is None else np.ascontiguousarray(w, float)
        kind = {RES_PLANE: KIND_PLANAR, RES_LINE: KIND_EDGE, RES_POINT: KIND_SPHERE}[res_type]
        self._n[("c", kind)] = len(p)
        return self._call("tloam_set_correspondences", int(res_type), len(p), _dp(p), _dp(a), _dp(b), _dp(d), _dp(w))

    def accumulate(self, se3):
        x = np.ascontiguousarray(se3, float)
        H = np.zeros(36); g = np.zeros(6); cost = C.c_double(0)
        self._call("tloam_accumulate", _dp(x), _dp(H), _dp(g), C.byref(cost))
        return H.reshape(6, 6), g, cost.value

    def get_normal_equations(self):
        """(H 6x6, g, cost) the minimiser held at the accepted iterate when its last Solve returned."""
        H = np.zeros(36); g = np.zeros(6); cost = C.c_double(0)
        self._call("tloam_get_normal_equations", _dp(H), _dp(g), C.byref(cost))
        return H.reshape(6, 6), g, cost.value

    def get_costs(self, res_type):
        kind = {RES_PLANE: KIND_PLANAR, RES_LINE: KIND_EDGE, RES_POINT: KIND_SPHERE}[res_type]
        cap = max(self._n.get(("c", kind), 0), 1)
        n = C.c_size_t(0)
        c = np.zeros(cap)
        self._call("tloam_get_costs", int(res_type), cap, C.byref(n), _dp(c))
        return c[:n.value]

    def solve(self, se3):
        x = np.array(se3, float)
        return x, self._info(Stats, "tloam_solve", _dp(x))

    def time_accumulate(self, se3, launches=100):
        x = np.ascontiguousarray(se3, float)
        us = C.c_double(0)
        self._call("tloam_time_accumulate", _dp(x), int(launches), C.byref(us))
        return us.value

    def time_build(self, launches=20):
        """(mean us per launch, queries per launch) of the correspondence-search kernel on the last frame's state."""
        us = C.c_double(0); n = C.c_int64(0)
        self._call("tloam_time_build", int(launches), C.byref(us), C.byref(n))
        return us.value, n.value

    def time_sharded_sweep(self, se3, launches=50, with_exchange=True):
        """collective: every rank calls it with the same arguments (tloam_time_sharded_sweep)."""
        x = np.ascontiguousarray(se3, float)
        us = C.c_double(0)
        self._call("tloam_time_sharded_sweep", _dp(x), int(launches), int(bool(with_exchange)), C.byref(us))
        return us.value

    def k3_timer(self, reset=False):
        us = C.c_double(0); n = C.c_int64(0); b = C.c_double(0)
        self._call("tloam_k3_timer", int(bool(reset)), C.byref(us), C.byref(n), C.byref(b))
        return us.value, n.value, b.value

    def k3_timer_all(self):
        us = C.c_double(0); n = C.c_int64(0)
        self._call("tloam_k3_timer_all", C.byref(us), C.byref(n))
        return us.value, n.value

    def k3_span(self, reset=False):
        """(total us, launches) of the streaming span of the one-launch GN iterations (tloam_k3_span)."""
        us = C.c_double(0); n = C.c_int64(0)
        self._call("tloam_k3_span", int(bool(reset)), C.byref(us), C.byref(n))
        return us.value, n.value

    def gn_iter_timer(self, reset=False):
        """(total us, periods) of the GN iterations as the device clocks them (tloam_gn_iter_timer); the first call arms it."""
        us = C.c_double(0); n = C.c_int64(0)
        self._call("tloam_gn_iter_timer", int(bool(reset)), C.byref(us), C.byref(n))
        return us.value, n.value

    def time_read_stream(self, nbytes, launches=20):
        """GB/s of a read stream with the sweep's access pattern over ~nbytes (tloam_time_read_stream)."""
        g = C.c_double(0)
        self._call("tloam_time_read_stream", int(nbytes), int(launches), C.byref(g))
        return g.value

    def info(self):
        """tloam_get_info as a dict."""
        return self._info(CtxInfo, "tloam_get_info")

    def grid_info(self):
        """tloam_get_grid_info as a dict: the search grids of the context's last grid build (per kind dim, n, ncell, cell; the
        build path GRID_SCAN_* and the size of a table entry on it)."""
        gi = GridInfo()
        self._call("tloam_get_grid_info", C.byref(gi))
        return {"dim": [list(d) for d in gi.dim], "n": gi.n[:], "ncell": gi.ncell[:], "cell": gi.cell[:],
                "scan_path": gi.scan_path, "table_elem_bytes": gi.table_elem_bytes}

    # ---- multi-GPU ---------------------------------------------------------------------------
    def comm_init_rccl(self, rank, nranks, unique_id: bytes):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._call("tloam_comm_init_rccl", int(rank), int(nranks), C.cast(buf, C.c_void_p))

    def comm_mailbox_export(self) -> bytes:
        """64 bytes (hipIpcMemHandle_t) of this context's exchange buffer; all-gather them in rank order."""
        buf = C.create_string_buffer(64)
        self._call("tloam_comm_mailbox_export", C.cast(buf, C.c_void_p))
        return bytes(buf.raw)

    def comm_init_mailbox(self, rank, nranks, handles):
        """handles: the nranks 64-byte handles in rank order (this rank's own entry is ignored)."""
        blob = b"".join(bytes(h) for h in handles)
        assert len(blob) == 64 * int(nranks)
        buf = C.create_string_buffer(blob, len(blob))
        self._call("tloam_comm_init_mailbox", int(rank), int(nranks), C.cast(buf, C.c_void_p))

    def comm_init_callback(self, rank, nranks, fn):
        """fn(device_ptr:int, count:int, stream:int) -> 0 ; must sum-all-reduce `count` doubles in place."""
        def tramp(user, dev, count, stream):
            try:
                return int(fn(dev, count, stream) or 0)
            except Exception:  # never unwind through C
                import traceback
                traceback.print_exc()
                return 1
        self._cb = ALLREDUCE_FN(tramp)
        self._call("tloam_comm_init_callback", int(rank), int(nranks), self._cb, None)


def rccl_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    rc = load_library().tloam_rccl_unique_id(C.cast(buf, C.c_void_p))
    if rc != 0:
        raise TloamHipError(f"tloam_rccl_unique_id: {STATUS.get(rc, rc)}")
    return buf.raw


def default_feature_config(**over) -> FeatureConfig:
    return _default(FeatureConfig, over)


def default_seg_config(**over) -> SegConfig:
    return _default(SegConfig, over)


def default_odom_config(**over) -> OdomConfig:
    """tloam_odom_default_config; keyword overrides name a top-level field (edge_down_sample) or one of a stage's
    fields as `<stage>__<field>`, e.g. feature__radius=0.3."""
    return _default(OdomConfig, over)


def default_map_config(**over) -> MapConfig:
    """tloam_map_default_config (mapping off, voxel 1.0) with keyword overrides, e.g. enabled=1"""
    return _default(MapConfig, over)


def default_voxel_map_config(**over) -> VoxelMapConfig:
    """tloam_voxel_map_default_config (off, voxel 1.0, origin 0) with keyword overrides, e.g. enabled=1, origin=(0, 0, 5)"""
    return _default(VoxelMapConfig, over)


def default_deskew_config(**over) -> DeskewConfig:
    """tloam_deskew_default_config (off, azimuth mode, counter-clockwise, start 0, ref 0) with keyword overrides"""
    return _default(DeskewConfig, over)


def default_place_config(**over) -> PlaceConfig:
    """tloam_place_default_config (off; 20 x 60 within 80 m, height offset 2; 10 candidates older than 50 keyframes, a loop
    below 0.30; a keyframe every 1 m or 0.2 rad) with keyword overrides"""
    return _default(PlaceConfig, over)


def default_loop_config(**over) -> LoopConfig:
    """tloam_loop_default_config (off; a window of 2, the loop record's yaw as the guess; the measured score bounds; the coarse
    stage's TLS values) with keyword overrides; `coarse__<name>` sets a field of the coarse TLS configuration"""
    return _default(LoopConfig, over)


def default_graph_config(**over) -> GraphConfig:
    """tloam_graph_default_config (30 Gauss-Newton iterations of at most 20000 conjugate-gradient iterations, step_tol 1e-7,
    cg_tol 1e-10, the odometry and loop sigmas) with keyword overrides"""
    return _default(GraphConfig, over)


def default_graph_robust_config(**over) -> GraphRobustConfig:
    """tloam_graph_robust_default_config (off; noise_chi2 36, mu_factor 1.4, at most 100 outer iterations) with keyword
    overrides, e.g. enabled=1"""
    return _default(GraphRobustConfig, over)


def default_closed_map_config(**over) -> ClosedMapConfig:
    """tloam_closed_map_default_config (voxel 1.0, origin 0, cloud_mask 0xF0) with keyword overrides, e.g. voxel=0.25,
    origin=(0, 0, 5), cloud_mask=0x0F"""
    return _default(ClosedMapConfig, over)


def default_closed_map_carve_config(**over) -> ClosedMapCarveConfig:
    """tloam_closed_map_carve_default_config (max_range 60, end_margin 1, radius 0.25, ray_mask 0: the build's) with keyword
    overrides, e.g. max_range=20.0, radius=float("inf")"""
    return _default(ClosedMapCarveConfig, over)


def default_closed_map_raycast_config(**over) -> ClosedMapRaycastConfig:
    """tloam_closed_map_raycast_default_config (max_range 120, radius_cells 0.75, planes 1, min_count 1, min_miss 3,
    miss_ratio 1, carve_gate 0) with `over` applied; an unknown field raises"""
    return _default(ClosedMapRaycastConfig, over)


def default_closed_map_free_config(**over) -> FreeConfig:
    """tloam_closed_map_free_default_config (max_range 60, end_margin 1, ray_mask 0: the build's, max_bytes 1 GiB, min_count 1,
    min_miss 3, miss_ratio 1, carve_gate 0) with keyword overrides; an unknown field raises"""
    return _default(FreeConfig, over)


def default_closed_map_frontier_config(**over) -> FrontierConfig:
    """tloam_closed_map_frontier_default_config (max_bytes 1 GiB, min_cells 8, reach 2, max_rounds 65536, rounds_per_wait 16)
    with keyword overrides"""
    return _default(FrontierConfig, over)


def default_closed_map_view_config(**over) -> ViewConfig:
    """tloam_closed_map_view_default_config (max_range 20, max_bytes 256 MiB, lds_bytes 131072, form 0: auto) with keyword
    overrides"""
    return _default(ViewConfig, over)


def default_closed_map_route_config(**over) -> RouteConfig:
    """tloam_closed_map_route_default_config (max_bytes 1 GiB, max_rounds 65536, rounds_per_wait 16) with keyword overrides"""
    return _default(RouteConfig, over)


def default_closed_map_clearance_config(**over) -> ClearanceConfig:
    """tloam_closed_map_clearance_default_config (max_distance 4, max_segment 120, max_bytes 1 GiB, unknown_is_obstacle 1) with
    keyword overrides; an unknown field raises"""
    return _default(ClearanceConfig, over)


def default_closed_map_diff_config(**over) -> ClosedMapDiffConfig:
    """tloam_closed_map_diff_default_config (max_range 60, end_margin 1, radius 0.25, plane_tol 0.1, near 0.5, min_miss 3,
    miss_ratio 1, carve_gate 0) with keyword overrides, e.g. max_range=20.0, carve_gate=1"""
    return _default(ClosedMapDiffConfig, over)


def default_closed_map_relocalise_config(**over) -> ClosedMapRelocaliseConfig:
    """tloam_closed_map_relocalise_default_config with keyword overrides."""
    return _default(ClosedMapRelocaliseConfig, over)


def default_closed_map_localise_config(**over) -> ClosedMapLocaliseConfig:
    """tloam_closed_map_localise_default_config with keyword overrides."""
    return _default(ClosedMapLocaliseConfig, over)


def default_closed_map_surfel_config(**over) -> ClosedMapSurfelConfig:
    """tloam_closed_map_surfel_default_config (min_points 5) with keyword overrides."""
    return _default(ClosedMapSurfelConfig, over)


def default_submap_config(**over) -> SubmapConfig:
    return _default(SubmapConfig, over)


def make_registration(method: str, cfg: TlsConfig | None = None, device: int = 0):
    """FrontEnd::initRegistraton (front_end.cpp:155-167) keyed on `local_registration_method`."""
    if method == "TLS_HIP":
        return HipRegistration(cfg, device)
    raise ValueError("Other methods are not yet supported")  # the reference's message, front_end.cpp:163
