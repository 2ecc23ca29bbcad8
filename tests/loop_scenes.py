"""Named hand-made keyframe sets for loop verification: one per branch of the assembly and the score
that the out-and-back street of tests/test_gpu_loop.py never reaches -- a window clipped at keyframe 0 and at q - 1, window 0
and a window wider than the database, a kind that reaches 10 target points by the window alone, keyframes inside the window
without a cloud of a kind (the skipped span), span counts around the 16 spans of one launch, a launch of more rows than
k_loop_assemble's 1024 x 256 threads, a kind of more source points than k_loop_score's 256 x 256 threads, a source of 9 points,
source points many grid cells from every target (what a score's reach above 1 must still find).
tests/test_loop_scenes.py asserts every scene's stated condition on the CPU; tests/test_gpu_loop_edges.py runs every scene on
the device against the restatement (tests/loop_np.py) and the public match calls, bit for bit.

The world is static and small: a 12 m ground patch, two walls at right angles, six poles, five compact blobs.  A keyframe's
eight clouds are random draws from it, each cloud a draw of its own (no two clouds are equal), moved into the keyframe's sensor
frame by inv(P_k).  Kinds as TLOAM_KIND_*: planar 0 (the walls), ground 1, edge 2 (the poles), sphere 3 (the blobs).  The poses
carry roll and pitch of a few degrees besides any yaw and lie 1 m apart or less; the last keyframe comes back beside keyframe 5.

A scene is (name, poses, src, tgt, q, m, window, spans, filled): src[k] / tgt[k] the four source / target clouds of keyframe k,
(q, m) the pair to verify under `window` (None: the configuration's default), `spans` the span count the scene states (None
where it states none), `filled` the target clouds before holes were cut (None without holes)."""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np

import loop_np as LN

PLANAR, GROUND, EDGE, SPHERE = range(4)
BASE_N = (300, 400, 150, 40)          # per keyframe and side: the smallest at which a match still has >= 10 of every kind
SPANS_PER_LAUNCH = 16                 # kLoopSpans
ASSEMBLE_THREADS = 1024 * 256         # k_loop_assemble: at most 1024 blocks of 256, one row per thread and turn
SCORE_THREADS = LN.SCORE_THREADS      # k_loop_score: 256 blocks of 256, one point per thread and turn
MIN_POINTS = 10                       # tloam_scan_match: fewer in one of the eight clouds is TLOAM_E_TOO_FEW_POINTS
DEFAULT_WINDOW = 2

WALLS = (((6.0, -5.0, 0.0), (0.0, 10.0, 0.0), (0.0, 0.0, 3.0)),     # (corner, first edge, second edge): x = 6 and y = 6
         ((-5.0, 6.0, 0.0), (10.0, 0.0, 0.0), (0.0, 0.0, 3.0)))
GROUND_HALF = 6.0
POLES = ((3.0, 2.5), (-2.0, 4.0), (-4.5, -1.0), (1.0, -4.0), (4.5, -2.5), (-1.5, -2.0))
POLE_HEIGHT = 3.0
BLOBS = ((2.0, 3.5, 0.6), (-3.0, 1.0, 1.2), (0.5, -3.0, 0.4), (4.0, 0.5, 1.5), (-1.0, 2.0, 2.0))
BLOB_HALF = 0.04


class Scene(NamedTuple):
    name: str
    poses: np.ndarray
    src: list
    tgt: list
    q: int
    m: int
    window: int | None
    spans: int | None
    filled: list | None


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


# ---- the world ---------------------------------------------------------------------------------------------------------------
def world_points(kind, n, rng):
    """n points of the world's `kind`, world frame"""
    if kind == PLANAR:
        w = rng.integers(0, len(WALLS), n)
        c, a, b = (np.asarray([W[i] for W in WALLS])[w] for i in range(3))
        return c + rng.random((n, 1)) * a + rng.random((n, 1)) * b
    if kind == GROUND:
        xy = (rng.random((n, 2)) * 2.0 - 1.0) * GROUND_HALF
        return np.column_stack([xy, np.zeros(n)])
    if kind == EDGE:
        p = np.asarray(POLES)[rng.integers(0, len(POLES), n)]
        return np.column_stack([p, rng.random(n) * POLE_HEIGHT])
    c = np.asarray(BLOBS)[rng.integers(0, len(BLOBS), n)]
    return c + (rng.random((n, 3)) * 2.0 - 1.0) * BLOB_HALF


def rot(yaw, pitch, roll):
    """Rz(yaw) Ry(pitch) Rx(roll)"""
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Rz = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cr, -sr], [0.0, sr, cr]])
    return Rz @ Ry @ Rx


def pose(x, y, z, yaw_deg, pitch_deg, roll_deg):
    T = np.eye(4)
    T[:3, :3] = rot(math.radians(yaw_deg), math.radians(pitch_deg), math.radians(roll_deg))
    T[:3, 3] = (x, y, z)
    return T


# out along x through keyframe 5 at the origin, a turn, and back beside keyframe 5: (x, y, z, yaw, pitch, roll), degrees
TRACK_12 = ((-3.5, 0.10, 1.00, 3.0, 1.5, -2.0), (-2.8, 0.00, 1.05, -2.0, -2.5, 1.0), (-2.1, -0.10, 0.95, 5.0, 2.0, 3.0),
            (-1.4, 0.05, 1.00, -4.0, 3.0, -1.5), (-0.7, 0.10, 1.02, 1.0, -1.0, 2.5), (0.0, 0.00, 1.00, 6.0, 2.5, -3.0),
            (0.7, -0.05, 0.98, 20.0, -3.0, 1.5), (1.4, 0.20, 1.03, 70.0, 1.0, 2.0), (1.5, 0.80, 1.00, 150.0, -2.0, -2.5),
            (0.9, 0.90, 0.97, 185.0, 3.0, 1.0), (0.5, 0.60, 1.04, 200.0, -1.5, 3.0), (0.2, 0.30, 1.01, 190.0, 2.0, -2.0))
# the same, longer: six more keyframes of a wider turn before the return
TRACK_18 = TRACK_12[:8] + ((2.1, 0.50, 1.00, 40.0, 2.0, 1.0), (2.6, 1.10, 1.02, 80.0, -2.0, 2.0),
                           (2.4, 1.90, 0.97, 130.0, 1.0, -3.0), (1.7, 2.20, 1.00, 180.0, 3.0, 1.5),
                           (1.1, 1.80, 1.03, 230.0, -2.5, -1.0), (1.2, 1.20, 0.99, 280.0, 1.5, 2.5)) + TRACK_12[8:]


def poses_of(track):
    return np.stack([pose(*p) for p in track])


def cloud(seed, k, side, kind, n, T):
    """keyframe k's cloud of (side, kind): n world points of a draw of its own, in the sensor frame of pose T"""
    rng = np.random.default_rng([seed, k, side, kind])
    w = world_points(kind, n, rng)
    Ti = np.linalg.inv(T)
    return np.ascontiguousarray(w @ Ti[:3, :3].T + Ti[:3, 3])


def keyframes(seed, poses, n_src=None, n_tgt=None):
    """(src, tgt) for every keyframe: BASE_N points per cloud unless n_src / n_tgt {(keyframe, kind): n} says otherwise"""
    n_src, n_tgt = n_src or {}, n_tgt or {}
    src = [[cloud(seed, k, 0, kind, n_src.get((k, kind), BASE_N[kind]), T) for kind in range(4)] for k, T in enumerate(poses)]
    tgt = [[cloud(seed, k, 1, kind, n_tgt.get((k, kind), BASE_N[kind]), T) for kind in range(4)] for k, T in enumerate(poses)]
    return src, tgt


def cut(tgt, holes):
    """the target clouds with the (keyframe, kind) of `holes` emptied"""
    return [[np.zeros((0, 3)) if (k, kind) in holes else c for kind, c in enumerate(kf)] for k, kf in enumerate(tgt)]


# ---- what the device will do with a scene, from the scene alone ----------------------------------------------------------------
def window_of(sc, window=None, m=None):
    w = window if window is not None else (sc.window if sc.window is not None else DEFAULT_WINDOW)
    return LN.window(sc.q, sc.m if m is None else m, w)


def span_rows(sc, window=None, m=None):
    """rows of every span in the order verify() lists them: the query's non-empty source kinds, then per kind the window's
    non-empty targets, ascending"""
    ks = window_of(sc, window, m)
    rows = [len(c) for c in sc.src[sc.q] if len(c)]
    for kind in range(4):
        rows += [len(sc.tgt[k][kind]) for k in ks if len(sc.tgt[k][kind])]
    return rows


def launch_rows(sc, window=None, m=None):
    """rows per k_loop_assemble launch: the spans in groups of 16"""
    rows = span_rows(sc, window, m)
    return [sum(rows[b:b + SPANS_PER_LAUNCH]) for b in range(0, len(rows), SPANS_PER_LAUNCH)]


def target_totals(sc, window=None, m=None):
    ks = window_of(sc, window, m)
    return [sum(len(sc.tgt[k][kind]) for k in ks) for kind in range(4)]


def scan_of(sc, k):
    """a small scan for keyframe k's descriptor: its target clouds end to end (the verification does not depend on it)"""
    parts = [c for c in (sc.filled or sc.tgt)[k] if len(c)]
    return np.ascontiguousarray(np.concatenate(parts)[:1000])


# ---- the scenes -------------------------------------------------------------------------------------------------------------
HOLES = {(4, PLANAR), (6, EDGE), (6, GROUND)}
# seven (keyframe offset from m, kind) holes that leave every kind in at least two of the window's keyframes
SEVEN = ((-2, PLANAR), (-2, GROUND), (-1, EDGE), (-1, SPHERE), (1, PLANAR), (1, EDGE), (2, SPHERE))
BIG_ROWS_N = 17000
BIG_ROWS_PLANAR_HOLES = (1, 4, 7, 10, 13)


def _plain(name, seed, q, m, window, spans=None, holes=(), n_src=None, n_tgt=None, track=TRACK_12):
    poses = poses_of(track)
    src, tgt = keyframes(seed, poses, n_src, n_tgt)
    holes = set(holes)
    return Scene(name, poses, src, cut(tgt, holes) if holes else tgt, q, m, window, spans, tgt if holes else None)


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "base":
        return _plain(name, 1, 11, 5, None)
    if name == "clip_low":
        return _plain(name, 2, 11, 1, 3)
    if name == "clip_high":
        return _plain(name, 3, 11, 10, 3)
    if name == "window_zero":
        return _plain(name, 4, 11, 5, 0)
    if name == "window_huge":
        return _plain(name, 5, 11, 5, 1 << 20)
    if name == "spread_sphere":      # also run at window 0 and at m = 0: SPREAD_RUNS
        return _plain(name, 6, 11, 5, 1, n_tgt={(k, SPHERE): 4 for k in range(12)})
    if name == "holes":
        return _plain(name, 7, 11, 5, 2, spans=4 + 4 * 5 - 3, holes=HOLES)
    if name == "spans_16":
        return _plain(name, 8, 11, 5, 1, spans=16)
    if name == "spans_17":
        return _plain(name, 9, 11, 5, 2, spans=17, holes=[(5 + d, kind) for d, kind in SEVEN])
    if name == "spans_33":
        return _plain(name, 10, 11, 5, 4, spans=33, holes=[(5 + 2 * d, kind) for d, kind in SEVEN])
    if name == "big_rows":
        # 16 000 points a keyframe, as first planned, cannot wrap the walk: a launch holds at most 16 spans, 256 000 rows.  With
        # 17 000, and five keyframes without a planar target so that the ground spans begin a launch (spans 16..32: 4 source
        # + 12 planar before them), the second launch is 16 ground spans of 272 000 rows
        n_tgt = {(k, GROUND): BIG_ROWS_N for k in range(17)}
        return _plain(name, 11, 17, 8, 8, holes=[(k, PLANAR) for k in BIG_ROWS_PLANAR_HOLES], n_tgt=n_tgt, track=TRACK_18)
    if name == "big_source":
        return _plain(name, 12, 11, 5, None, n_src={(11, GROUND): SCORE_THREADS + 300})
    if name == "nine_sphere":
        return _plain(name, 13, 11, 5, None, n_src={(11, SPHERE): 9})
    if name == "far_points":
        # base's sizes, and FAR_N more sphere points in the query's source around a sixth blob that no target holds: further
        # than FAR_MIN from every sphere target (many cells of the sphere grid: a walk of the 27 cells around them finds
        # nothing), nearer than FAR_MAX to one
        sc = _plain(name, 14, 11, 5, None)
        rng = np.random.default_rng([14, 99])
        far = np.asarray(FAR_BLOB) + (rng.random((FAR_N, 3)) * 2.0 - 1.0) * BLOB_HALF
        Ti = np.linalg.inv(sc.poses[sc.q])
        sc.src[sc.q][SPHERE] = np.ascontiguousarray(np.concatenate([sc.src[sc.q][SPHERE], far @ Ti[:3, :3].T + Ti[:3, 3]]))
        return sc
    raise KeyError(name)


FAR_BLOB, FAR_N, FAR_MIN, FAR_MAX = (-4.0, -4.0, 1.0), 10, 3.0, 5.0
NAMES = ("base", "clip_low", "clip_high", "window_zero", "window_huge", "spread_sphere", "holes", "spans_16", "spans_17",
         "spans_33", "big_rows", "big_source", "nine_sphere", "far_points")
# the place configuration under which base's own keyframes (scan_of) give loop records of many headings, for init_mode
PLACE_FOR_LOOPS = dict(exclude_recent=2)
# spread_sphere's three runs: (m, window, the window's sphere targets)
SPREAD_RUNS = ((5, 1, 12), (5, 0, 4), (0, 1, 8))
