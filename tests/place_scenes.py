"""Named hand-made inputs for place recognition: one per branch of tl_place.hip that a generator scan
reaches only by accident, or never -- the clamps of the binning, the second turn of k_place_bin's grid-stride loop, wave runs
of every shape, more than 256 and 512 searchable keyframes, exact ties, empty columns, the strict threshold, grids other
than 20 x 60.  tests/test_place_scenes.py checks every scene on the CPU (margin report, descriptor, witness);
tests/test_gpu_place_edges.py runs every scene on the device against the restatement (tests/place_np.py), bit for bit.

Everything is built on scan_of: an R x S descriptor of small dyadic rationals turned into one return per non-zero bin, at the
bin's centre.  With dyadic values z + height_offset gives the value back exactly, every key sum is exact, and an intended tie
is an exact tie.

A descriptor scene is (name, xyz, grid, boundary, desc, witness): `boundary` lists the returns that may appear in
place_np.margins (empty for every scene but axis_clamps, whose returns sit on atan2's IEEE special values on purpose), `desc`
is the descriptor written down independently of place_np.describe, witness(xyz, grid) proves on the restatement that the
scene reaches the branch it is named for.
A database scene is (name, cfg, device, descs, scans, witness): the scans are added one by one under the identity pose with
frame numbers 100, 101, ...; cfg is the restatement's configuration, `device` what the device gets on top of it
(reserve_keyframes); witness(db, descs) is a predicate on the restated PlaceDB."""
from __future__ import annotations

import functools
import math
from typing import Callable, NamedTuple

import numpy as np

import place_np as P

GRID_KEYS = ("n_rings", "n_sectors", "max_radius", "height_offset")
TURN = 1024 * 256         # k_place_bin: at most 1024 blocks of 256, one return per thread and turn
WAVE, BLOCK = 64, 256
FIRST_FRAME = 100


class DescScene(NamedTuple):
    name: str
    xyz: np.ndarray
    grid: dict
    boundary: tuple
    desc: np.ndarray
    witness: Callable


class DbScene(NamedTuple):
    name: str
    cfg: dict
    device: dict
    descs: list
    scans: list
    witness: Callable


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def grid_of(**over):
    c = P.cfg_of(**over)
    return {k: c[k] for k in GRID_KEYS}


def centre(i, j, **grid):
    """(x, y) of the centre of bin (ring i, sector j)"""
    c = P.cfg_of(**grid)
    r = (np.asarray(i) + 0.5) * c["max_radius"] / c["n_rings"]
    theta = -P.PI + (np.asarray(j) + 0.5) * P.TWO_PI / c["n_sectors"]
    return r * np.cos(theta), r * np.sin(theta)


def returns_of(i, j, h, **grid):
    """one return per entry: bin (i, j) at its centre, height h in the descriptor"""
    x, y = centre(i, j, **grid)
    z = np.asarray(h, np.float64) - P.cfg_of(**grid)["height_offset"]
    return np.ascontiguousarray(np.stack([x, y, z], axis=1))


def scan_of(desc, **grid):
    """an R x S descriptor -> the scan with one return per non-zero bin, at the bin's centre, ring by ring"""
    c = P.cfg_of(**grid)
    d = np.asarray(desc, np.float64)
    assert d.shape == (c["n_rings"], c["n_sectors"])
    i, j = np.nonzero(d)
    return returns_of(i, j, d[i, j], **grid)


def far_scan(**grid):
    """a few returns, every one beyond max_radius: the all-zero descriptor of a scan that is not empty"""
    m = P.cfg_of(**grid)["max_radius"]
    return np.array([[1.25 * m, 0.0, 1.0], [0.0, -2.5 * m, 3.0], [-1.125 * m, 1.125 * m, 0.5]])


def dyadic(seed, R, S, lo=1, hi=33, step=8.0):
    """seeded R x S multiples of 1 / step in [lo / step, (hi - 1) / step]"""
    return np.random.default_rng(seed).integers(lo, hi, (R, S)) / step


def square_cols(seed, R, S):
    """every column holds k in {1, 4, 9, 16} equal entries v = m / 8 and zeros: its norm sqrt(k) v is exact, so the cosine of a
    column with itself is exactly 1 and the distance of a descriptor to its own column roll exactly 0.0"""
    rng = np.random.default_rng(seed)
    d = np.zeros((R, S))
    counts = [k for k in (1, 4, 9, 16) if k <= R]
    for j in range(S):
        k = counts[rng.integers(len(counts))]
        d[rng.choice(R, k, replace=False), j] = rng.integers(1, 17) / 8.0
    return d


def noisy(seed, d, p=0.25, step=0.125):
    """d with one dyadic step added to or taken from a seeded share of its entries (no entry goes to zero or below)"""
    rng = np.random.default_rng(seed)
    e = rng.choice([-step, 0.0, step], d.shape, p=[p / 2, 1 - p, p / 2])
    return np.where(d + e > 0.0, d + e, d)


def quotients(xyz, **grid):
    """the unclamped (ring, sector) quotients of the restatement's binning"""
    c = P.cfg_of(**grid)
    x, y = xyz[:, 0], xyz[:, 1]
    with np.errstate(over="ignore", invalid="ignore"):
        qr = np.sqrt(x * x + y * y) / (c["max_radius"] / c["n_rings"])
        qs = (np.arctan2(y, x) + P.PI) / (P.TWO_PI / c["n_sectors"])
    return qr, qs


# ---- descriptor scenes ---------------------------------------------------------------------------------------------------
AXIS_GRIDS = ((20, 60), (7, 37), (1, 2), (64, 360))
# The ring quotient of a return below max_radius reaches R only where max_radius / R rounds down: never where R is a power of
# two (the division is exact, so is the quotient, and it stays below R), and not at 80 m with 20 rings (ring width 4.0).  The
# radii below are ones where nextafter(max_radius, 0) / (max_radius / R) rounds to R; (1, 2) and (64, 360) cannot hit the clamp
AXIS_RADIUS = {(20, 60): 41.0, (7, 37): 61.0, (1, 2): 80.0, (64, 360): 80.0}
AXIS_USED = 5


def _axis_clamps(R, S):
    grid = grid_of(n_rings=R, n_sectors=S, max_radius=AXIS_RADIUS[R, S])
    m, ho = grid["max_radius"], grid["height_offset"]
    a = 0.37 * m
    xyz = np.array([
        [-a, 0.0, 5.0 - ho],               # 0: atan2 = +pi, the sector quotient is S: clamped to S - 1
        [-a, -0.0, 4.5 - ho],              # 1: atan2 = -pi: sector 0
        [a, 0.0, 3.0 - ho],                # 2: atan2 = +0: sector S / 2
        [a, -0.0, 3.5 - ho],               # 3: atan2 = -0: sector S / 2
        [np.nextafter(m, 0.0), 0.0, 4.0 - ho],   # 4: the ring quotient rounds to R: clamped to R - 1
        [m, 0.0, 9.0],                     # unused: r == max_radius
        [5e-324, 0.0, 9.0],                # unused: x * x underflows, r == 0
        [1e-200, 1e-200, 9.0],             # unused: r == 0
        [1e200, 0.0, 9.0]])                # unused: x * x overflows, r == inf
    ra = int(0.37 * R)
    want = np.zeros((R, S))
    for (i, j), h in zip([(ra, S - 1), (ra, 0), (ra, S // 2), (ra, S // 2), (R - 1, S // 2)], [5.0, 4.5, 3.0, 3.5, 4.0]):
        want[i, j] = max(want[i, j], h)

    def witness(xyz, grid):
        ring, sector, used = P.bins(xyz, **grid)
        qr, qs = quotients(xyz, **grid)
        return (used[:AXIS_USED].all() and not used[AXIS_USED:].any()
                and math.floor(qs[0]) == S and sector[0] == S - 1          # the sector clamp is hit
                and qs[1] == 0.0 and sector[1] == 0
                and sector[2] == S // 2 and sector[3] == S // 2
                and (math.floor(qr[4]) == R) == (R & (R - 1) != 0) and ring[4] == R - 1   # the ring clamp is hit
                and xyz[4, 0] < grid["max_radius"] and list(ring[:4]) == [ra] * 4)
    boundary = (0, 1, 2, 3, 4) if S % 2 == 0 else (0, 1, 4)   # +-0 over x > 0 is sector S / 2 exactly only for an even S
    return DescScene(f"axis_clamps_{R}x{S}", xyz, grid, boundary, want, witness)


def _heights(name, height_offset, cells):
    """cells: (sector, [heights z + height_offset is to give], the bin's value), all in ring 3"""
    grid = grid_of(height_offset=height_offset)
    i, j, z = [], [], []
    want = np.zeros((grid["n_rings"], grid["n_sectors"]))
    for sector, zs, value in cells:
        for v in zs:
            i.append(3); j.append(sector); z.append(v)
        want[3, sector] = value
    x, y = centre(np.array(i), np.array(j), **grid)
    xyz = np.ascontiguousarray(np.stack([x, y, np.array(z, np.float64)], axis=1))

    def witness(xyz, grid):
        d = P.describe(xyz, **grid)[0]
        return bits(d) == bits(want) and bool(np.signbit(d[3, 6]) == np.signbit(want[3, 6])) and (d[3, 5] < 0)
    return DescScene(name, xyz, grid, (), want, witness)


def _heights_signed_zero():
    # height_offset -0.0: z + (-0.0) is z, sign of zero included (with any other offset a sum is never -0.0)
    tiny = 5e-324
    return _heights("heights_signed_zero", -0.0, [
        (5, [-1.5, -0.75, -1.0], -0.75),          # a negative maximum
        (6, [-0.0, -0.0], -0.0),                  # -0.0: occupied, and not the empty bin's +0.0
        (7, [0.0], 0.0),                          # +0.0: occupied, reads like the empty bin
        (8, [-0.0, 0.0, -0.0], 0.0),              # +0.0 is above -0.0
        (9, [-tiny, tiny, 0.0, -0.0], tiny),      # denormals
        (10, [-tiny, -1.0], -tiny),
        (11, [1.25], 1.25)])


def _heights_offset():
    return _heights("heights_offset", 2.0, [
        (5, [-3.5, -2.75, -3.0], -0.75),          # a negative maximum under the default offset
        (6, [-3.0, -2.0, -2.5], 0.0),             # z == -height_offset: the sum +0.0 beats the negative sums
        (7, [-2.0], 0.0),
        (11, [-0.75], 1.25)])


RUN_LENGTHS = (1, 2, 63, 64, 65, 256, 257)
RUN_MAXIMA = ("first", "middle", "last")
RUN_PAD = 37


@functools.lru_cache(maxsize=None)
def run_table():
    """(start, length, position of the maximum, (ring, sector), maximum) of every run of `runs`, in scan order.  Earlier runs
    have the larger maxima: a maximum that leaks up the wave from another run's lanes shows"""
    table, at, k = [], RUN_PAD, 0
    for L in RUN_LENGTHS:
        for pos in RUN_MAXIMA:
            p = {"first": 0, "middle": L // 2, "last": L - 1}[pos]
            table.append((at, L, p, (1, k), 8.0 - k / 8.0))
            at += L
            k += 1
    return tuple(table), at


def _runs():
    grid = grid_of()
    R, S = grid["n_rings"], grid["n_sectors"]
    table, at = run_table()
    i, j, h = [0] * RUN_PAD, [0] * RUN_PAD, [(k % 7 + 1) / 64.0 for k in range(RUN_PAD)]
    want = np.zeros((R, S))
    want[0, 0] = 7 / 64.0
    for start, L, p, (bi, bj), top in table:
        v = ((np.arange(L) * 7) % 61 + 1) / 64.0
        v[p] = top
        i += [bi] * L; j += [bj] * L; h += list(v)
        want[bi, bj] = top
    # a run broken by a NaN return (two runs of one bin), one broken by a return of another bin, one of negative heights
    nan_at = len(h) + 20
    i += [2] * 64; j += [0] * 64; h += [(k % 5 + 1) / 64.0 for k in range(64)]
    h[nan_at - 17], h[nan_at + 9] = 5.0, 4.5
    want[2, 0] = 5.0
    other_at = len(h) + 30
    i += [2] * 61; j += [1] * 30 + [2] + [1] * 30; h += [(k % 5 + 1) / 64.0 for k in range(61)]
    h[other_at - 30], h[other_at], h[other_at + 30] = 4.0, 0.5, 3.75
    want[2, 1], want[2, 2] = 4.0, 0.5
    i += [2] * 65; j += [3] * 65; h += [-(k % 9 + 2) / 64.0 for k in range(65)]
    h[-33] = -1 / 64.0
    want[2, 3] = -1 / 64.0
    xyz = returns_of(np.array(i), np.array(j), np.array(h), **grid)
    xyz[nan_at, 0] = np.nan

    def witness(xyz, grid):
        ring, sector, used = P.bins(xyz, **grid)
        flat = np.where(used, ring * S + sector, -1)
        ok = len({b for *_, b, _ in table}) == len(table)                 # a bin per run
        for start, L, p, (bi, bj), top in table:
            ok = ok and (flat[start:start + L] == bi * S + bj).all() and flat[start - 1] != bi * S + bj
            ok = ok and xyz[start + p, 2] + grid["height_offset"] == top
        crosses = lambda w: any(s // w != (s + L - 1) // w for s, L, *_ in table)   # noqa: E731
        inside = any(s // WAVE == (s + L - 1) // WAVE and L > 1 for s, L, *_ in table)
        return (ok and crosses(WAVE) and crosses(BLOCK) and inside and not used[nan_at]
                and flat[nan_at - 1] == flat[nan_at + 1] == 2 * S and flat[other_at] == 2 * S + 2
                and flat[other_at - 1] == flat[other_at + 1] == 2 * S + 1 and len(xyz) < TURN)
    return DescScene("runs", xyz, grid, (), want, witness)


TWO_TURNS_N = TURN + 3 * BLOCK + 17
TWO_TURNS_RUN = 100


def _two_turns():
    grid = grid_of()
    R, S = grid["n_rings"], grid["n_sectors"]
    n = TWO_TURNS_N
    k = np.arange(n)
    flat = (k // TWO_TURNS_RUN) % (R * S)         # runs of 100 returns, bin after bin, each bin two or three times
    h = np.random.default_rng(7).integers(1, 257, n) / 64.0      # (0, 4]
    h[TURN + 5] = 6.0                             # in the run that crosses the turn boundary
    h[n - 1] = 7.0                                # the last return, in the partial block of the second turn
    xyz = returns_of(flat // S, flat % S, h, **grid)
    want = np.zeros(R * S)
    np.maximum.at(want, flat, h)

    def witness(xyz, grid):
        ring, sector, used = P.bins(xyz, **grid)
        b = ring * S + sector
        d = P.describe(xyz, **grid)[0].reshape(-1)
        return (used.all() and len(xyz) > TURN and (len(xyz) - TURN) % BLOCK != 0 and len(xyz) < 2 * TURN
                and b[TURN - 1] == b[TURN]                                  # a run crosses the turn boundary
                and d[b[TURN + 5]] == 6.0 and d[b[-1]] == 7.0 and b[TURN + 5] != b[-1]   # winners of the second turn
                and h[:TURN].max() < 6.0)
    return DescScene("two_turns", xyz, grid, (), want.reshape(R, S), witness)


DESC_BUILDERS = {f"axis_clamps_{R}x{S}": functools.partial(_axis_clamps, R, S) for R, S in AXIS_GRIDS}
DESC_BUILDERS.update(heights_signed_zero=_heights_signed_zero, heights_offset=_heights_offset, runs=_runs,
                     two_turns=_two_turns)
DESC_NAMES = tuple(DESC_BUILDERS)
SMALL_DESC_NAMES = tuple(n for n in DESC_NAMES if n != "two_turns")


@functools.lru_cache(maxsize=None)
def desc_scene(name) -> DescScene:
    return DESC_BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def described(name):
    """the restatement's (descriptor, ring key, sector key) of a descriptor scene"""
    sc = desc_scene(name)
    return P.describe(sc.xyz, **sc.grid)


# ---- database scenes -----------------------------------------------------------------------------------------------------
def _db(name, cfg, descs, witness, device=None, scans=None):
    grid = grid_of(**{k: v for k, v in cfg.items() if k in GRID_KEYS})
    if scans is None:
        scans = [scan_of(d, **grid) for d in descs]
    return DbScene(name, cfg, device or {}, descs, scans, witness)


def last_loop(db, q):
    for L in db.loops:
        if L["query"] == q:
            return L
    return None


def roll(d, r):
    """the candidate a query d matches at shift r: column j of d is column j + r of the result"""
    return np.roll(d, r, axis=1)


def _rank_ties():
    D = square_cols(11, 20, 60)
    descs = [roll(D, r) for r in (11, 23, 0, 35, 47)] + [D]

    def witness(db, descs):
        kd = [P.key_distance(db.rkey[5], db.rkey[k]) for k in range(5)]
        L = last_loop(db, 5)
        return (kd == [0.0] * 5 and db.candidates(5) == [0, 1] and L is not None
                and (L["match"], L["shift"], L["d"]) == (0, 11, 0.0)
                and P.shift_distances(descs[5], descs[2])[0] == 0.0)       # the exact copy ties and is not reached
    return _db("rank_ties", dict(num_candidates=2, exclude_recent=1), descs, witness)


def _shift_ties_halves():
    A = square_cols(12, 20, 30)
    H = np.concatenate([A, A], axis=1)
    descs = [roll(H, 7), H]

    def witness(db, descs):
        d = P.shift_distances(descs[1], descs[0])
        L = last_loop(db, 1)
        return d[7] == 0.0 and d[37] == 0.0 and (d[:7] > 0.0).all() and L is not None and (L["shift"], L["d"]) == (7, 0.0)
    return _db("shift_ties_halves", dict(num_candidates=1, exclude_recent=1), descs, witness)


def _shift_ties_constant():
    col = square_cols(13, 20, 1)
    Cn = np.repeat(col, 60, axis=1)
    descs = [Cn, Cn.copy()]

    def witness(db, descs):
        d = P.shift_distances(descs[1], descs[0])
        L = last_loop(db, 1)
        return (d == 0.0).all() and L is not None and (L["shift"], L["d"], L["yaw"]) == (0, 0.0, 0.0)
    return _db("shift_ties_constant", dict(num_candidates=1, exclude_recent=1), descs, witness)


def _pick(name, descs, want, check):
    def witness(db, descs):
        best = [(float(d.min()), int(np.argmin(d))) for d in (P.shift_distances(descs[2], descs[k]) for k in (0, 1))]
        L = last_loop(db, 2)
        return (sorted(db.candidates(2)) == [0, 1] and check(best) and L is not None
                and (L["match"], L["shift"]) == want and L["d"] == best[want[0]][0])
    return _db(name, dict(num_candidates=2, exclude_recent=1), descs, witness)


def _pick_ties_copies():
    D = square_cols(14, 20, 60)
    return _pick("pick_ties_copies", [roll(D, 5), roll(D, 5), D], (0, 5), lambda b: b[0] == b[1] == (0.0, 5))


def _pick_ties_shift():
    D = square_cols(15, 20, 60)   # equal d; the lower shift belongs to the higher id
    return _pick("pick_ties_shift", [roll(D, 9), roll(D, 4), D], (1, 4), lambda b: b == [(0.0, 9), (0.0, 4)])


def _pick_ties_distance():
    D = square_cols(16, 20, 60)   # the lower d belongs to the higher shift and the higher id
    return _pick("pick_ties_distance", [roll(noisy(3, D), 3), roll(D, 20), D], (1, 20),
                 lambda b: b[0][1] == 3 and b[0][0] > 0.0 and b[1] == (0.0, 20))


YAW_ROLLS = (0, 1, 29, 30, 31, 59)


def _yaw_wrap():
    descs = []
    for k, r in enumerate(YAW_ROLLS):
        D = square_cols(20 + k, 20, 60)
        descs += [roll(D, r), D]

    def witness(db, descs):
        ok = True
        for k, r in enumerate(YAW_ROLLS):
            L = last_loop(db, 2 * k + 1)
            ok = ok and L is not None and (L["match"], L["shift"], L["d"]) == (2 * k, r, 0.0)
            ok = ok and L["yaw"] == P.yaw_of(r, 60) and abs(L["yaw"]) <= math.pi
        yaw = {r: last_loop(db, 2 * k + 1)["yaw"] for k, r in enumerate(YAW_ROLLS)}
        return (ok and yaw[0] == 0.0 and yaw[30] == math.pi and yaw[31] < -3.0 and yaw[29] > 3.0
                and -0.11 < yaw[59] < -0.10 and 0.10 < yaw[1] < 0.11)
    return _db("yaw_wrap", dict(num_candidates=1, exclude_recent=1), descs, witness)


def _empty():
    R, S = 20, 60
    Z = np.zeros((R, S))
    B = dyadic(31, R, S); B[:, 5:15] = 0.0
    Q = dyadic(33, R, S); Q[:, 0:10] = 0.0
    descs = [dyadic(30, R, S), Z, B, dyadic(32, R, S), Z.copy(), Q]
    grid = grid_of()
    scans = [scan_of(d, **grid) if d.any() else far_scan(**grid) for d in descs]

    def witness(db, descs):
        L4, L3 = last_loop(db, 4), last_loop(db, 3)
        nq, nb = P.col_norms(descs[5]), P.col_norms(descs[2])
        return (all(len(s) > 0 for s in db_scene("empty").scans)
                and (P.shift_distances(descs[4], descs[0]) == 1.0).all()       # nv == 0 at every shift
                and L4 is not None and (L4["match"], L4["shift"], L4["d"]) == (0, 0, 1.0)
                and 1 in db.candidates(3) and L3 is not None and L3["match"] != 1 and L3["d"] < 1.0
                and 2 in db.candidates(5) and 1 in db.candidates(5)
                and ((nq == 0) & (nb != 0)).any() and ((nq != 0) & (nb == 0)).any() and ((nq == 0) & (nb == 0)).any())
    return _db("empty", dict(num_candidates=4, exclude_recent=1, dist_thres=2.0), descs, witness, scans=scans)


THRESHOLDS = ("at_d", "just_above_d", "far_below_d")


def _threshold(which):
    A = dyadic(40, 20, 60)
    B = noisy(41, roll(A, -4))
    d = float(P.shift_distances(B, A).min())
    thres = {"at_d": d, "just_above_d": float(np.nextafter(d, np.inf)), "far_below_d": 0.25 * d}[which]
    loops = {"at_d": 0, "just_above_d": 1, "far_below_d": 0}[which]

    def witness(db, descs):
        best = db.search(1)
        return (0.0 < d < 1.0 and best[0] == d and best[1] == 4 and len(db.loops) == loops
                and (loops == 0 or db.loops[0]["d"] == d))
    return _db(f"threshold_{which}", dict(num_candidates=1, exclude_recent=1, dist_thres=thres), [A, B], witness)


def _recent(ex):
    over = dict(n_rings=7, n_sectors=37, num_candidates=2, exclude_recent=ex, dist_thres=2.0)
    descs = [dyadic(50 + k, 7, 37) for k in range(6)]

    def witness(db, descs):
        m = [max(0, q - ex + 1) for q in range(6)]
        return ([len(db.candidates(q)) for q in range(6)] == [min(2, v) for v in m]
                and [L["query"] for L in db.loops] == [q for q in range(6) if m[q] > 0]
                and {(v > 2) - (v < 2) for v in m if v > 0} == {-1, 0, 1})   # num_candidates above, at and below m
    return _db(f"recent_{ex}", over, descs, witness)


GRIDS = ((1, 2), (7, 37), (20, 64), (20, 65), (64, 360), (20, 60))


def _grids(R, S):
    over = dict(n_rings=R, n_sectors=S, exclude_recent=1, dist_thres=2.0)
    if (R, S) == (7, 37):
        over.update(num_candidates=32, max_radius=50.0, height_offset=-1.5)
    D = dyadic(60 + R + S, R, S, lo=2)
    descs = [noisy(70 + k, roll(D, (3 * k) % S)) for k in range(6)]

    def witness(db, descs):
        want = min(over.get("num_candidates", P.DEFAULTS["num_candidates"]), 5)
        return (len(db.loops) == 5 and len(db.candidates(5)) == want and db.desc[0].shape == (R, S)
                and (R == 1 or any(L["shift"] != 0 for L in db.loops)))   # (one ring: every cosine is 1, every shift ties)
    return _db(f"grids_{R}x{S}", over, descs, witness)


MANY = 600
MANY_QUERIES = {594: (256, 512), 599: (512, MANY)}   # query -> the id range its nearest ring keys lie in


def _many():
    R, S = 4, 8
    over = dict(n_rings=R, n_sectors=S, num_candidates=32, exclude_recent=1, dist_thres=2.0)

    def family(k):   # ids 0 .. 255 far from everything later; 590 .. 594 look like 256 .. 511, 595 .. 599 like 512 .. 589
        if k < 256:
            return 192, 257
        if k < 512 or 590 <= k < 595:
            return 64, 129
        return 1, 33
    descs = [dyadic(1000 + k, R, S, *family(k)) for k in range(MANY)]

    def witness(db, descs):
        ok = len(db.desc) == MANY and len(db.loops) == MANY - 1
        for q, (lo, hi) in MANY_QUERIES.items():
            cand = db.candidates(q)
            near = [k for k in cand if lo <= k < hi]
            ok = ok and len(cand) == 32 and min(cand) >= 256 and len(near) >= 27
            # a rank pass that stopped at 256 keyframes would have returned other candidates
            kd = [P.key_distance(db.rkey[q], db.rkey[k]) for k in range(256)]
            ok = ok and min(kd) > max(P.key_distance(db.rkey[q], db.rkey[k]) for k in cand)
        return ok and last_loop(db, 599)["match"] >= 512 and 256 <= last_loop(db, 594)["match"]
    return _db("many", over, descs, witness, device=dict(reserve_keyframes=4))


DB_BUILDERS = dict(rank_ties=_rank_ties, shift_ties_halves=_shift_ties_halves, shift_ties_constant=_shift_ties_constant,
                   pick_ties_copies=_pick_ties_copies, pick_ties_shift=_pick_ties_shift,
                   pick_ties_distance=_pick_ties_distance, yaw_wrap=_yaw_wrap, empty=_empty)
DB_BUILDERS.update({f"threshold_{w}": functools.partial(_threshold, w) for w in THRESHOLDS})
DB_BUILDERS.update({f"recent_{ex}": functools.partial(_recent, ex) for ex in (1, 3)})
DB_BUILDERS.update({f"grids_{R}x{S}": functools.partial(_grids, R, S) for R, S in GRIDS})
DB_BUILDERS.update(many=_many)
DB_NAMES = tuple(DB_BUILDERS)


@functools.lru_cache(maxsize=None)
def db_scene(name) -> DbScene:
    return DB_BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def restated(name) -> P.PlaceDB:
    """the restatement's database after every scan of the scene (computed once; nothing changes it afterwards)"""
    sc = db_scene(name)
    db = P.PlaceDB(**sc.cfg)
    for f, s in enumerate(sc.scans):
        db.add(s, np.eye(4), FIRST_FRAME + f)
    return db
