"""The clearance's restatement (tests/closed_map_clearance_np.py) without a GPU: the transform against a
brute-force all-pairs minimum and against scipy's exact Euclidean transform, the wall scene's figures as integers, and the
segment walk on single hand-made rays."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import carve_scenes as CS  # noqa: E402
import closed_map_carve_np as CN  # noqa: E402
import closed_map_clearance_np as KN  # noqa: E402
import closed_map_free_np as FN  # noqa: E402
import localise_scenes as LS  # noqa: E402

B, O = KN.BEYOND, KN.OUTSIDE


def brute(obstacle, R, wrap):
    """min over every obstacle cell of the squared distance, all pairs; with `wrap` everything outside is one, R layers deep"""
    obstacle = np.asarray(obstacle, bool)
    if wrap:
        obstacle = np.pad(obstacle, R, constant_values=True)
    obs = np.argwhere(obstacle)
    cells = np.argwhere(np.ones(obstacle.shape, bool))
    if len(obs):
        d2 = ((cells[:, None, :] - obs[None, :, :]) ** 2).sum(axis=2).min(axis=1)
    else:
        d2 = np.full(len(cells), B, np.int64)
    d2 = np.where(d2 <= R * R, d2, B).astype(np.uint16).reshape(obstacle.shape)
    return d2[(slice(R, -R),) * d2.ndim] if wrap else d2


@pytest.mark.parametrize("wrap", [False, True])
def test_the_transform_is_the_all_pairs_minimum(wrap):
    rng = np.random.default_rng(3)
    for shape, density in (((7, 6, 5), 0.05), ((4, 4, 12), 0.02), ((9, 8), 0.1), ((3, 3, 3), 0.0), ((1, 1, 1), 1.0)):
        obstacle = rng.random(shape) < density
        for R in (1, 2, 3, 7):
            got = KN.transform(obstacle, R, wrap)
            assert got.dtype == np.uint16 and got.tobytes() == brute(obstacle, R, wrap).tobytes(), (shape, R)
    # the truncation edge: R * R is stored, R * R + 1 is not
    line = np.zeros((1, 1, 12), bool)
    line[0, 0, 0] = True
    assert KN.transform(line, 3, False)[0, 0].tolist() == [0, 1, 4, 9] + [B] * 8
    two = np.zeros((1, 4, 4), bool)
    two[0, 0, 0] = True
    assert KN.transform(two, 3, False)[0].tolist() == [[0, 1, 4, 9], [1, 2, 5, B], [4, 5, 8, B], [9, B, B, B]]
    assert (KN.transform(np.zeros((3, 4, 5), bool), 2, False) == B).all()
    assert KN.transform(np.zeros((3, 3, 3), bool), 2, True)[1].tolist() == [[1, 1, 1], [1, 4, 1], [1, 1, 1]]


def test_the_transform_is_scipys_exact_one():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    for shape in ((20, 17, 13), (5, 40, 8)):
        obstacle = rng.random(shape) < 0.01
        for R in (1, 3, 7):
            for wrap in (False, True):
                pad = np.pad(obstacle, R, constant_values=True) if wrap else obstacle
                d = ndi.distance_transform_edt(~pad) if pad.any() else np.full(pad.shape, np.inf)
                with np.errstate(invalid="ignore"):
                    d2 = np.rint(d * d)
                want = np.where(d2 <= R * R, d2, B).astype(np.uint16)
                if wrap:
                    want = want[R:-R, R:-R, R:-R]
                assert KN.transform(obstacle, R, wrap).tobytes() == want.tobytes(), (shape, R, wrap)


def test_the_host_arithmetic():
    assert [KN.radius_cells(m, 0.5) for m in (4.0, 4.0000001, 3.9999999, 0.5, 0.4, 64.0, 64.1, 0.0, np.nan, np.inf)] \
        == [8, 9, 8, 1, 1, 128, None, None, None, None]
    assert [KN.need_d2(r, 0.5, 8) for r in (0.0, 0.5, 1.0, 1.25, 4.0, 4.03, 4.04, -1.0, np.nan, np.inf)] \
        == [0, 1, 4, 7, 64, 65, None, None, None, None]


@pytest.fixture(scope="module")
def wall():
    poses, clouds, _, _ = LS.wall()
    V = CN.build_map(poses, clouds, CS.MASK, 0.5)
    G = FN.FreeNP(V, max_range=12.0, end_margin=1.0)
    assert G.reset(poses=poses)
    G.add_keyframes(poses, clouds, CS.MASK)
    return G


def field(G, **cfg):
    K = KN.ClearNP(G, **cfg)
    assert K.build()
    return K


PROBES = np.array([(6, 2, 1.5), (6, 3.9, 1.5), (6, 0, 1.5), (6, 5.2, 1.5), (6, 4.7, 1.5), (6, 7, 1.5)], np.float64)


def test_the_wall(wall):
    K = field(wall, max_distance=4.0, unknown_is_obstacle=0)
    assert K.d2.shape == (56, 56, 76) and K.R == 8
    s = K.states
    assert [int((s == k).sum()) for k in (FN.UNKNOWN, FN.FREE, FN.OCCUPIED)] == [237286, 875, 175]
    table = {(4, 0): (175, 3023, 22548, 16, 475), (8, 0): (175, 10467, 324336, 64, 791), (4, 1): (237461, 238336, 1776, 9, 875),
             (8, 1): (237461, 238336, 1776, 9, 875)}
    for (R, wrap), want in table.items():
        K = field(wall, max_distance=0.5 * R, unknown_is_obstacle=wrap)
        info = K.info()
        got = (info["obstacle_cells"], info["finite_cells"], info["sum_d2"], info["max_d2"],
               int((K.d2[K.states == FN.FREE] != B).sum()))
        assert got == want and info["radius_cells"] == R and info["bytes"] == 4 * 76 * 56 * 56, (R, wrap, got)
    # section 29's probe points
    state, d2, dist, counts = field(wall, unknown_is_obstacle=0).points(PROBES)
    assert d2.tolist() == [36, 9, B, 0, 1, 16] and list(counts) == [0, 2, 3, 1]
    assert dist.tolist() == [3.0, 1.5, np.inf, 0.0, 0.5, 2.0]
    state1, d2, dist, _ = field(wall, unknown_is_obstacle=1).points(PROBES)
    assert d2.tolist() == [4, 4, 1, 0, 0, 0] and state1.tobytes() == state.tobytes()
    # ... a point outside the box and one no cell holds
    K0, K1 = field(wall, unknown_is_obstacle=0), field(wall, unknown_is_obstacle=1)
    far = np.array([(6, 40, 1.5), (np.nan, 0, 0)])
    for K, want in ((K0, [O, O]), (K1, [0, O])):
        state, d2, dist, _ = K.points(far)
        assert d2.tolist() == want and state.tolist() == [FN.UNKNOWN, FN.INVALID]
        assert np.isnan(dist[1]) and (np.isnan(dist[0]) if want[0] == O else dist[0] == 0.0)


def test_the_walls_columns(wall):
    state = wall.columns(0.5, 2.9)
    assert state.shape == (56, 76) and [int((state == k).sum()) for k in (FN.UNKNOWN, FN.FREE, FN.OCCUPIED)] == [4016, 215, 25]
    for wrap, want in ((0, (605, 15976, 64)), (1, (4256, 1674, 25))):
        K = KN.ClearNP(wall, unknown_is_obstacle=wrap)
        got_state, d2 = K.columns(0.5, 2.9)
        fin = d2[d2 != B].astype(np.int64)
        assert got_state.tobytes() == state.tobytes() and (len(fin), int(fin.sum()), int(fin.max())) == want
    assert KN.ClearNP(wall, max_distance=100.0).columns(0.5, 2.9) is None        # R = 200


def test_refused_builds(wall):
    assert not KN.ClearNP(wall, max_distance=64.1).build() and KN.ClearNP(wall, max_distance=64.0).build()
    cells = 76 * 56 * 56
    assert not KN.ClearNP(wall, max_bytes=4 * cells - 1).build() and KN.ClearNP(wall, max_bytes=4 * cells).build()


def bits(x):
    return np.asarray(x, np.float64).tobytes()


def test_segments_on_single_rays(wall):
    """the sensor's cell is (12, 0, 2); the wall fills the cells y = 10; the box is y = -28 .. 27"""
    K0, K1 = field(wall, unknown_is_obstacle=0), field(wall, unknown_is_obstacle=1)
    t = np.array([6.25, 0.25, 1.25])      # a cell centre
    one = lambda K, S, E, r: [a[0] for a in K.segments(np.asarray(S, np.float64)[None], np.asarray(E, np.float64)[None], r)[:3]]  # noqa: E731
    # along the wall, two cells in front of it (the cells y = 8: d2 = 4): a body of two cells passes, one of 2.5 does not
    S, E = (2.25, 4.25, 1.25), (8.25, 4.25, 1.25)
    assert one(K0, S, E, 1.0) == [KN.CLEAR, 4, -1.0] and one(K0, S, E, 1.25) == [KN.BLOCKED, 4, 0.0]
    # into the wall: 16 cells along y, cell k entered at (k - 0.5) / 16; d2 = (10 - k)^2
    E = t + [0.0, 8.0, 0.0]
    assert one(K0, t, E, 0.5) == [KN.BLOCKED, 0, 9.5 / 16] and one(K0, t, E, 1.0) == [KN.BLOCKED, 1, 8.5 / 16]
    assert one(K0, t, E, 1.01) == [KN.BLOCKED, 4, 7.5 / 16] and one(K0, t, E, 4.0) == [KN.BLOCKED, 49, 2.5 / 16]
    assert one(K0, t, E, 0.0) == [KN.CLEAR, 0, -1.0]                                # need = 0 never blocks
    # from free space up into unknown: cell z = 2 + k entered at (k - 0.5) / 8
    status, least, tb = one(K1, t, t + [0.0, 0.0, 4.0], 0.5)
    assert status == KN.BLOCKED and least == 0 and tb in [(k - 0.5) / 8 for k in range(1, 9)]
    assert K1.points(t[None] + [0.0, 0.0, 0.5 * (8 * tb + 0.5)])[0][0] == FN.UNKNOWN    # the cell it stopped in
    assert K1.points(t[None] + [0.0, 0.0, 0.5 * (8 * tb - 0.5)])[0][0] == FN.FREE       # ... and the one before
    assert one(K0, t, t + [0.0, 0.0, 4.0], 0.5) == [KN.CLEAR, B, -1.0]
    # out of the box: 32 cells down y, the first outside cell y = -29 entered at 28.5 / 32
    E = t - [0.0, 16.0, 0.0]
    assert one(K0, t, E, 0.5) == [KN.LEFT_BOX, B, 28.5 / 32] and one(K0, t, E, 0.0) == [KN.LEFT_BOX, B, 28.5 / 32]
    assert one(K1, t, E, 0.0) == [KN.CLEAR, 0, -1.0] and one(K1, t, E, 0.5)[:2] == [KN.BLOCKED, 0]
    # inside one cell: the one cell is the walk
    E = t + [0.125, 0.0625, -0.125]
    assert one(K0, t, E, 4.0) == [KN.CLEAR, B, -1.0] and one(K1, t, E, 0.5) == [KN.CLEAR, 1, -1.0]
    assert one(K1, t, E, 0.75) == [KN.BLOCKED, 1, 0.0]
    # skipped: not finite, zero length, beyond max_segment, beyond the grid
    for E in ([np.nan, 0.0, 0.0], [np.inf, 0.0, 0.0], t, t + [0.0, 130.0, 0.0], [2.0 ** 19 + 5.0, 0.0, 0.0]):
        assert one(K0, t, E, 0.5) == [KN.SKIPPED, O, -1.0]
    # the largest radius the field vouches for, and one step beyond
    assert K0.segments(t[None], (t + [0.0, 8.0, 0.0])[None], 4.03)[1][0] == 64 and K0.segments(t[None], t[None], 4.04) is None
    assert K0.segments(t[None], t[None], -0.1) is None and K0.segments(t[None], t[None], np.nan) is None
    # a batch's counts, and a pose
    S = np.tile(t, (5, 1))
    E = np.array([t + [0.0, 8.0, 0.0], t - [0.0, 16.0, 0.0], t + [0.125, 0.0625, -0.125], t, (2.25, 4.25, 1.25)])
    status, least, tb, counts = K0.segments(S, E, 0.5)
    assert status.tolist() == [KN.BLOCKED, KN.LEFT_BOX, KN.CLEAR, KN.SKIPPED, KN.CLEAR] and counts.tolist() == [1, 2, 1, 1]
    pose = np.eye(4)
    pose[:3, 3] = [0.5, -0.25, 0.0]
    moved = K0.segments(S - pose[:3, 3], E - pose[:3, 3], 0.5, pose)
    assert moved[0].tobytes() == status.tobytes() and moved[1].tobytes() == least.tobytes() and bits(moved[2]) == bits(tb)
