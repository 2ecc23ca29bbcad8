"""-m gpu: loop verification on the hand-made keyframe sets of tests/loop_scenes.py.  Every scene goes
through place_add_scan, place_set_keyframe_clouds and loop_verify_pair and is compared bit for bit with expected(): the target
restated by tests/loop_np.py from the stored clouds and poses, the two matches through the public calls, the score summed in
the device's order (loop_np.score_device_order) and verify()'s status rules.  On top of that: the neighbouring window or the
filled hole gives other bits (a device that assembled the wrong window could not pass), the accept rule's >= / <=, the strict
inlier bound at d^2 == inlier_dist^2 exactly, a reach above 1 and an inlier_dist up to DBL_MAX, the status paths, both
init_modes on the loop records the place search finds among base's keyframes, and clouds set twice.

The only tolerances are the project's 0.05 m / 0.01 rad on `base`; everything else is bit equality or an exact count."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import loop_np as LN  # noqa: E402
import loop_scenes as LS  # noqa: E402
from tloam_amd.synth import Frame  # noqa: E402

pytestmark = pytest.mark.gpu

bits = LS.bits
SCALARS = ("status", "accepted", "inliers", "points")
FLOATS = ("init", "rel_pose", "overlap", "rmse")


# ---- the restatement -----------------------------------------------------------------------------------------------------
class Matchers:
    """the contexts expected() matches on, one per TLS configuration, kept for the module (a context costs more than a match)"""

    def __init__(self, reg):
        self.reg, self.ctx = reg, {}

    def get(self, cfg):
        key = bytes(cfg)
        if key not in self.ctx:
            self.ctx[key] = self.reg.HipRegistration(type(cfg).from_buffer_copy(key))
        return self.ctx[key]

    def close(self):
        for H in self.ctx.values():
            H.close()


@pytest.fixture(scope="module")
def matchers(hip_module):
    M = Matchers(hip_module)
    yield M
    M.close()


@pytest.fixture(scope="module")
def dev(hip_module):
    """the context under test, configured anew by every load()"""
    H = hip_module.HipRegistration()
    yield H
    H.close()


def loop_cfg(reg, sc, **over):
    if sc.window is not None:
        over.setdefault("window", sc.window)
    return reg.default_loop_config(enabled=1, **over)


def expected(reg, scene, q, m, loop_cfg, init, matchers):
    """what verify() gives for (q, m) of `scene` (its poses, the query's source clouds, the keyframes' target clouds) under
    loop_cfg from `init` (None: rigid_inverse(P_m) P_q)"""
    init = LN.t_rel(scene.poses[m], scene.poses[q]) if init is None else np.asarray(init, float)
    zero = reg.Stats().as_dict()
    e = {"status": 0, "accepted": False, "init": init, "rel_pose": init, "coarse": zero, "fine": zero, "inliers": 0, "points": 0,
         "overlap": 0.0, "rmse": 0.0}
    src = scene.src[q]
    tgt = LN.assemble(q, m, loop_cfg.window, scene.poses, scene.tgt)
    if sum(len(c) for c in src) == 0 or sum(len(c) for c in tgt) == 0:
        e["status"] = -6
        return e
    A, B = matchers.get(loop_cfg.coarse), matchers.get(reg.default_config())
    A.set_input_source(Frame(*src))
    A.set_input_target(Frame(*tgt))
    rc1, T1, st1 = A.scan_match(init)
    if rc1 not in (0, -7):
        e["status"] = rc1
        return e
    e["coarse"] = st1
    B.set_input_source(Frame(*src))
    B.set_input_target(Frame(*tgt))
    rc2, T2, st2 = B.scan_match(T1)
    e["status"] = rc1 if rc1 != 0 else rc2
    if rc2 not in (0, -7):
        e["rel_pose"] = T1
        return e
    e["fine"], e["rel_pose"] = st2, T2
    ov, rmse, inl, pts = LN.score_device_order(src, tgt, T2, loop_cfg.inlier_dist)
    e.update(overlap=ov, rmse=rmse, inliers=inl, points=pts,
             accepted=e["status"] == 0 and ov >= loop_cfg.min_overlap and rmse <= loop_cfg.max_rmse)
    return e


def same_stats(got, want, what):
    for k in want:
        if k != "host_wait_us":
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (what, k, got[k], want[k])


def same(c, e, what, but=()):
    """a constraint against an expectation (or another constraint): every field the two share, bit for bit"""
    for k in SCALARS:
        if k not in but:
            assert c[k] == e[k], (what, k, c[k], e[k])
    for k in FLOATS:
        if k not in but:
            assert bits(c[k]) == bits(e[k]), (what, k, c[k], e[k])
    same_stats(c["coarse"], e["coarse"], (what, "coarse"))
    same_stats(c["fine"], e["fine"], (what, "fine"))


def differs(a, b):
    """two expectations are told apart by the fine match's cost or the score"""
    return bits(a["fine"]["solver_cost"]) != bits(b["fine"]["solver_cost"]) or bits(a["rmse"]) != bits(b["rmse"])


# ---- a scene onto the device ---------------------------------------------------------------------------------------------
def load(H, sc, cfg, **place):
    H.place_configure(enabled=1, **place)   # (the default search looks 50 keyframes back: no records unless `place` says so)
    H.loop_configure(cfg)
    for k in range(len(sc.poses)):
        assert H.place_add_scan(LS.scan_of(sc, k), sc.poses[k], 100 + k) == k
        H.place_set_keyframe_clouds(k, sc.src[k], sc.tgt[k])
    assert H.loop_info()["arena_points"] == sum(len(c) for k in range(len(sc.poses)) for c in sc.src[k] + sc.tgt[k])


def stored(H, sc, q, m, window):
    """the scene as the device holds it: the poses and the window's and the query's clouds read back (they are the scene's)"""
    poses = H.place_read_keyframes()["poses"]
    assert bits(poses) == bits(sc.poses)
    src, tgt = [list(s) for s in sc.src], [list(t) for t in sc.tgt]
    for k in set(LN.window(q, m, window)) | {q}:
        got = H.place_read_keyframe_clouds(k)
        for kind in range(4):
            assert bits(got[0][kind]) == bits(sc.src[k][kind]) and bits(got[1][kind]) == bits(sc.tgt[k][kind]), (k, kind)
        src[k], tgt[k] = got
    return sc._replace(poses=poses, src=src, tgt=tgt)


def verify(reg, H, sc, matchers, q=None, m=None, init=None, **over):
    """(the device's constraint, the expectation) for the scene's pair under the scene's window and `over`"""
    q, m = sc.q if q is None else q, sc.m if m is None else m
    cfg = loop_cfg(reg, sc, **over)
    load(H, sc, cfg)
    c = H.loop_verify_pair(q, m, init)
    assert (c["query"], c["match"], c["query_frame"], c["match_frame"]) == (q, m, 100 + q, 100 + m)
    assert H.loop_info()["n_constraints"] == 0   # (pairs are not appended)
    e = expected(reg, stored(H, sc, q, m, cfg.window), q, m, cfg, init, matchers)
    print(f"{sc.name} ({q}, {m}) window {cfg.window}: status {c['status']} accepted {c['accepted']} inliers {c['inliers']} / "
          f"{c['points']} overlap {c['overlap']!r} rmse {c['rmse']!r} (expected {e['status']} {e['inliers']} {e['rmse']!r}) "
          f"fine cost {c['fine']['solver_cost']!r}")
    return c, e, cfg


# ---- every scene ------------------------------------------------------------------------------------------------------------
# the other window (or the hole filled) whose expectation must differ from the right one
NEIGHBOUR = {"clip_low": dict(window=2), "clip_high": dict(window=2), "window_zero": dict(window=1), "holes": dict(filled=True)}
NEIGHBOUR_TOO = {"clip_low": dict(window=4), "clip_high": dict(window=4)}


@pytest.mark.parametrize("name", LS.NAMES)
def test_scene_equals_the_restatement(hip_module, dev, matchers, name):
    reg, sc = hip_module, LS.scene(name)
    c, e, cfg = verify(reg, dev, sc, matchers)
    same(c, e, name)
    if name == "nine_sphere":
        assert c["status"] == -2 and not c["accepted"] and bits(c["rel_pose"]) == bits(c["init"])
        assert bits(c["init"]) == bits(LN.t_rel(sc.poses[sc.m], sc.poses[sc.q]))
    else:
        assert c["status"] in (0, -7) and c["points"] == sum(len(x) for x in sc.src[sc.q]) and c["inliers"] > 0
    for other in (NEIGHBOUR.get(name), NEIGHBOUR_TOO.get(name)):
        if other is None:
            continue
        if other.get("filled"):
            wrong = expected(reg, sc._replace(tgt=sc.filled), sc.q, sc.m, cfg, None, matchers)
        else:
            wrong = expected(reg, sc, sc.q, sc.m, loop_cfg(reg, sc, **other), None, matchers)
        assert wrong["status"] in (0, -7) and differs(wrong, e), (name, other)


def test_spread_sphere_runs_by_the_clamp_alone(hip_module, dev, matchers):
    reg, sc = hip_module, LS.scene("spread_sphere")
    for m, w, total in LS.SPREAD_RUNS:
        c, e, _ = verify(reg, dev, sc, matchers, m=m, window=w)
        same(c, e, (m, w))
        if total >= LS.MIN_POINTS:
            assert c["status"] in (0, -7) and c["points"] > 0
        else:
            assert c["status"] == -2 and not c["accepted"] and bits(c["rel_pose"]) == bits(c["init"]) and c["points"] == 0


# ---- base: right, and the rules around its score ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base_run(hip_module, dev, matchers):
    sc = LS.scene("base")
    c, e, cfg = verify(hip_module, dev, sc, matchers)
    same(c, e, "base")
    return sc, c


def test_base_at_the_defaults_is_accepted_and_right(base_run):
    sc, c = base_run
    truth = np.linalg.inv(sc.poses[sc.m]) @ sc.poses[sc.q]
    err = np.linalg.inv(truth) @ c["rel_pose"]
    dt = np.linalg.norm(err[:3, 3])
    da = np.arccos(np.clip((np.trace(err[:3, :3]) - 1) / 2, -1, 1))
    print(f"base: {dt:.5f} m {da:.6f} rad overlap {c['overlap']:.4f} rmse {c['rmse']:.4f}")
    assert c["status"] == 0 and c["accepted"], c
    assert dt <= 0.05 and da <= 0.01, (dt, da)   # (the bounds of test_true_revisits_are_accepted_and_right)


def test_accept_rule_at_its_edges(hip_module, dev, matchers, base_run):
    sc, first = base_run
    o, r = first["overlap"], first["rmse"]
    assert 0.0 < o < 1.0 and 0.0 < r < np.inf
    for over, accepted in ((dict(min_overlap=o), True), (dict(min_overlap=float(np.nextafter(o, 2.0))), False),
                           (dict(max_rmse=r), True), (dict(max_rmse=float(np.nextafter(r, 0.0))), False)):
        c, e, _ = verify(hip_module, dev, sc, matchers, **over)
        assert c["accepted"] is accepted, over
        same(c, e, over)
        same(c, first, over, but=("accepted",))


def test_inlier_bound_is_strict(hip_module, dev, matchers, base_run):
    sc, first = base_run
    src, tgt = sc.src[sc.q], LN.assemble(sc.q, sc.m, LS.DEFAULT_WINDOW, sc.poses, sc.tgt)
    d2 = np.sort(np.concatenate([LN.nearest_d2(LN.move(first["rel_pose"], src[k]), tgt[k]) for k in range(4)]))
    root = np.sqrt(d2)
    ok = np.zeros(len(d2), bool)
    ok[1:-1] = (root[1:-1] * root[1:-1] == d2[1:-1]) & (d2[:-2] < d2[1:-1]) & (d2[1:-1] < d2[2:]) & (d2[1:-1] > 0.0)
    assert ok.any()
    i = int(np.flatnonzero(ok)[np.argmin(np.abs(np.flatnonzero(ok) - len(d2) // 2))])   # (the one nearest the median)
    v, s = float(d2[i]), float(root[i])
    up = float(np.nextafter(s, np.inf))
    assert s * s == v and up * up > v
    runs = []
    for dist, inside in ((s, False), (up, True)):
        assert (v < dist * dist) is inside
        c, e, _ = verify(hip_module, dev, sc, matchers, inlier_dist=dist)
        same(c, e, dist)
        assert c["inliers"] == int((d2 < dist * dist).sum()) and (c["inliers"] > i if inside else c["inliers"] == i)
        same(c, first, dist, but=("accepted", "inliers", "overlap", "rmse"))   # (the matches do not depend on inlier_dist)
        runs.append(c)
    assert runs[1]["inliers"] > runs[0]["inliers"]


def test_reach_above_one(hip_module, dev, matchers, base_run):
    sc, first = base_run
    c, e, _ = verify(hip_module, dev, sc, matchers, inlier_dist=5.0)   # (cells of 0.5 m and 1 m: a reach of 10 and of 5)
    same(c, e, 5.0)
    same(c, first, 5.0, but=("accepted", "inliers", "overlap", "rmse"))
    assert c["inliers"] > first["inliers"]
    # far_points: ten source points 3 to 5 m from every target of their kind, which only a walk beyond the 27 cells finds
    far = LS.scene("far_points")
    near, _, _ = verify(hip_module, dev, far, matchers)
    c, e, _ = verify(hip_module, dev, far, matchers, inlier_dist=LS.FAR_MAX)
    same(c, e, "far")
    same(c, near, "far", but=("accepted", "inliers", "overlap", "rmse"))
    assert near["inliers"] <= near["points"] - LS.FAR_N and c["inliers"] == c["points"] == sum(LS.BASE_N) + LS.FAR_N


@pytest.mark.parametrize("name", ("base", "far_points"))
@pytest.mark.parametrize("dist", (1e13, 1e200, sys.float_info.max))
def test_inlier_dist_beyond_any_int(hip_module, dev, matchers, dist, name):
    """inlier_dist / cell past INT_MAX: the reach is formed in double and bounded by the grid, so every target is walked.  (The
    cast used to be undefined there -- INT_MIN on x86-64, hence a reach of 1 -- and far_points' ten points, cells away from
    every target, were not inliers whatever the distance.)"""
    sc = LS.scene(name)
    first, _, _ = verify(hip_module, dev, sc, matchers)
    c, e, _ = verify(hip_module, dev, sc, matchers, inlier_dist=dist, max_rmse=1e300)
    same(c, e, dist)
    same(c, first, dist, but=("accepted", "inliers", "overlap", "rmse"))
    assert c["inliers"] == c["points"] == sum(len(x) for x in sc.src[sc.q]) and c["overlap"] == 1.0 and c["accepted"]


# ---- status paths -------------------------------------------------------------------------------------------------------------
def test_status_paths(hip_module, dev, matchers):
    reg, sc = hip_module, LS.scene("base")
    stretched = np.eye(4)
    stretched[:3, :3] *= 2.0                      # finite, not rigid
    c, e, _ = verify(reg, dev, sc, matchers, init=stretched)
    same(c, e, "2 I")
    assert c["status"] == -3 and not c["accepted"] and bits(c["rel_pose"]) == bits(stretched) == bits(c["init"])
    for bad in (np.nan, np.inf, -np.inf):
        T = np.eye(4)
        T[1, 3] = bad
        with pytest.raises(reg.TloamHipError, match="TLOAM_E_INVALID"):
            dev.loop_verify_pair(sc.q, sc.m, T)
    n = len(sc.poses)
    for q, m in ((5, 5), (4, 5), (5, -1), (n, 5), (n + 7, 0)):
        with pytest.raises(reg.TloamHipError, match="TLOAM_E_INVALID"):
            dev.loop_verify_pair(q, m)
    assert dev.loop_info()["n_constraints"] == 0 and dev.loop_verify_pair(n - 1, 0)["points"] == sum(LS.BASE_N)


# ---- init_mode, on loop records ----------------------------------------------------------------------------------------------
# The records are those the place search finds among base's own keyframes once exclude_recent lets it look (LS.PLACE_FOR_LOOPS;
# tests/test_loop_scenes.py counts them on the restatement).  The out-and-back pass of tests/test_gpu_loop.py would give records
# too, but its module fixture is built again for every module that asks for it -- 39 s of scan generation, measured -- which no
# test here is worth; what is checked does not depend on where the records come from.
@pytest.mark.parametrize("mode", (0, 1))
def test_init_modes(hip_module, dev, matchers, mode):
    reg, sc = hip_module, LS.scene("base")
    cfg = loop_cfg(reg, sc, init_mode=mode)
    load(dev, sc, cfg, **LS.PLACE_FOR_LOOPS)
    n = dev.loop_verify_pending()
    loops, cons = dev.place_loops(), dev.loop_constraints()
    assert n == len(loops) == len(cons) >= 5 and dev.loop_info()["n_constraints"] == n
    assert len({L["yaw"] for L in loops}) >= 4 and max(abs(L["yaw"]) for L in loops) > 1.0
    for L, c in zip(loops, cons):
        q, m = L["query"], L["match"]
        assert (c["query"], c["match"], c["d"], c["yaw"]) == (q, m, L["d"], L["yaw"])
        if mode == 0:   # Rz(yaw), no translation (the host's cos / sin and Python's math are the same libm's: bit for bit)
            cy, sy = math.cos(L["yaw"]), math.sin(L["yaw"])
            init = np.array([[cy, -sy, 0.0, 0.0], [sy, cy, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
        else:           # rigid_inverse(P_m) P_q of the stored poses
            init = LN.t_rel(sc.poses[m], sc.poses[q])
        assert bits(c["init"]) == bits(init), (mode, q, m)
        same(c, expected(reg, sc, q, m, cfg, init, matchers), (mode, q, m))
        if mode == 1:   # init None is mode 1
            same(dev.loop_verify_pair(q, m), c, ("pair", q, m))
    assert dev.loop_info()["n_constraints"] == n   # (pairs are not appended)


# ---- clouds set twice ---------------------------------------------------------------------------------------------------------
def test_replaced_clouds_are_the_ones_verified(hip_module, dev, matchers):
    reg, sc = hip_module, LS.scene("base")
    cfg = loop_cfg(reg, sc)
    load(dev, sc, cfg)
    k = sc.m
    sets = [([LS.cloud(seed, k, 0, kind, LS.BASE_N[kind] + 17 * seed, sc.poses[k]) for kind in range(4)],
             [LS.cloud(seed, k, 1, kind, LS.BASE_N[kind] + 13 * seed, sc.poses[k]) for kind in range(4)]) for seed in (98, 99)]
    for src, tgt in sets:
        dev.place_set_keyframe_clouds(k, src, tgt)
    got = dev.place_read_keyframe_clouds(k)
    for kind in range(4):
        assert bits(got[0][kind]) == bits(sets[1][0][kind]) and bits(got[1][kind]) == bits(sets[1][1][kind])
        assert bits(got[1][kind]) != bits(sc.tgt[k][kind])
    second = sc._replace(src=[sets[1][0] if j == k else s for j, s in enumerate(sc.src)],
                         tgt=[sets[1][1] if j == k else t for j, t in enumerate(sc.tgt)])
    for q, m in ((sc.q, k), (k, 2)):   # keyframe k as a target of the window, and as the query
        c = dev.loop_verify_pair(q, m)
        e = expected(reg, stored(dev, second, q, m, cfg.window), q, m, cfg, None, matchers)
        same(c, e, (q, m))
        assert c["status"] == 0 and c["points"] == sum(len(x) for x in second.src[q])
        assert differs(e, expected(reg, sc, q, m, cfg, None, matchers))   # (the first clouds give other bits)
