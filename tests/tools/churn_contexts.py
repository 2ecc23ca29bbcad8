#!/usr/bin/env python3
"""TEST TOOL (GPU box): contexts created and destroyed in quick succession, each handed the device memory of a dead one.

The round-5 bug this hunts for relatives of: a new context finding valid-looking hand-over rows of a dead context in its recycled
row buffer (tests/test_gpu_parity.py::test_contexts_following_each_other_never_see_each_others_rows runs twenty successions; this
runs as many as asked for, over scenes of different sizes and through BOTH drivers of the outer loop, and also keeps a second,
long-lived context solving between the successions so that allocations interleave).  Every result must reproduce the first pass
over its scene bit for bit (one-call driver) / to 1e-12 (stepwise driver: different finish kernel, same sums); no call may fail or
take anywhere near the second a timed-out hand-over costs.

A second phase churns whole-pipeline contexts: every round creates a context, configures every optional store with a reserve of at
least PIPE_STORE_MB (global map, voxel map, place recognition, loop verification's keyframe-cloud arena, closed map; the deskew on),
runs a short odometry sequence that makes keyframes, verifies a pair (the two child contexts come to life), optimises the graph,
builds the closed map, reads from every store and destroys the context.  The footprint measure and its 256 MB bounds are the first
phase's, the baseline taken after the first quarter of the rounds; the rounds are refused unless
(rounds after the baseline) x PIPE_STORE_MB >= 512 MB, so that one configured store leaked per round cannot stay under the bound.
(The deskew's and the graph's buffers are sized by the scan and the keyframes, a few MB: a leak of those alone takes more rounds
to show than the standing test runs.)  Every round's poses, constraint and closed map must be those of the first round bit for bit.

    python tests/tools/churn_contexts.py [successions=400] [pipeline_rounds=24]      (0 skips a phase)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tloam_amd import registration as reg, synth  # noqa: E402


def pose_delta(A, B):
    D = np.linalg.inv(A) @ B
    R = D[:3, :3]
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * 0.5
    return float(np.linalg.norm(D[:3, 3])), float(np.arctan2(np.linalg.norm(w), (np.trace(R) - 1.0) * 0.5))


def footprint():
    """(free device memory, resident host memory of this process) in MB"""
    import resource
    import torch
    free, _ = torch.cuda.mem_get_info(0)
    return free / 2**20, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0


def churn_solves(n):
    scenes = [synth.make_scene(seed=41), synth.make_scene(seed=33),
              synth.make_scene(seed=7, n_src=synth.KITTI_SRC, n_tgt=synth.KITTI_TGT),
              synth.make_scene(seed=8, n_src=synth.KITTI_SRC, n_tgt=synth.KITTI_TGT, pred_err=(0.05, -0.02, 0.01, 0.004, -0.002, 0.006)),
              synth.make_scene(seed=9, n_src=(40_000, 50_000, 35_000, 8_000), n_tgt=(30_000, 30_000, 20_000, 5_000))]
    keys = ("gn_evaluations", "gn_iterations", "accepted_steps", "outer_iterations", "n_corr", "converged_early")

    def counters(st):
        return tuple(int(x) for k in keys for x in np.atleast_1d(st[k]))

    want = []
    for sc in scenes:
        H = reg.HipRegistration()
        H.set_frames(sc.source, sc.target)
        rc, T, st = H.scan_match(sc.T_pred)
        assert rc == 0, rc
        want.append((T.copy(), counters(st)))
        H.close()
    keeper = reg.HipRegistration()
    keeper.set_frames(scenes[2].source, scenes[2].target)
    worst = 0.0
    t_start = time.time()

    base = None
    for i in range(n):
        if i == min(200, n // 4):     # (allocator pools, the HIP runtime's own caches and the largest scene have been seen by now)
            base = footprint()
        k = (i * 7 + i // 5) % len(scenes)
        sc, (T_want, c_want) = scenes[k], want[k]
        H = reg.HipRegistration()
        H.set_frames(sc.source, sc.target)
        reps = 1 + i % 3
        for r in range(reps):
            t0 = time.perf_counter()
            if (i + r) % 2 == 0:
                rc, T, st = H.scan_match(sc.T_pred)
                assert rc == 0, (i, r, rc)
                assert T.tobytes() == T_want.tobytes() and counters(st) == c_want, ("one-call", i, r, k)
            else:
                assert H.sm_begin(sc.T_pred) == 0
                done = False
                while not done:
                    rc, done, st = H.sm_outer()
                    assert rc == 0, (i, r, rc)
                rc, T, st = H.sm_end()
                assert rc == 0 and counters(st) == c_want, ("stepwise", i, r, k)
                dt, dr = pose_delta(T, T_want)
                assert dt < 1e-12 and dr < 1e-12, ("stepwise", i, r, k, dt, dr)
            worst = max(worst, time.perf_counter() - t0)
        if i % 4 == 0:   # the long-lived context between two short-lived ones
            rc, T, st = keeper.scan_match(scenes[2].T_pred)
            assert rc == 0 and T.tobytes() == want[2][0].tobytes() and counters(st) == want[2][1], ("keeper", i)
        H.close()
    keeper.close()
    if base is not None:
        end = footprint()
        print("footprint after %d successions: device free %.0f -> %.0f MB, host peak RSS %.0f -> %.0f MB" % (n, base[0], end[0], base[1], end[1]))
        assert base[0] - end[0] < 256.0, "device memory is leaking: %.0f MB in %d successions" % (base[0] - end[0], n - min(200, n // 4))
        assert end[1] - base[1] < 256.0, "host memory is leaking: %.0f MB" % (end[1] - base[1])
    print("churn ok: %d successions over %d scenes in %.1f s, slowest call %.1f ms" % (n, len(scenes), time.time() - t_start, worst * 1e3))
    assert worst < 0.5, worst


# ---- the second phase: whole-pipeline contexts ------------------------------------------------------------------------------
PIPE_STORE_MB = 64          # every configured store reserves at least this much device memory (sizes below)
PIPE_RESERVE = dict(
    map_points=1 << 22,     # x, y, z doubles: 96 MiB
    voxels=1 << 21,         # voxel map and closed map: 40 B of rows + 8 B of table per voxel: 96 MiB each
    keyframes=8192,         # 20 x 60 descriptor doubles + keys + pose per keyframe: 80 MiB
    arena_points=1 << 22,   # three doubles per point: 96 MiB
)
PIPE_FEATURE = dict(radius=0.5, cvr_submap=0.05)   # (the feature settings of tests/test_gpu_loop.py's odometry runs)
PIPE_FRAMES = 7


def pipeline_round(scans):
    """one context through the whole pipeline -> everything it computed, as bytes"""
    R = PIPE_RESERVE
    H = reg.HipRegistration()
    H.map_configure(enabled=1, reserve_points=R["map_points"])
    H.voxel_map_configure(enabled=1, reserve_voxels=R["voxels"])
    H.deskew_configure(enabled=1)
    H.place_configure(enabled=1, kf_dist=2.0, exclude_recent=2, reserve_keyframes=R["keyframes"])
    H.loop_configure(enabled=1, reserve_points=R["arena_points"])
    H.closed_map_configure(reserve_voxels=R["voxels"])
    H.odometry_reset(None, reg.default_odom_config(**{f"feature__{k}": v for k, v in PIPE_FEATURE.items()}))
    out = []
    for f, xyz in enumerate(scans):
        rc, T, _ = H.odometry_frame(xyz)
        assert rc in (0, -7), (f, rc)
        out.append(T)
    n_kf = H.place_info()["n_keyframes"]
    assert n_kf >= 2, n_kf
    H.loop_verify_pending()
    pair = H.loop_verify_pair(n_kf - 1, 0)
    assert pair["status"] == 0 and pair["points"] > 0, pair
    ginfo = H.graph_optimize()
    assert ginfo["n_nodes"] == n_kf, ginfo
    cinfo = H.closed_map_build(1)
    assert cinfo["n_voxels"] > 0, cinfo
    # something from every store
    assert H.map_info()["capacity_points"] >= R["map_points"] and H.voxel_map_info()["capacity_voxels"] >= R["voxels"]
    assert H.place_info()["capacity_keyframes"] >= R["keyframes"] and H.loop_info()["arena_capacity_points"] >= R["arena_points"]
    assert H.closed_map_info()["capacity_voxels"] >= R["voxels"]
    assert H.deskew_info()["frames_deskewed"] > 0
    out += [H.map_read(), *H.voxel_map_read(), H.registered_scan(), H.place_read_keyframes()["poses"],
            *H.place_read_keyframe_clouds(n_kf - 1)[1], pair["rel_pose"], H.graph_poses(), *H.closed_map_read(), H.closed_map_poses()]
    H.close()
    return [np.ascontiguousarray(a).tobytes() for a in out]


def churn_pipelines(rounds):
    from tloam_amd import synth_hdl64
    first = max(rounds // 4, 1)     # (the baseline: allocator pools and the runtime's caches have seen a whole context by now)
    assert (rounds - first) * PIPE_STORE_MB >= 512, \
        "%d rounds after the baseline x %d MB: a store leaked per round could stay under the bound" % (rounds - first, PIPE_STORE_MB)
    scans = synth_hdl64.sequence(PIPE_FRAMES, seed=3)[0]
    t_start = time.time()
    want = base = None
    for i in range(rounds):
        if i == first:
            base = footprint()
        got = pipeline_round(scans)
        if want is None:
            want = got
        assert got == want, ("pipeline round %d differs from the first" % i, [j for j, (a, b) in enumerate(zip(got, want)) if a != b])
    end = footprint()
    print("pipeline footprint after %d rounds: device free %.0f -> %.0f MB, host peak RSS %.0f -> %.0f MB" % (rounds, base[0], end[0], base[1], end[1]))
    assert base[0] - end[0] < 256.0, "device memory is leaking: %.0f MB in %d pipeline rounds" % (base[0] - end[0], rounds - first)
    assert end[1] - base[1] < 256.0, "host memory is leaking: %.0f MB" % (end[1] - base[1])
    print("pipeline churn ok: %d rounds of %d frames in %.1f s" % (rounds, PIPE_FRAMES, time.time() - t_start))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 400
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    if n > 0:
        churn_solves(n)
    if rounds > 0:
        churn_pipelines(rounds)


if __name__ == "__main__":
    main()
