"""The launch forms of a scanMatching frame (tloam_amd/csrc/tl_forms.hpp: decide_forms) against the predicates
the driver asked before it had them, without a GPU: a stand-alone program (tests/host/frame_forms_main.cpp, its own main, no HIP,
only that header) built with -fsanitize=address,undefined and run as a child process over the cross product of rank layouts,
knobs and size boundaries; `old_forms` below restates, from the driver as it was before tl_forms.hpp, what it then launched."""
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOBS = ("no_persistent_solve", "no_direct_set", "no_device_loop", "no_build_reuse", "fused_large", "no_qbin_ride")
LAYOUTS = {            # nranks, loopback, mailbox
    "one rank": (1, 0, 0),
    "loop-back mailbox": (1, 1, 1),
    "2 ranks, mailbox": (2, 0, 1),
    "2 ranks, collective": (2, 0, 0),
}
LIFTED = 1 << 30


def _chunks(n):          # a segment's capacity: its factors rounded up to the sweep's chunk of 128 (reserve_seg)
    return [max((x + 127) // 128, 1) * 128 for x in n]


def _size(n_src, maxnum, k3_grid, k3_single, seg_cap=None, has_grid=(1, 1, 1, 1)):
    cap = seg_cap if seg_cap is not None else _chunks([min(s, max(m, 0)) for s, m in zip(n_src, maxnum)])
    return dict(n_src=list(n_src), maxnum=list(maxnum), n_tgt=[20000] * 4, has_grid=list(has_grid), k3_grid=k3_grid, k3_single=k3_single,
                seg_cap=list(cap))


def sizes(device_cus):
    kitti = [3000, 3000, 2500, 900]
    big = [60000, 40000, 25000, 6072]                 # 131072 source points
    out = []
    for first in (4096, 4097):                        # a kind's flag bytes: kFlagbStride
        out.append(_size([first, 3000, 2500, 900], [LIFTED] * 4, 12, 1))
    for last in (1384, 1385):                         # 16384 | 16385 source slots, the caps keep the segments small
        out.append(_size([5000, 5000, 5000, last], [2000] * 4, 12, 1))
        out.append(_size([4096, 4096, 4096, last + 2712], [2000] * 4, 12, 1))
    for last in (6072, 6073):                         # 131072 | 131073 source slots
        out.append(_size(big[:3] + [last], [LIFTED] * 4, 512, 0))
        out.append(_size(big[:3] + [last], [LIFTED, LIFTED, LIFTED, last - 1], 512, 0))        # one cap one below its n_src
        out.append(_size(big[:3] + [last], [LIFTED] * 4, 512, 0, has_grid=(1, 1, 0, 1)))       # a kind without a search grid
    out.append(_size([4095, 4095, 4095, 4099], [LIFTED] * 4, 33, 1, seg_cap=[4096, 4096, 4096, 4096]))   # capacity sum 16384
    out.append(_size([4095, 4095, 4095, 4099], [LIFTED] * 4, 33, 1, seg_cap=[4096, 4096, 4096, 4224]))   # ... 16512
    for grid in (16, 17, device_cus, device_cus + 1):  # the one-launch Solve's grid: kTaggedRows, the device's CUs
        out.append(_size(kitti, [LIFTED] * 4, grid, 1))
    out.append(_size(kitti, [LIFTED] * 4, 12, 0))
    out.append(_size([0, 0, 0, 0], [LIFTED] * 4, 1, 1))   # (no source slots: a pre-built set)
    return out


def inputs():
    for cus in (256, 8):
        for layout in LAYOUTS.values():
            for knobs in itertools.product((0, 1), repeat=len(KNOBS)):
                for factor_num in (3, 4):
                    for max_iterations in (1, 8, 9):
                        for sz in sizes(cus):
                            i = dict(nranks=layout[0], loopback=layout[1], mailbox=layout[2], device_cus=cus, factor_num=factor_num,
                                     max_iterations=max_iterations, **sz)
                            i.update(zip(KNOBS, knobs))
                            yield i


def line_of(i):
    head = [i["nranks"], i["loopback"], i["mailbox"], i["device_cus"]] + [i[k] for k in KNOBS] + [i["factor_num"], i["max_iterations"]]
    return " ".join(str(v) for v in head + i["maxnum"] + i["n_src"] + i["n_tgt"] + i["has_grid"] + [i["k3_grid"], i["k3_single"]] + i["seg_cap"])


def old_forms(i):
    """What the driver launched for such a frame when every site asked its own predicate (tl_api_match.hip, tl_nn.hip, tl_gn.hip
    before tl_forms.hpp; the names are the functions' and locals' of that source)."""
    one_rank = i["nranks"] == 1 and not i["loopback"]
    exchanging = i["nranks"] > 1 or bool(i["loopback"])
    n_slots = sum(i["n_src"])
    direct_set_size = n_slots > 131072                                       # kQuadLimit
    solve_small_fits = i["k3_grid"] <= 16 and i["k3_grid"] <= i["device_cus"]  # kTaggedRows
    solve_small_path = one_rank and bool(i["k3_single"]) and not i["no_persistent_solve"] and solve_small_fits
    # tloam_sm_begin: the direct set, and its demotion once the grids are built
    direct = not (i["no_direct_set"] or not one_rank or i["factor_num"] != 4 or not direct_set_size)
    direct = direct and not any(s > m or t == 0 for s, m, t in zip(i["n_src"], i["maxnum"], i["n_tgt"]))
    direct = direct and all(i["has_grid"])
    prepare_small_fits = n_slots <= 16384
    flagb = solve_small_path and prepare_small_fits and all(s <= 4096 for s in i["n_src"])   # SlotView::flagb != nullptr
    prepare_small_path = one_rank and prepare_small_fits
    self_prepare_path = flagb and prepare_small_path and solve_small_path
    finish_small_path = one_rank and sum(i["seg_cap"]) <= 16384
    # enqueue_build (the flag bytes are written whoever drives the loop; the stepwise API then prepares with k_prepare_small)
    if direct:
        prepare = "NONE"
    elif self_prepare_path:
        prepare = "IN_SOLVE"
    elif prepare_small_path:
        prepare = "SMALL"
    elif one_rank:
        prepare = "TILES"
    else:
        prepare = "FULL"
    # enqueue_solve
    one_launch = bool(i["fused_large"]) and ((not i["k3_single"]) if one_rank else bool(i["mailbox"]))
    if solve_small_path:
        solve = "PERSISTENT"
    elif one_launch:
        solve = "FUSED_LARGE"
    elif exchanging:
        solve = "SHARDED_MBOX" if i["mailbox"] else "SHARDED_COLLECTIVE"
    elif i["k3_single"]:
        solve = "SMALL_STEP"
    else:
        solve = "SWEEP_REDUCE"
    # enqueue_finish
    finish = "DIRECT" if direct else "SMALL" if finish_small_path else "SHARDED" if exchanging else "LARGE"
    # tloam_scan_match, enqueue_outer_iterations
    M = i["max_iterations"]
    device_loop = one_rank and 1 <= M <= 8 and not i["no_build_reuse"] and not i["no_device_loop"]
    rides = "NO"
    if device_loop:
        ride = prepare_small_path and finish_small_path and 0 < n_slots <= 16384                 # build_finish_small_fits
        ride_large = not ride and one_rank and not finish_small_path and n_slots > 131072        # build_finish_large_fits
        fin_in_solve = self_prepare_path and finish_small_path and M <= 8                        # kMaxOuterInLaunch
        rides = "IN_SOLVE" if fin_in_solve else "ON_SEARCH_SMALL" if ride else "ON_SEARCH_LARGE" if ride_large else "NO"
    qbin = one_rank and not i["no_qbin_ride"] and direct_set_size
    return " ".join(["DIRECT" if direct else "COMPACT", prepare, solve, finish, rides, "DEVICE" if device_loop else "HOST", "1" if qbin else "0"])


def test_decide_forms_agrees_with_the_scattered_predicates_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "frame_forms")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host", "frame_forms_main.cpp"), "-o", exe])
    ins = list(inputs())
    run = subprocess.run([exe], input="\n".join(line_of(i) for i in ins) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stderr == ""
    got = run.stdout.splitlines()
    assert len(got) == len(ins) > 4000
    seen = set()
    for i, g in zip(ins, got):
        assert g == old_forms(i), (i, g, old_forms(i))
        seen.update(enumerate(g.split()))
    # every form of every decision was reached by some input
    for pos, names in enumerate((("COMPACT", "DIRECT"), ("NONE", "IN_SOLVE", "SMALL", "TILES", "FULL"),
                                 ("PERSISTENT", "FUSED_LARGE", "SHARDED_MBOX", "SHARDED_COLLECTIVE", "SMALL_STEP", "SWEEP_REDUCE"),
                                 ("DIRECT", "SMALL", "LARGE", "SHARDED"), ("NO", "ON_SEARCH_SMALL", "ON_SEARCH_LARGE", "IN_SOLVE"),
                                 ("DEVICE", "HOST"), ("0", "1"))):
        for name in names:
            assert (pos, name) in seen, (pos, name)
