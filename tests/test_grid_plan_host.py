"""The plan of a search-grid build (tloam_amd/csrc/tl_grid_plan.hpp: plan_grids, grid_reservation) against the
statements it replaced, without a GPU: a stand-alone program (tests/host/grid_plan_main.cpp, its own main, no HIP, only that
header) built with -fsanitize=address,undefined and run as a child process; `old_build` below restates, from build_grids_over and
the scans' size helpers as they were before tl_grid_plan.hpp, what a build then sized, laid out, reserved and launched.  Python
floats are IEEE doubles: the cell-growth loop compares bit for bit (the doubles travel in C99 hexadecimal)."""
import itertools
import math
import os
import subprocess

from tloam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = 4
BUFFERS = ("gp", "cell_of_pt", "rank_of_pt", "cell_start", "cell_cnt32", "cell_scan32", "totals32", "cell_cnt", "scan1p", "cell_scan", "scan_tmp")
ZEROED = ("cell_cnt32", "cell_cnt", "scan1p")
NO_KIND = dict(n=0, radius=1.0, lo=[0.0] * 3, hi=[0.0] * 3)


# ---- the scans' size helpers as tl_nn.hip had them ----------------------------------------------------------------------
def scan_tile_count(n):
    tiles = (n + 2048 - 1) // 2048
    return 0 if (n <= 16384 or tiles > 1024) else tiles


def scan_1p_applies(n, device_cus):
    return (n + 2048 - 1) // 2048 > 1024 and (n + 16384 - 1) // 16384 <= device_cus - device_cus // 16


def scan_tmp_elems(n):
    total = 0
    while n > 1:
        tiles = (n + 2048 - 1) // 2048
        total += 2 * tiles
        if tiles == 1:
            break
        n = tiles
    return total + 16


def scan_1p_ctl_elems(n):
    return (n + 16384 - 1) // 16384 + 8


# ---- build_grids_over as it was, up to its first launch -----------------------------------------------------------------
def old_build(i, cap):
    """-> (plan line fields, reservation, marks): `marks` names the layout and the outcome of the growth condition the case met"""
    kinds, cus, no_scan_1p, sparse_ok = i["kinds"], i["device_cus"], not i["allowed"], i["sparse_ok"]
    n, tgt_off, tgt_total = [0] * KINDS, [0] * KINDS, 0
    for k, K in enumerate(kinds):
        use = K["radius"] > 0.0 and K["n"] > 0
        n[k] = K["n"] if use else 0
        tgt_off[k] = tgt_total
        tgt_total += n[k]
    out = []
    ncells = [0] * KINDS
    cell_total = 0
    for k, K in enumerate(kinds):
        lo, hi = K["lo"], K["hi"]
        if n[k] > 0 and not (lo[0] <= hi[0] and lo[1] <= hi[1] and lo[2] <= hi[2]):
            n[k] = 0
        if n[k] == 0:
            out.append(dict(cell=0.0, inv_cell=1.0, org=[0.0] * 3, dim=[1, 1, 1], ncell=0))
            continue
        cell = K["radius"] * (1.0 + 1e-6)
        sparse_cap = max(16384.0, 32.0 * float(n[k])) if sparse_ok else 4.0e6
        while True:
            cells, dims = 1.0, [0.0] * 3
            for a in range(3):
                dims[a] = math.floor((hi[a] - lo[a]) / cell) + 1.0
                cells *= dims[a]
            if cells <= 4.0e6 and cells <= sparse_cap:
                break
            cell *= 1.25
        dim = [int(d) for d in dims]
        ncells[k] = dim[0] * dim[1] * dim[2]
        out.append(dict(cell=cell, inv_cell=1.0 / cell, org=list(lo), dim=dim, ncell=ncells[k]))
        cell_total += ncells[k]
    nc = max(cell_total, 1)
    n_tab = sum((c + 1 + 3) & ~3 for c in ncells)
    single_pass = (not no_scan_1p) and scan_1p_applies(nc + 1, cus)
    tiles = 0 if (cell_total == 0 or single_pass) else scan_tile_count(n_tab)
    at = 0
    for k in range(KINDS):
        out[k]["cell_base"] = at
        out[k]["start_base"] = at + (0 if tiles > 0 else k)      # out[k].cell_start = G.cell_start.p + cell_base[k] + (tiles > 0 ? 0 : k)
        at += ((ncells[k] + 1 + 3) & ~3) if tiles > 0 else ncells[k]
    res = dict.fromkeys(BUFFERS, 0)
    res["gp"] = res["cell_of_pt"] = max(tgt_total, 1)
    res["rank_of_pt"] = tgt_total + 1
    if tiles > 0:
        grow = n_tab > cap["cell_cnt32"] or n_tab > cap["cell_start"]
        nt_res = 2 * n_tab + 64 if grow else n_tab
        res.update(cell_start=nt_res, cell_cnt32=nt_res, cell_scan32=nt_res, totals32=1024)
    else:
        grow = nc + 1 > cap["cell_cnt"] or nc + KINDS + 1 > cap["cell_start"]
        nc_res = 2 * nc + 64 if grow else nc
        res.update(cell_start=nc_res + KINDS + 1, cell_cnt=nc_res + 1)
        if single_pass:
            res["scan1p"] = scan_1p_ctl_elems(nc_res + 1)
        else:
            res.update(cell_scan=nc_res + 1, scan_tmp=scan_tmp_elems(nc_res + 1))
    scan = ("NONE" if cell_total == 0 else "SINGLE_PASS" if single_pass else "TILES" if tiles > 0
            else "SMALL" if nc + 1 <= 16384 else "GENERIC")
    elem = 0 if cell_total == 0 else 4 if tiles > 0 else 8
    head = [scan, tiles, elem, tgt_total, cell_total, n_tab]
    per_kind = [[n[k], tgt_off[k], out[k]["cell"], out[k]["inv_cell"], *out[k]["org"], *out[k]["dim"], out[k]["ncell"], out[k]["cell_base"],
                 out[k]["start_base"]] for k in range(KINDS)]
    return head, per_kind, res, ("padded" if tiles > 0 else "packed", "padded" if tiles > 0 else "packed", grow)


# ---- the cases --------------------------------------------------------------------------------------------------------
def _kind(dims, n, radius=1.0, lo=(-7.0, 3.0, -2.0)):
    """a box of dims - 0.5 radii per axis: that many cells per axis while the cell stays at the radius"""
    return dict(n=n, radius=radius, lo=list(lo), hi=[l + (d - 0.5) * radius for l, d in zip(lo, dims)])


def _alone(K, at=2):
    return [K if k == at else NO_KIND for k in range(KINDS)]


def kind_sets():
    """name -> (kinds, sparse_ok, {cus, allowed -> expected scan} or None)"""
    every = lambda scan: {(c, a): scan for c in (256, 32, 8) for a in (True, False)}
    big = every("GENERIC")
    big[(256, True)] = "SINGLE_PASS"
    street = [dict(n=n, radius=r, lo=[-40.0, -12.0, -2.0], hi=[40.0 + k, 12.0, 4.0 + k]) for k, (n, r) in enumerate(zip(synth.KITTI_TGT, (0.5, 0.5, 1.0, 0.5)))]
    inverted = dict(n=12, radius=0.5, lo=[1e300] * 3, hi=[-1e300] * 3)
    sparse = dict(n=300, radius=0.5, lo=[-35.0, -35.0, -1.0], hi=[35.0, 35.0, 5.0])
    return {
        "25^3": (_alone(_kind((25, 25, 25), 2000)), True, every("SMALL")),
        "26^3": (_alone(_kind((26, 26, 26), 2000)), True, every("TILES")),
        "16371 cells": (_alone(_kind((16371, 1, 1), 2000)), True, every("SMALL")),
        "16372 cells": (_alone(_kind((16372, 1, 1), 2000)), True, every("TILES")),
        "126x130x128": (_alone(_kind((126, 130, 128), 66000)), True, every("TILES")),
        "150x341x41": (_alone(_kind((150, 341, 41), 66000)), True, every("GENERIC")),
        "128^3": (_alone(_kind((128, 128, 128), 66000)), True, big),
        "four kinds": (street, True, every("TILES")),
        "inverted box in front": ([inverted] + street[1:], True, every("TILES")),
        "radius 0": ([street[0], dict(street[1], radius=0.0)] + street[2:], True, every("TILES")),
        "all empty": ([NO_KIND, dict(NO_KIND, n=5, radius=0.0), inverted, dict(NO_KIND, n=0)], True, every("NONE")),
        "sparse kind": (_alone(sparse, 3), True, None),
        "sparse kind, direct-set caps": (_alone(sparse, 3), False, None),
        "first try over 4e6": (_alone(dict(n=500000, radius=0.5, lo=[-100.0, -100.0, -5.0], hi=[100.0, 100.0, 25.0]), 0), False, None),
    }


def capacities(i):
    """for the case's own sizes: nothing, exactly enough, and each of the two buffers its growth condition looks at one short"""
    _, _, res, (layout, _, _) = old_build(i, dict(cell_start=1 << 40, cell_cnt=1 << 40, cell_cnt32=1 << 40))
    hist = "cell_cnt32" if layout == "padded" else "cell_cnt"
    enough = dict(cell_start=0, cell_cnt=0, cell_cnt32=0)
    enough.update({"cell_start": res["cell_start"], hist: res[hist]})
    yield dict(cell_start=0, cell_cnt=0, cell_cnt32=0)
    yield enough
    yield dict(enough, cell_start=enough["cell_start"] - 1)
    yield dict(enough, **{hist: enough[hist] - 1})


def line_of(i, cap):
    f = [i["device_cus"], int(i["allowed"]), int(i["sparse_ok"])]
    for K in i["kinds"]:
        f += [K["n"], float(K["radius"]).hex()] + [float(v).hex() for v in K["lo"] + K["hi"]]
    return " ".join(str(v) for v in f + [cap["cell_start"], cap["cell_cnt"], cap["cell_cnt32"]])


def parse(line):
    parts = [p.split() for p in line.split("|")]
    head = [parts[0][0]] + [int(v) for v in parts[0][1:]]
    per_kind = [[int(p[0]), int(p[1])] + [float.fromhex(v) for v in p[2:7]] + [int(v) for v in p[7:]] for p in parts[1:1 + KINDS]]
    w = parts[1 + KINDS]
    res = {b: int(w[2 * j]) for j, b in enumerate(BUFFERS)}
    zeroed = {b for j, b in enumerate(BUFFERS) if w[2 * j + 1] == "1"}
    return head, per_kind, res, zeroed


def test_plan_grids_agrees_with_the_build_it_replaced_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "grid_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host", "grid_plan_main.cpp"), "-o", exe])
    cases = []
    for (name, (kinds, sparse_ok, expect)), cus, allowed in itertools.product(kind_sets().items(), (256, 32, 8), (True, False)):
        i = dict(kinds=kinds, sparse_ok=sparse_ok, device_cus=cus, allowed=allowed)
        for cap in capacities(i):
            cases.append((name, i, cap, expect[(cus, allowed)] if expect else None))
    run = subprocess.run([exe], input="\n".join(line_of(i, cap) for _, i, cap, _ in cases) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stderr == ""
    got = run.stdout.splitlines()
    assert len(got) == len(cases) == 14 * 6 * 4
    seen = set()
    for (name, i, cap, scan), g in zip(cases, got):
        head, per_kind, res, marks = old_build(i, cap)
        g_head, g_kinds, g_res, g_zeroed = parse(g)
        assert g_head == head, (name, i, cap)
        for k in range(KINDS):
            assert g_kinds[k] == per_kind[k], (name, k, i, cap)      # (floats compared as floats: exact)
        assert g_res == res, (name, i, cap)
        assert g_zeroed == {b for b in ZEROED if res[b] > 0}, (name, i, cap)
        if scan:
            assert head[0] == scan, (name, i["device_cus"], i["allowed"], head)
        seen.update([("scan", head[0]), ("layout", marks[0]), ("grow", marks[1], marks[2])])
    # the dimensions and sizes the cases were made for (256 CUs, single pass allowed, nothing allocated yet)
    first = {name: old_build(i, cap) for name, i, cap, _ in reversed(cases) if i["device_cus"] == 256 and i["allowed"]}
    assert first["26^3"][0][:2] == ["TILES", 9] and first["26^3"][0][4] == 17576
    assert first["16371 cells"][0][4:] == [16371, 16384] and first["16372 cells"][0][4:] == [16372, 16388]
    assert first["126x130x128"][0][:2] == ["TILES", 1024] and first["126x130x128"][0][4] == 2096640
    assert first["150x341x41"][0][4] == 2097150 and scan_tile_count(2097150 + 1) == 1024 and scan_tile_count(first["150x341x41"][0][5]) == 0
    assert first["128^3"][0][4] == 2097152
    assert all(first["four kinds"][1][k][12] % 2048 != 0 for k in (1, 2, 3))          # no base of kinds 1..3 on a tile
    assert first["inverted box in front"][1][0][0] == 0 and first["inverted box in front"][1][1][1] == 12   # dropped, place kept
    assert first["sparse kind"][1][3][2] > 1.0 and first["sparse kind"][1][3][10] <= 16384
    assert first["sparse kind, direct-set caps"][1][3][2] == 0.5 * (1.0 + 1e-6)
    assert first["first try over 4e6"][1][0][2] > 0.5 * (1.0 + 1e-6)
    # every path, both layouts and both outcomes of each layout's growth condition were reached by some input
    for scan in ("NONE", "SMALL", "TILES", "SINGLE_PASS", "GENERIC"):
        assert ("scan", scan) in seen, scan
    for layout in ("padded", "packed"):
        assert ("layout", layout) in seen
        for grow in (True, False):
            assert ("grow", layout, grow) in seen, (layout, grow)
