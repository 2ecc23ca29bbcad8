"""Builds tloam_amd/libtloam_hip.so (hand-written HIP kernels + the C ABI) for gfx950 with hipcc.

In-tree on purpose: the .so travels with the repo snapshot to the GPU box.  No CPU fallback is
built -- if hipcc is missing this raises.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libtloam_hip.so")
OBJ = os.path.join(CSRC, "_obj")

COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
# kernel arguments: the first 12 dwords of every kernel arrive preloaded in SGPRs (gfx950 command processor) instead of
# behind a scalar-load round trip -- the K3 / minimiser / finish kernels order their arguments for it (tl_gn.hip)
PRELOAD = ["-mllvm", "-amdgpu-kernarg-preload-count=12"]
COMMON += os.environ.get("TLOAM_EXTRA_HIPCC_FLAGS", "").split()  # development aid (-DTLOAM_K3_PROFILE ...)
UNITS = [
    # K1/K2: un-fused fp64 so the discontinuous gates see the oracle's operation order
    ("tl_nn.hip", ["-ffp-contract=off", *PRELOAD]),
    ("tl_scan.hip", ["-ffp-contract=off", *PRELOAD]),   # the scans: moved out of tl_nn.hip, compiled as it is
    ("tl_submap.hip", ["-ffp-contract=off"]),   # voxel indices / means in the oracle's operation order
    ("tl_feature.hip", ["-ffp-contract=off"]),  # PCA gates (flatness / cvr thresholds) like the oracle
    ("tl_seg.hip", ["-ffp-contract=off"]),      # segmentation: height / plane / voxel / curvature gates as the reference rounds them
    ("tl_odom.hip", []),                        # the odometry frame's gathers (copies) and selection counts (comparisons)
    ("tl_map.hip", ["-ffp-contract=off"]),      # the global map: transform and voxel_min_bound in the oracle's operation order
    ("tl_vmap.hip", ["-ffp-contract=off"]),     # the merged voxel map: transform, quantisation and centroids as DESIGN.md 14 states
    ("tl_cmap.hip", ["-ffp-contract=off"]),     # the closed map: transform and quantisation as DESIGN.md 14 states (tl_voxel.hpp)
    ("tl_extend.hip", ["-ffp-contract=off"]),   # the closed map's extension: the staged voxels numbered and committed (tl_voxel.hpp asks for the flag)
    ("tl_carve.hip", ["-ffp-contract=off"]),    # the closed map's carve: the ray walk and the miss test as DESIGN.md 21 states
    ("tl_surfel.hip", ["-ffp-contract=off"]),   # the closed map's surfels: moments, covariance and eig3_sym as DESIGN.md 22 states
    ("tl_snapshot.hip", ["-ffp-contract=off"]), # the closed map's snapshot: integer checksums and range tests (tl_voxel.hpp asks for the flag)
    ("tl_localise.hip", ["-ffp-contract=off"]), # localisation in the closed map: association, residuals, sums and the step as DESIGN.md 23 states
    ("tl_diff.hip", ["-ffp-contract=off"]),     # a scan diffed against the closed map: association, labels and the ray walk as DESIGN.md 26 states
    ("tl_raycast.hip", ["-ffp-contract=off"]),  # the closed map's ray-cast: the ray walk and the hit tests as DESIGN.md 28 states
    ("tl_free.hip", ["-ffp-contract=off"]),     # the closed map's free space: the ray walk and the free condition as DESIGN.md 29 states
    ("tl_clear.hip", ["-ffp-contract=off"]),    # the closed map's clearance: integer passes, and the segments' ray walk as DESIGN.md 30 states
    ("tl_route.hip", ["-ffp-contract=off"]),    # the route through the closed map: integer relaxation; the points' cells as DESIGN.md 31 states
    ("tl_frontier.hip", ["-ffp-contract=off"]), # the closed map's frontiers: integer labelling; the points' cells and the centres as DESIGN.md 32 states
    ("tl_view.hip", ["-ffp-contract=off"]),     # the closed map's view gain: the rays' ends and the walk as DESIGN.md 33 states (tl_voxel.hpp asks for the flag)
    ("tl_deskew.hip", ["-ffp-contract=off"]),   # the deskew: sweep time, exp(s xi) and the point action as DESIGN.md 15 states
    ("tl_place.hip", ["-ffp-contract=off"]),    # place recognition: Scan Context bins, keys and shift distances as DESIGN.md 16 states
    ("tl_loop.hip", ["-ffp-contract=off"]),     # loop verification: the target's transform and the score's distances as DESIGN.md 17 states
    ("tl_graph.hip", ["-ffp-contract=off"]),    # pose-graph optimisation: residuals, adjoints and sums as DESIGN.md 18 states
    # K3 / K5: no implicit contraction -- the same inlined residual code is compiled into several kernels (streaming sweep,
    # one-wave-per-chunk sweep, the one-launch Solve) and has to round alike in all of them (the tests compare those paths
    # bit for bit; with `fast` and with `on` the optimiser fused the same source line differently from kernel to kernel):
    # every fused multiply-add in tl_gn.hip / tl_step.hpp is spelled __builtin_fma
    ("tl_gn.hip", ["-ffp-contract=off", *PRELOAD]),
    ("tl_api.hip", []),          # context lifetime, configuration, sharding rules
    ("tl_api_frames.hip", []),   # HBM residency: hand-over of the clouds, search grids, staged frames
    ("tl_api_match.hip", []),    # the scanMatching driver
    ("tl_api_sets.hip", []),     # its factor set outside a frame: getters, pre-built sets, accumulate / solve, the timing helpers
    ("tl_api_comm.hip", []),     # multi-GPU exchange (RCCL at run time, callback, mailbox)
    ("tl_api_submap.hip", []),
    ("tl_api_feature.hip", []),
    ("tl_api_seg.hip", []),
    ("tl_api_odom.hip", ["-ffp-contract=off"]),   # the constant-velocity prediction, summed in the order DESIGN.md 12 states
    ("tl_api_map.hip", []),      # the global map and the registered scan
    ("tl_api_vmap.hip", []),     # the merged voxel map
    ("tl_api_deskew.hip", ["-ffp-contract=off"]),   # the deskew's configuration and xi = log(step), formed on the host
    ("tl_api_place.hip", ["-ffp-contract=off"]),    # place recognition's keyframe policy and database
    ("tl_api_loop.hip", ["-ffp-contract=off"]),     # loop verification: T_rel and the initial guesses formed on the host
    ("tl_api_graph.hip", ["-ffp-contract=off"]),    # pose-graph optimisation: the chain's Z and the weights formed on the host
    ("tl_api_cmap.hip", []),     # the closed map; its poses come rounded from tl_api_graph.hip
    ("tl_api_extend.hip", []),   # the closed map's extension; its poses come rounded from tl_api_graph.hip
    ("tl_api_carve.hip", []),    # the closed map's carve
    ("tl_api_surfel.hip", []),   # the closed map's surfels
    ("tl_api_localise.hip", ["-ffp-contract=off"]),   # localisation in the closed map: the prior's quaternion and matrix formed on the host
    ("tl_api_diff.hip", ["-ffp-contract=off"]),       # a scan diffed against the closed map: the pose checked as the localiser's prior
    ("tl_api_raycast.hip", ["-ffp-contract=off"]),    # the closed map's ray-cast: radius and radius2 formed on the host
    ("tl_api_free.hip", ["-ffp-contract=off"]),       # the closed map's free space: the auto box formed on the host in double
    ("tl_api_clear.hip", ["-ffp-contract=off"]),      # the closed map's clearance: R and need formed on the host in double
    ("tl_api_route.hip", ["-ffp-contract=off"]),      # the route through the closed map: need formed on the host in double
    ("tl_api_frontier.hip", ["-ffp-contract=off"]),   # the closed map's frontiers: the approach points formed on the host in double
    ("tl_api_view.hip", ["-ffp-contract=off"]),       # the closed map's view gain: the window's side and the approach poses formed on the host in double
    ("tl_api_snapshot.hip", []), # the closed map's snapshot: save, probe, load
    ("tl_probe.hip", []),        # read-stream bandwidth probe (the on-box ceiling of the bench's roofline block)
]
HEADERS = ["tl_common.hpp", "tl_forms.hpp", "tl_grid_plan.hpp", "tl_scan.hpp", "tl_se3.hpp", "tl_knn.hpp", "tl_walk.hpp", "tl_voxel.hpp", "tl_ctx.hpp", "tl_step.hpp", "tl_finish.hpp", "tl_prep.hpp", "tl_seg.hpp", "tl_extend_host.hpp", "tl_free_box.hpp", "tl_clear_box.hpp", "tl_tile_box.hpp", "tl_tile.hpp", "tl_view_box.hpp", os.path.join("..", "..", "include", "tloam_hip.h")]


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the MI355X path cannot be built (there is no CPU fallback)")
    return exe


def needs_build():
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    srcs = [os.path.join(CSRC, u) for u, _ in UNITS] + [os.path.join(CSRC, h) for h in HEADERS]
    return any(os.path.getmtime(s) > t for s in srcs)


def build_variant(name, flags, units=("tl_gn.hip",), verbose=False):
    """Tuning builds (never the product library): tloam_amd/_variants/lib_<name>.so = the shipped objects with
    `units` recompiled under extra -D flags.  Selected at run time with TLOAM_HIP_LIB=<path>."""
    build(force=False, verbose=verbose)
    hipcc = _hipcc()
    vdir = os.path.join(HERE, "_variants")
    odir = os.path.join(vdir, "obj_" + name)
    os.makedirs(odir, exist_ok=True)
    objs, procs = [], []
    for src, extra in UNITS:
        if src in units:
            obj = os.path.join(odir, src.replace(".hip", ".o"))
            if "-DNO_PRELOAD" in flags:   # A/B of the kernel-argument preload
                extra = [f for f in extra if f not in PRELOAD]
            cmd = [hipcc, *COMMON, *extra, *flags, "-c", os.path.join(CSRC, src), "-o", obj]
            procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        else:
            obj = os.path.join(OBJ, src.replace(".hip", ".o"))
        objs.append(obj)
    for cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            sys.stderr.write(out)
            raise RuntimeError("hipcc failed: " + " ".join(cmd))
    out = os.path.join(vdir, f"lib_{name}.so")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out, *objs, "-ldl"])
    return out


def build(force=False, verbose=False):
    if not force and not needs_build():
        return OUT
    hipcc = _hipcc()
    os.makedirs(OBJ, exist_ok=True)
    objs = []
    procs = []
    for src, extra in UNITS:
        obj = os.path.join(OBJ, src.replace(".hip", ".o"))
        cmd = [hipcc, *COMMON, *extra, "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        objs.append(obj)
    for cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            sys.stderr.write(out)
            raise RuntimeError("hipcc failed: " + " ".join(cmd))
        if verbose and out.strip():
            print(out)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT, *objs, "-ldl"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return OUT


if __name__ == "__main__":
    if "--variant" in sys.argv:   # python -m tloam_amd.build --variant NAME [--units a.hip,b.hip] -- -DFOO=1 ...
        i = sys.argv.index("--variant")
        units = ("tl_gn.hip",)
        if "--units" in sys.argv:
            units = tuple(sys.argv[sys.argv.index("--units") + 1].split(","))
        flags = sys.argv[sys.argv.index("--") + 1:] if "--" in sys.argv else []
        print(build_variant(sys.argv[i + 1], flags, units, verbose=True))
    else:
        print(build(force="--force" in sys.argv, verbose=True))
