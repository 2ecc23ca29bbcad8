"""The closed map without a GPU: the ctypes mirrors of tloam_closed_map_config / _info against the C
header, the defaults, the entry points in the built library, and that its inputs restate as the contract says: the voxel map's
restatement (tests/voxel_map_np.py) fed each keyframe's transformed concatenation."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import voxel_map_np as VN  # noqa: E402
from tloam_amd import registration as reg  # noqa: E402

ROOT = os.path.dirname(HERE)
CLOSED_MAP_SYMBOLS = ("tloam_closed_map_default_config", "tloam_closed_map_configure", "tloam_closed_map_get_info",
                      "tloam_closed_map_build", "tloam_closed_map_read", "tloam_closed_map_read_box",
                      "tloam_closed_map_read_poses", "tloam_graph_correct_pose")


def test_closed_map_struct_layout_matches_the_c_header():
    cfg_fields = ("voxel", "origin", "cloud_mask", "reserved0", "reserve_voxels")
    info_fields = ("n_keyframes", "added_keyframes", "empty_keyframes", "overflow_keyframes", "n_voxels", "n_points",
                   "capacity_voxels", "pose_source", "launches")
    offs = ", ".join([f"offsetof(tloam_closed_map_config, {f})" for f in cfg_fields] +
                     [f"offsetof(tloam_closed_map_info, {f})" for f in info_fields])
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "tloam_hip.h"
int main(void) {
  size_t v[] = {sizeof(tloam_closed_map_config), sizeof(tloam_closed_map_info), %s};
  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%%zu ", v[i]);
  printf("%%d %%d %%d %%d\n", TLOAM_CLOSED_MAP_POSES_STORED, TLOAM_CLOSED_MAP_POSES_CORRECTED, TLOAM_CLOSED_MAP_POSES_CALLER,
         TLOAM_ABI_VERSION);
  return 0;
}''' % offs
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c"); exe = os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = list(map(int, subprocess.check_output([exe]).split()))
    M, I = reg.ClosedMapConfig, reg.ClosedMapInfo
    assert [n for n, _ in M._fields_] == list(cfg_fields) and [n for n, _ in I._fields_] == list(info_fields)
    want = [C.sizeof(M), C.sizeof(I)] + [getattr(M, f).offset for f in cfg_fields] + [getattr(I, f).offset for f in info_fields]
    assert vals[:-4] == want
    assert vals[:7] == [48, 64, 0, 8, 32, 36, 40]
    assert vals[-4:] == [0, 1, 2, 8]   # the pose sources; additive: the ABI stays 8


def test_closed_map_defaults():
    cfg = reg.default_closed_map_config()
    assert (cfg.voxel, tuple(cfg.origin), cfg.cloud_mask, cfg.reserved0, cfg.reserve_voxels) == (1.0, (0.0, 0.0, 0.0), 0xF0, 0, 0)
    over = reg.default_closed_map_config(voxel=0.25, origin=(1.0, -2.0, 0.5), cloud_mask=0x0F, reserve_voxels=64)
    assert (over.voxel, tuple(over.origin), over.cloud_mask, over.reserve_voxels) == (0.25, (1.0, -2.0, 0.5), 0x0F, 64)
    with pytest.raises(KeyError):
        reg.default_closed_map_config(enabled=1)
    with pytest.raises(KeyError):
        reg.default_closed_map_config(mask=0xFF)


def test_closed_map_symbols_are_exported():
    L = reg.load_library()
    for name in CLOSED_MAP_SYMBOLS:
        assert name in reg.EXPORTED_SYMBOLS
        getattr(L, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", reg.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(CLOSED_MAP_SYMBOLS) <= exported
    for name in ("closed_map_configure", "closed_map_build", "closed_map_info", "closed_map_read", "closed_map_read_box",
                 "closed_map_poses"):
        assert callable(getattr(reg.HipRegistration, name))


def test_a_keyframe_that_leaves_the_grid_drops_out_of_the_order_too():
    """the contract's order: ids follow the smallest global index over the keyframes that add -- which is what feeding the
    restatement the adding keyframes alone, ascending, gives"""
    rng = np.random.default_rng(0)
    clouds = [rng.uniform(-20, 20, (500, 3)) for _ in range(4)]
    clouds[1][17] = [float(1 << 21), 0.0, 0.0]   # keyframe 1 leaves the grid
    clouds[2][5] = [np.nan, 0.0, 0.0]            # a non-finite point is left out; its keyframe adds
    V = VN.VoxelMapNP(0.5)
    added = [V.add_frame(c) for c in clouds]
    assert added == [True, False, True, True] and V.overflow_frames == 1
    W = VN.VoxelMapNP(0.5)
    for k in (0, 2, 3):
        W.add_frame(clouds[k])
    assert V.keys.tobytes() == W.keys.tobytes() and V.N.tobytes() == W.N.tobytes() and V.Q.tobytes() == W.Q.tobytes()
    assert int(V.N.sum()) == 3 * 500 - 1
