"""The ctypes mirrors of tloam_map_config / tloam_map_info against the C header, the map's defaults against the reference's
configuration, the new entry points in the built library, and the PCD export round trip (no GPU needed)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tloam_amd import map_io
from tloam_amd import registration as reg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP_SYMBOLS = ("tloam_map_default_config", "tloam_map_configure", "tloam_map_get_info", "tloam_map_read",
               "tloam_registered_scan")


def test_map_struct_layout_matches_the_c_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "tloam_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(tloam_map_config), offsetof(tloam_map_config, enabled),
         offsetof(tloam_map_config, voxel), offsetof(tloam_map_config, reserve_points), sizeof(tloam_map_info),
         offsetof(tloam_map_info, n_points), offsetof(tloam_map_info, n_frames), offsetof(tloam_map_info, last_first),
         offsetof(tloam_map_info, last_count), offsetof(tloam_map_info, capacity_points),
         offsetof(tloam_map_info, overflow_frames));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c"); exe = os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = list(map(int, subprocess.check_output([exe]).split()))
    M, I = reg.MapConfig, reg.MapInfo
    assert vals == [C.sizeof(M), M.enabled.offset, M.voxel.offset, M.reserve_points.offset, C.sizeof(I), I.n_points.offset,
                    I.n_frames.offset, I.last_first.offset, I.last_count.offset, I.capacity_points.offset,
                    I.overflow_frames.offset]


def test_map_defaults_are_the_reference_configuration():
    cfg = reg.default_map_config()
    assert cfg.enabled == 0          # mapping_flag: false (lidar_odometry.yaml:21)
    assert cfg.voxel == 1.0          # global_map += ...VoxelDownSample(1.0) (front_end.cpp:272)
    assert cfg.reserve_points == 0   # the implementation's default reservation
    over = reg.default_map_config(enabled=1, voxel=0.5)
    assert over.enabled == 1 and over.voxel == 0.5
    with pytest.raises(KeyError):
        reg.default_map_config(mapping_flag=1)


def test_map_symbols_are_exported():
    L = reg.load_library()
    for name in MAP_SYMBOLS:
        assert name in reg.EXPORTED_SYMBOLS
        getattr(L, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", reg.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(MAP_SYMBOLS) <= exported


@pytest.mark.parametrize("ascii", (False, True))
def test_pcd_round_trip_is_bit_exact(tmp_path, ascii):
    rng = np.random.default_rng(5)
    xyz = np.concatenate([rng.normal(0, 50, (997, 3)), [[0.0, -0.0, 5e-324], [1e308, -1e-300, np.pi]]])
    path = str(tmp_path / "map.pcd")
    map_io.write_pcd(path, xyz, ascii=ascii)
    back = map_io.read_pcd(path)
    assert back.dtype == np.float64 and back.shape == xyz.shape
    assert back.tobytes() == xyz.tobytes()
    head = open(path, "rb").read(400).decode("ascii", errors="replace")
    for line in ("VERSION 0.7", "FIELDS x y z", "SIZE 8 8 8", "TYPE F F F", f"POINTS {len(xyz)}"):
        assert line in head
    empty = str(tmp_path / "empty.pcd")
    map_io.write_pcd(empty, np.zeros((0, 3)), ascii=ascii)
    assert map_io.read_pcd(empty).shape == (0, 3)


def test_pcd_reader_refuses_other_layouts(tmp_path):
    path = str(tmp_path / "f4.pcd")
    with open(path, "wb") as fh:
        fh.write(b"VERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\nWIDTH 1\nHEIGHT 1\nPOINTS 1\nDATA binary\n")
        fh.write(np.zeros(3, np.float32).tobytes())
    with pytest.raises(ValueError):
        map_io.read_pcd(path)
