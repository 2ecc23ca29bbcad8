"""The ctypes mirrors of tloam_map_config / tloam_map_info against the C header, the map's defaults against the reference's
configuration, the new entry points in the built library, and the PCD export round trip (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

import abi_kit
from tloam_amd import map_io
from tloam_amd import registration as reg

MAP_SYMBOLS = ("tloam_map_default_config", "tloam_map_configure", "tloam_map_get_info", "tloam_map_read",
               "tloam_registered_scan")


def test_map_struct_layout_matches_the_c_header():
    """(every field of every mirror against the header: tests/test_abi_header.py)"""
    for name, S in (("tloam_map_config", reg.MapConfig), ("tloam_map_info", reg.MapInfo)):
        assert abi_kit.sizes(name) == [C.sizeof(S)] and abi_kit.offsets(name) == [getattr(S, f).offset for f, _ in S._fields_]


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
    abi_kit.assert_exported(MAP_SYMBOLS)


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
