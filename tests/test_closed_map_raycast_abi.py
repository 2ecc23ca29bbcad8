"""The ray-cast of the closed map without a GPU: the ctypes mirrors of tloam_closed_map_raycast_config /
_info against the C header, the defaults, the entry points in the built library and the Python methods."""
import inspect

import pytest

import abi_kit
from tloam_amd import raycast as RC
from tloam_amd import registration as reg

RAYCAST_SYMBOLS = ("tloam_closed_map_raycast_default_config", "tloam_closed_map_raycast_configure",
                   "tloam_closed_map_get_raycast_info", "tloam_closed_map_raycast")


def test_raycast_struct_layout_matches_the_c_header():
    """(every field of both mirrors against the header: tests/test_abi_header.py)"""
    assert abi_kit.sizes("tloam_closed_map_raycast_config", "tloam_closed_map_raycast_info") == [48, 64]
    assert abi_kit.constants("TLOAM_RAYCAST_SKIPPED", "TLOAM_RAYCAST_MISS", "TLOAM_RAYCAST_HIT_CENTROID", "TLOAM_RAYCAST_HIT_PLANE") \
        == [reg.RAYCAST_SKIPPED, reg.RAYCAST_MISS, reg.RAYCAST_HIT_CENTROID, reg.RAYCAST_HIT_PLANE] == [0, 1, 2, 3]
    assert (RC.RAYCAST_SKIPPED, RC.RAYCAST_MISS, RC.RAYCAST_HIT_CENTROID, RC.RAYCAST_HIT_PLANE) == (0, 1, 2, 3)
    assert abi_kit.constants("TLOAM_ABI_VERSION") == [8]   # additive: the ABI stays 8


def test_raycast_defaults():
    cfg = reg.default_closed_map_raycast_config()
    assert [getattr(cfg, f) for f, _ in cfg._fields_] == [120.0, 0.75, 1, 3, 1.0, 1, 0]
    diff = reg.default_closed_map_diff_config()
    assert (cfg.min_miss, cfg.miss_ratio, cfg.carve_gate) == (diff.min_miss, diff.miss_ratio, diff.carve_gate)   # the diff's gate
    assert reg.default_closed_map_raycast_config(planes=2, carve_gate=1).planes == 2
    with pytest.raises(KeyError):
        reg.default_closed_map_raycast_config(end_margin=1.0)


def test_raycast_symbols_are_exported():
    abi_kit.assert_exported(RAYCAST_SYMBOLS)
    sig = {name: list(inspect.signature(getattr(reg.HipRegistration, name)).parameters) for name in
           ("closed_map_raycast_configure", "closed_map_raycast", "closed_map_raycast_info")}
    assert sig == {"closed_map_raycast_configure": ["self", "cfg", "over"],
                   "closed_map_raycast": ["self", "ends", "pose", "want_ids"], "closed_map_raycast_info": ["self"]}
    assert inspect.signature(reg.HipRegistration.closed_map_raycast).parameters["want_ids"].default is False
    assert list(inspect.signature(RC.lidar_pattern).parameters) == ["rings", "n_az", "elev_lo", "elev_hi", "length"]
    assert list(inspect.signature(RC.scan_check).parameters) == ["H", "points", "pose", "extend"]
    assert inspect.signature(RC.scan_check).parameters["extend"].default == 2.0
