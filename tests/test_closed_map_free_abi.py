"""The free space of the closed map without a GPU: the ctypes mirrors of tloam_closed_map_free_config /
_info against the C header, the defaults, the entry points in the built library and the Python methods."""
import inspect

import pytest

import abi_kit
from tloam_amd import map_io
from tloam_amd import registration as reg

FREE_SYMBOLS = ("tloam_closed_map_free_default_config", "tloam_closed_map_free_configure", "tloam_closed_map_get_free_info",
                "tloam_closed_map_free_reset", "tloam_closed_map_free_add_keyframes", "tloam_closed_map_free_add_scan",
                "tloam_closed_map_occupancy", "tloam_closed_map_read_free", "tloam_closed_map_free_columns",
                "tloam_closed_map_read_free_words")


def test_free_struct_layout_matches_the_c_header():
    """(every field of both mirrors against the header: tests/test_abi_header.py)"""
    assert abi_kit.sizes("tloam_closed_map_free_config", "tloam_closed_map_free_info") == [56, 128]
    assert abi_kit.constants("TLOAM_OCCUPANCY_INVALID", "TLOAM_OCCUPANCY_UNKNOWN", "TLOAM_OCCUPANCY_FREE", "TLOAM_OCCUPANCY_OCCUPIED") \
        == [reg.OCCUPANCY_INVALID, reg.OCCUPANCY_UNKNOWN, reg.OCCUPANCY_FREE, reg.OCCUPANCY_OCCUPIED] == [0, 1, 2, 3]
    assert abi_kit.constants("TLOAM_ABI_VERSION") == [8]   # additive: the ABI stays 8
    assert reg.load_library().tloam_abi_version() == 8


def test_free_defaults():
    cfg = reg.default_closed_map_free_config()
    assert [getattr(cfg, f) for f, _ in cfg._fields_] == [60.0, 1.0, 1 << 30, 1, 3, 1.0, 0, 0]
    carve, diff = reg.default_closed_map_carve_config(), reg.default_closed_map_diff_config()
    assert (cfg.max_range, cfg.end_margin, cfg.ray_mask) == (carve.max_range, carve.end_margin, carve.ray_mask)   # the carve's rays
    assert (cfg.min_miss, cfg.miss_ratio, cfg.carve_gate) == (diff.min_miss, diff.miss_ratio, diff.carve_gate)     # the diff's gate
    assert reg.default_closed_map_free_config(carve_gate=1, max_bytes=4096).max_bytes == 4096
    with pytest.raises(KeyError):
        reg.default_closed_map_free_config(radius=1.0)
    info = reg.FreeInfo().as_dict()
    assert list(info) == abi_kit.header_structs()["tloam_closed_map_free_info"]
    assert info["lo_cells"] == (0, 0, 0) and info["n_bricks"] == (0, 0, 0)


def test_free_symbols_are_exported():
    abi_kit.assert_exported(FREE_SYMBOLS)
    names = ("closed_map_free_configure", "closed_map_free_reset", "closed_map_free_add_keyframes", "closed_map_free_add_scan",
             "closed_map_free_info", "closed_map_free_build", "closed_map_occupancy", "closed_map_free_cells",
             "closed_map_free_columns")
    sig = {name: list(inspect.signature(getattr(reg.HipRegistration, name)).parameters) for name in names}
    assert sig == {"closed_map_free_configure": ["self", "cfg", "over"], "closed_map_free_reset": ["self", "lo_cells", "hi_cells"],
                   "closed_map_free_add_keyframes": ["self"], "closed_map_free_add_scan": ["self", "points", "pose"],
                   "closed_map_free_info": ["self"], "closed_map_free_build": ["self", "lo_cells", "hi_cells"],
                   "closed_map_occupancy": ["self", "points", "pose", "want_ids"], "closed_map_free_cells": ["self", "lo", "hi"],
                   "closed_map_free_columns": ["self", "z_lo", "z_hi", "min_free"]}
    assert inspect.signature(reg.HipRegistration.closed_map_occupancy).parameters["pose"].default is None
    assert inspect.signature(reg.HipRegistration.closed_map_free_columns).parameters["min_free"].default == 1
    assert list(inspect.signature(map_io.write_free_pcd).parameters) == ["path", "H", "lo", "hi", "ascii"]
