"""The clearance of the closed map without a GPU: the ctypes mirrors of tloam_closed_map_clearance_config /
_info against the C header, the constants, the defaults, the entry points in the built library and the Python methods."""
import inspect

import pytest

import abi_kit
from tloam_amd import map_io
from tloam_amd import registration as reg

CLEARANCE_SYMBOLS = ("tloam_closed_map_clearance_default_config", "tloam_closed_map_clearance_configure",
                     "tloam_closed_map_clearance_build", "tloam_closed_map_get_clearance_info", "tloam_closed_map_read_clearance",
                     "tloam_closed_map_clearance_points", "tloam_closed_map_clearance_segments",
                     "tloam_closed_map_clearance_columns")


def test_clearance_struct_layout_matches_the_c_header():
    """(every field of both mirrors against the header: tests/test_abi_header.py)"""
    assert abi_kit.sizes("tloam_closed_map_clearance_config", "tloam_closed_map_clearance_info") == [32, 96]
    assert abi_kit.constants("TLOAM_CLEARANCE_BEYOND", "TLOAM_CLEARANCE_OUTSIDE") == [reg.CLEARANCE_BEYOND, reg.CLEARANCE_OUTSIDE] \
        == [0xFFFF, 0xFFFE]
    assert abi_kit.constants("TLOAM_CLEARANCE_SKIPPED", "TLOAM_CLEARANCE_CLEAR", "TLOAM_CLEARANCE_BLOCKED", "TLOAM_CLEARANCE_LEFT_BOX") \
        == [reg.CLEARANCE_SKIPPED, reg.CLEARANCE_CLEAR, reg.CLEARANCE_BLOCKED, reg.CLEARANCE_LEFT_BOX] == [0, 1, 2, 3]
    assert 3 * 128 * 128 < reg.CLEARANCE_OUTSIDE            # every sum inside the passes fits beside the two sentinels
    assert abi_kit.constants("TLOAM_ABI_VERSION") == [8]   # additive: the ABI stays 8
    assert reg.load_library().tloam_abi_version() == 8


def test_clearance_defaults():
    cfg = reg.default_closed_map_clearance_config()
    assert [getattr(cfg, f) for f, _ in cfg._fields_] == [4.0, 120.0, 1 << 30, 1, 0]
    assert cfg.max_segment == reg.default_closed_map_raycast_config().max_range     # the ray-cast's segments
    assert cfg.max_bytes == reg.default_closed_map_free_config().max_bytes
    assert reg.default_closed_map_clearance_config(unknown_is_obstacle=0, max_distance=2.0).max_distance == 2.0
    with pytest.raises(KeyError):
        reg.default_closed_map_clearance_config(radius=1.0)
    info = reg.ClearanceInfo().as_dict()
    assert list(info) == abi_kit.header_structs()["tloam_closed_map_clearance_info"]
    assert info["lo_cells"] == (0, 0, 0) and info["n_cells"] == (0, 0, 0) and info["radius_cells"] == 0


def test_clearance_symbols_are_exported():
    abi_kit.assert_exported(CLEARANCE_SYMBOLS)
    names = ("closed_map_clearance_configure", "closed_map_clearance_build", "closed_map_clearance_info",
             "closed_map_clearance_field", "closed_map_clearance_points", "closed_map_clearance_segments",
             "closed_map_clearance_columns")
    sig = {name: list(inspect.signature(getattr(reg.HipRegistration, name)).parameters) for name in names}
    assert sig == {"closed_map_clearance_configure": ["self", "cfg", "over"], "closed_map_clearance_build": ["self"],
                   "closed_map_clearance_info": ["self"], "closed_map_clearance_field": ["self"],
                   "closed_map_clearance_points": ["self", "points", "pose", "want_distance"],
                   "closed_map_clearance_segments": ["self", "starts", "ends", "radius", "pose"],
                   "closed_map_clearance_columns": ["self", "z_lo", "z_hi", "min_free"]}
    assert inspect.signature(reg.HipRegistration.closed_map_clearance_points).parameters["pose"].default is None
    assert inspect.signature(reg.HipRegistration.closed_map_clearance_segments).parameters["pose"].default is None
    assert inspect.signature(reg.HipRegistration.closed_map_clearance_columns).parameters["min_free"].default == 1
    assert list(inspect.signature(map_io.write_clearance_pcd).parameters) == ["path", "H", "lo", "hi", "ascii"]
    assert list(inspect.signature(map_io.read_clearance_pcd).parameters) == ["path"]
