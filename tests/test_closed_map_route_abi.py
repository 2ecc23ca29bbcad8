"""The route through the closed map without a GPU: the ctypes mirrors of tloam_closed_map_route_config /
_info against the C header, the constants, the defaults, the entry points in the built library and the Python methods."""
import inspect

import pytest

import abi_kit
from tloam_amd import map_io
from tloam_amd import registration as reg

ROUTE_SYMBOLS = ("tloam_closed_map_route_default_config", "tloam_closed_map_route_configure", "tloam_closed_map_route_build",
                 "tloam_closed_map_get_route_info", "tloam_closed_map_read_route", "tloam_closed_map_route_points",
                 "tloam_closed_map_route_paths", "tloam_closed_map_route_columns")


def test_route_struct_layout_matches_the_c_header():
    """(every field of both mirrors against the header: tests/test_abi_header.py)"""
    assert abi_kit.sizes("tloam_closed_map_route_config", "tloam_closed_map_route_info") == [16, 136]
    assert abi_kit.constants("TLOAM_ROUTE_UNREACHED", "TLOAM_ROUTE_BLOCKED", "TLOAM_ROUTE_OUTSIDE") \
        == [reg.ROUTE_UNREACHED, reg.ROUTE_BLOCKED, reg.ROUTE_OUTSIDE] == [0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD]
    assert abi_kit.constants("TLOAM_ROUTE_PATH_OUTSIDE", "TLOAM_ROUTE_PATH_REACHED", "TLOAM_ROUTE_PATH_UNREACHED",
                             "TLOAM_ROUTE_PATH_BLOCKED", "TLOAM_ROUTE_PATH_TRUNCATED") \
        == [reg.ROUTE_PATH_OUTSIDE, reg.ROUTE_PATH_REACHED, reg.ROUTE_PATH_UNREACHED, reg.ROUTE_PATH_BLOCKED, reg.ROUTE_PATH_TRUNCATED] \
        == [0, 1, 2, 3, 4]
    assert 5 * ((1 << 30) // 4) < reg.ROUTE_OUTSIDE          # under the default max_bytes no cost can meet a sentinel
    assert abi_kit.constants("TLOAM_ABI_VERSION") == [8]   # additive: the ABI stays 8
    assert reg.load_library().tloam_abi_version() == 8


def test_route_defaults():
    cfg = reg.default_closed_map_route_config()
    assert [getattr(cfg, f) for f, _ in cfg._fields_] == [1 << 30, 65536, 16]
    assert cfg.max_bytes == reg.default_closed_map_clearance_config().max_bytes
    assert reg.default_closed_map_route_config(rounds_per_wait=1, max_rounds=7).max_rounds == 7
    with pytest.raises(KeyError):
        reg.default_closed_map_route_config(radius=1.0)
    info = reg.RouteInfo().as_dict()
    assert list(info) == abi_kit.header_structs()["tloam_closed_map_route_info"]
    assert info["lo_cells"] == (0, 0, 0) and info["n_cells"] == (0, 0, 0) and info["rounds"] == 0
    assert set(reg.ROUTE_DIAGNOSTICS) < set(info) and reg.ROUTE_DIAGNOSTICS == ("tile_updates", "rounds", "launches", "waits")


def test_route_symbols_are_exported():
    abi_kit.assert_exported(ROUTE_SYMBOLS)
    names = ("closed_map_route_configure", "closed_map_route_build", "closed_map_route_info", "closed_map_route_field",
             "closed_map_route_points", "closed_map_route_paths", "closed_map_route_columns")
    sig = {name: list(inspect.signature(getattr(reg.HipRegistration, name)).parameters) for name in names}
    assert sig == {"closed_map_route_configure": ["self", "cfg", "over"], "closed_map_route_build": ["self", "goals", "radius", "pose"],
                   "closed_map_route_info": ["self"], "closed_map_route_field": ["self"],
                   "closed_map_route_points": ["self", "points", "pose", "want_distance"],
                   "closed_map_route_paths": ["self", "starts", "max_cells", "pose"],
                   "closed_map_route_columns": ["self", "z_lo", "z_hi", "goals", "radius", "min_free", "pose"]}
    assert inspect.signature(reg.HipRegistration.closed_map_route_build).parameters["radius"].default == 0.0
    assert inspect.signature(reg.HipRegistration.closed_map_route_paths).parameters["pose"].default is None
    assert inspect.signature(reg.HipRegistration.closed_map_route_columns).parameters["min_free"].default == 1
    assert list(inspect.signature(map_io.write_route_pcd).parameters) == ["path", "H", "lo", "hi", "ascii"]
    assert list(inspect.signature(map_io.read_route_pcd).parameters) == ["path"]
    assert list(inspect.signature(map_io.write_route_paths_pcd).parameters) == ["path", "H", "starts", "max_cells", "pose", "ascii"]
    assert list(inspect.signature(map_io.read_route_paths_pcd).parameters) == ["path"]
