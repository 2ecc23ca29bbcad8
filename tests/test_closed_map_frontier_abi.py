"""The frontiers of the closed map without a GPU: the ctypes mirrors of tloam_closed_map_frontier_config /
_cluster / _info against the C header, the constants, the defaults, the entry points in the built library and the Python
methods."""
import ctypes as C
import inspect

import numpy as np
import pytest

import abi_kit
from tloam_amd import map_io
from tloam_amd import registration as reg

FRONTIER_SYMBOLS = ("tloam_closed_map_frontier_default_config", "tloam_closed_map_frontier_configure", "tloam_closed_map_frontier_build",
                    "tloam_closed_map_get_frontier_info", "tloam_closed_map_read_frontier", "tloam_closed_map_frontier_clusters",
                    "tloam_closed_map_read_frontier_cells", "tloam_closed_map_frontier_points", "tloam_closed_map_frontier_costs",
                    "tloam_closed_map_frontier_columns")


def test_frontier_struct_layout_matches_the_c_header():
    """(every field of the three mirrors against the header: tests/test_abi_header.py)"""
    assert abi_kit.sizes("tloam_closed_map_frontier_config", "tloam_closed_map_frontier_cluster", "tloam_closed_map_frontier_info") \
        == [24, 64, 152]
    # the cluster record has no implicit padding: its members' sizes sum to its size, and numpy reads an array of them alike
    assert sum(abi_kit.member_sizes("tloam_closed_map_frontier_cluster")) == 64
    dt = np.dtype(reg.FRONTIER_CLUSTER_DTYPE)
    assert dt.itemsize == C.sizeof(reg.FrontierCluster) == 64
    assert [dt.fields[f][1] for f, _ in reg.FrontierCluster._fields_] == abi_kit.offsets("tloam_closed_map_frontier_cluster")
    assert abi_kit.constants("TLOAM_FRONTIER_FREE", "TLOAM_FRONTIER_UNKNOWN", "TLOAM_FRONTIER_OCCUPIED", "TLOAM_FRONTIER_OUTSIDE",
                             "TLOAM_FRONTIER_ALL") \
        == [reg.FRONTIER_FREE, reg.FRONTIER_UNKNOWN, reg.FRONTIER_OCCUPIED, reg.FRONTIER_OUTSIDE, reg.FRONTIER_ALL] \
        == [0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC, 0xFFFFFFFF]
    assert (1 << 30) // 4 < reg.FRONTIER_OUTSIDE            # under the default max_bytes no index can meet a sentinel
    assert abi_kit.constants("TLOAM_ABI_VERSION") == [8]   # additive: the ABI stays 8
    assert reg.load_library().tloam_abi_version() == 8


def test_frontier_defaults():
    cfg = reg.default_closed_map_frontier_config()
    assert [getattr(cfg, f) for f, _ in cfg._fields_] == [1 << 30, 8, 2, 65536, 16]
    route = reg.default_closed_map_route_config()
    assert (cfg.max_bytes, cfg.max_rounds, cfg.rounds_per_wait) == (route.max_bytes, route.max_rounds, route.rounds_per_wait)
    assert reg.default_closed_map_frontier_config(min_cells=1, reach=4).reach == 4
    with pytest.raises(KeyError):
        reg.default_closed_map_frontier_config(radius=1.0)
    info = reg.FrontierInfo().as_dict()
    assert list(info) == abi_kit.header_structs()["tloam_closed_map_frontier_info"]
    assert info["lo_cells"] == (0, 0, 0) and info["n_cells"] == (0, 0, 0) and info["clusters"] == 0
    assert set(reg.FRONTIER_DIAGNOSTICS) < set(info) and reg.FRONTIER_DIAGNOSTICS == ("tile_updates", "rounds", "launches", "waits")


def test_frontier_symbols_are_exported():
    abi_kit.assert_exported(FRONTIER_SYMBOLS)
    names = ("closed_map_frontier_configure", "closed_map_frontier_build", "closed_map_frontier_info", "closed_map_frontier_field",
             "closed_map_frontier_clusters", "closed_map_frontier_cells", "closed_map_frontier_points", "closed_map_frontier_costs",
             "closed_map_frontier_columns")
    sig = {name: list(inspect.signature(getattr(reg.HipRegistration, name)).parameters) for name in names}
    assert sig == {"closed_map_frontier_configure": ["self", "cfg", "over"], "closed_map_frontier_build": ["self"],
                   "closed_map_frontier_info": ["self"], "closed_map_frontier_field": ["self"], "closed_map_frontier_clusters": ["self"],
                   "closed_map_frontier_cells": ["self", "root"], "closed_map_frontier_points": ["self", "points", "pose"],
                   "closed_map_frontier_costs": ["self"], "closed_map_frontier_columns": ["self", "z_lo", "z_hi", "min_free"]}
    assert inspect.signature(reg.HipRegistration.closed_map_frontier_cells).parameters["root"].default == reg.FRONTIER_ALL
    assert inspect.signature(reg.HipRegistration.closed_map_frontier_columns).parameters["min_free"].default == 1
    assert list(inspect.signature(map_io.write_frontier_pcd).parameters) == ["path", "H", "ascii"]
    assert list(inspect.signature(map_io.read_frontier_pcd).parameters) == ["path"]
    assert list(inspect.signature(map_io.write_frontier_clusters_pcd).parameters) == ["path", "H", "with_cost", "ascii"]
    assert list(inspect.signature(map_io.read_frontier_clusters_pcd).parameters) == ["path"]
