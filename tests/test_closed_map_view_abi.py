"""The view gain of the closed map without a GPU: the ctypes mirrors of tloam_closed_map_view_config /
_record / _info against the C header, the defaults, the entry points in the built library and the Python methods."""
import ctypes as C
import inspect

import numpy as np
import pytest

import abi_kit
from tloam_amd import map_io
from tloam_amd import registration as reg

VIEW_SYMBOLS = ("tloam_closed_map_view_default_config", "tloam_closed_map_view_configure", "tloam_closed_map_view_gain",
                "tloam_closed_map_view_cells", "tloam_closed_map_frontier_gains", "tloam_closed_map_get_view_info")


def test_view_struct_layout_matches_the_c_header():
    """(every field of the three mirrors against the header: tests/test_abi_header.py)"""
    assert abi_kit.sizes("tloam_closed_map_view_config", "tloam_closed_map_view_record", "tloam_closed_map_view_info") == [24, 64, 88]
    # the record has no implicit padding: its members' sizes sum to its size, and numpy reads an array of them alike
    assert sum(abi_kit.member_sizes("tloam_closed_map_view_record")) == 64
    dt = np.dtype(reg.VIEW_GAIN_DTYPE)
    assert dt.itemsize == C.sizeof(reg.ViewRecord) == 64
    assert [dt.fields[f][1] for f, _ in reg.ViewRecord._fields_] == abi_kit.offsets("tloam_closed_map_view_record")
    assert [f for f, _ in reg.ViewRecord._fields_] == list(dt.names)
    assert abi_kit.constants("TLOAM_ABI_VERSION") == [8]   # additive: the ABI stays 8
    assert reg.load_library().tloam_abi_version() == 8


def test_view_defaults():
    cfg = reg.default_closed_map_view_config()
    assert [getattr(cfg, f) for f, _ in cfg._fields_] == [20.0, 256 << 20, 131072, 0]
    assert reg.default_closed_map_view_config(max_range=7.5, form=2).form == 2
    with pytest.raises(KeyError):
        reg.default_closed_map_view_config(radius=1.0)
    info = reg.ViewInfo().as_dict()
    assert list(info) == abi_kit.header_structs()["tloam_closed_map_view_info"]
    assert all(v == 0 for v in info.values())
    assert set(reg.VIEW_DIAGNOSTICS) < set(info)
    assert (reg.VIEW_FORM_AUTO, reg.VIEW_FORM_LDS, reg.VIEW_FORM_GLOBAL) == (0, 1, 2)


def test_view_symbols_are_exported():
    abi_kit.assert_exported(VIEW_SYMBOLS)
    names = ("closed_map_view_configure", "closed_map_view_gain", "closed_map_view_cells", "closed_map_frontier_gains",
             "closed_map_view_info")
    sig = {name: list(inspect.signature(getattr(reg.HipRegistration, name)).parameters) for name in names}
    assert sig == {"closed_map_view_configure": ["self", "cfg", "over"], "closed_map_view_gain": ["self", "poses", "ends"],
                   "closed_map_view_cells": ["self", "pose", "ends"], "closed_map_frontier_gains": ["self", "ends"],
                   "closed_map_view_info": ["self"]}
    assert list(inspect.signature(map_io.write_view_pcd).parameters) == ["path", "H", "pose", "ends", "ascii"]
    assert list(inspect.signature(map_io.read_view_pcd).parameters) == ["path"]
