"""The surfels of the closed map without a GPU: the ctypes mirrors of tloam_closed_map_surfel_config /
_info against the C header, the defaults, the entry points in the built library and the Python methods."""
import inspect

import pytest

import abi_kit
from tloam_amd import map_io
from tloam_amd import registration as reg

SURFEL_SYMBOLS = ("tloam_closed_map_surfel_default_config", "tloam_closed_map_surfel_configure", "tloam_closed_map_get_surfel_info",
                  "tloam_closed_map_surfels", "tloam_closed_map_read_moments", "tloam_closed_map_read_surfels",
                  "tloam_closed_map_read_surfels_box")


def test_surfel_struct_layout_matches_the_c_header():
    """(every field of both mirrors against the header: tests/test_abi_header.py)"""
    assert abi_kit.sizes("tloam_closed_map_surfel_config", "tloam_closed_map_surfel_info") == [8, 40]
    assert abi_kit.offsets("tloam_closed_map_surfel_config") == [0, 4]
    assert abi_kit.offsets("tloam_closed_map_surfel_info") == [0, 8, 16, 24, 32, 36]
    assert abi_kit.constants("TLOAM_ABI_VERSION") == [8]   # additive: the ABI stays 8


def test_surfel_defaults():
    cfg = reg.default_closed_map_surfel_config()
    assert (cfg.min_points, cfg.reserved0) == (5, 0)
    assert reg.default_closed_map_surfel_config(min_points=3).min_points == 3
    with pytest.raises(KeyError):
        reg.default_closed_map_surfel_config(min_planarity=0.1)
    d = {k: p.default for k, p in inspect.signature(reg.HipRegistration.closed_map_read_surfels_box).parameters.items()}
    assert (d["lo"], d["hi"], d["min_count"], d["max_sigma"], d["min_planarity"]) == (None, None, 1, float("inf"), 0.05)


def test_surfel_symbols_are_exported():
    abi_kit.assert_exported(SURFEL_SYMBOLS)
    for name in ("closed_map_surfel_configure", "closed_map_surfels", "closed_map_surfel_info", "closed_map_moments",
                 "closed_map_read_surfels", "closed_map_read_surfels_box"):
        assert callable(getattr(reg.HipRegistration, name))
    for name in ("write_surfel_pcd", "read_surfel_pcd", "write_closed_map_surfel_pcd"):
        assert callable(getattr(map_io, name))
