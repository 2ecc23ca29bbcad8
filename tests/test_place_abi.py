"""Place recognition without a GPU: the ctypes mirrors of tloam_place_config / _info / _loop against the
C header, the defaults (and the restatement's), the new entry points in the built library, and null arguments.  The invalid
configurations need a context, hence a device: tests/test_gpu_place.py."""
import ctypes as C
import os

import pytest

import abi_kit
from tloam_amd import registration as reg

HERE = os.path.dirname(os.path.abspath(__file__))
PLACE_SYMBOLS = ("tloam_place_default_config", "tloam_place_configure", "tloam_place_get_info", "tloam_place_read_keyframes",
                 "tloam_place_read_loops", "tloam_place_add_scan", "tloam_place_describe")


def test_place_struct_layouts_match_the_c_header():
    """(every field of the three mirrors against the header: tests/test_abi_header.py)"""
    assert abi_kit.sizes("tloam_place_config", "tloam_place_info", "tloam_place_loop") == [72, 32, 56]
    assert C.sizeof(reg.PlaceConfig) == 72 and C.sizeof(reg.PlaceInfo) == 32 and C.sizeof(reg.PlaceLoop) == 56
    assert reg.PlaceConfig.max_radius.offset == 24 and reg.PlaceConfig.reserve_keyframes.offset == 64   # explicit padding


def test_place_defaults():
    c = reg.default_place_config()
    assert (c.enabled, c.n_rings, c.n_sectors, c.num_candidates, c.exclude_recent, c.reserved0) == (0, 20, 60, 10, 50, 0)
    assert (c.max_radius, c.height_offset, c.kf_dist, c.kf_angle, c.dist_thres, c.reserve_keyframes) == (80.0, 2.0, 1.0, 0.2,
                                                                                                         0.30, 0)
    o = reg.default_place_config(enabled=1, n_rings=10, exclude_recent=3, dist_thres=0.25)
    assert (o.enabled, o.n_rings, o.exclude_recent, o.dist_thres) == (1, 10, 3, 0.25)
    with pytest.raises(KeyError):
        reg.default_place_config(radius=10.0)


def test_place_defaults_match_the_restatement():
    import sys
    sys.path.insert(0, HERE)
    import place_np as P
    c = reg.default_place_config()
    for k, v in P.DEFAULTS.items():
        assert getattr(c, k) == v, k


def test_place_symbols_are_exported():
    abi_kit.assert_exported(PLACE_SYMBOLS)


def test_null_arguments_are_refused():
    L = reg.load_library()
    info = reg.PlaceInfo()
    assert L.tloam_place_get_info(None, C.byref(info)) == -1
    assert L.tloam_place_read_keyframes(None, 0, 0, None, None, None, None, None) == -1
    assert L.tloam_place_read_loops(None, 0, 0, None) == -1
    assert L.tloam_place_add_scan(None, None, 0, None, 0, None) == -1
    assert L.tloam_place_describe(None, None, None, 0, None, None, None) == -1
