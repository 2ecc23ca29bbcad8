"""The diff of a scan against the closed map without a GPU: the ctypes mirrors of
tloam_closed_map_diff_config / _info against the C header, the defaults, the entry points in the built library and the Python
methods."""
import inspect

import pytest

import abi_kit
from tloam_amd import registration as reg

DIFF_SYMBOLS = ("tloam_closed_map_diff_default_config", "tloam_closed_map_diff_configure", "tloam_closed_map_get_diff_info",
                "tloam_closed_map_diff", "tloam_closed_map_read_diff", "tloam_closed_map_read_gone")


def test_diff_struct_layout_matches_the_c_header():
    """(every field of both mirrors against the header: tests/test_abi_header.py)"""
    assert abi_kit.sizes("tloam_closed_map_diff_config", "tloam_closed_map_diff_info") == [64, 120]
    assert abi_kit.constants("TLOAM_DIFF_INVALID", "TLOAM_DIFF_SURFACE", "TLOAM_DIFF_OCCUPIED", "TLOAM_DIFF_NEW") \
        == [reg.DIFF_INVALID, reg.DIFF_SURFACE, reg.DIFF_OCCUPIED, reg.DIFF_NEW] == [0, 1, 2, 3]
    assert abi_kit.constants("TLOAM_DIFF_ACCUMULATE") == [reg.DIFF_ACCUMULATE] == [1]
    assert abi_kit.constants("TLOAM_ABI_VERSION") == [8]   # additive: the ABI stays 8


def test_diff_defaults():
    cfg = reg.default_closed_map_diff_config()
    assert [getattr(cfg, f) for f, _ in cfg._fields_] == [60.0, 1.0, 0.25, 0.1, 0.5, 3, 1.0, 0, 0]
    carve, loc = reg.default_closed_map_carve_config(), reg.default_closed_map_localise_config()
    assert (cfg.max_range, cfg.end_margin, cfg.radius) == (carve.max_range, carve.end_margin, carve.radius)
    assert cfg.plane_tol == loc.min_residual
    assert reg.default_closed_map_diff_config(max_range=20.0, carve_gate=1).carve_gate == 1
    with pytest.raises(KeyError):
        reg.default_closed_map_diff_config(ray_mask=3)
    gone = inspect.signature(reg.HipRegistration.closed_map_read_gone).parameters
    assert (gone["min_through"].default, gone["gone_ratio"].default) == (3, 1.0)


def test_diff_symbols_are_exported():
    abi_kit.assert_exported(DIFF_SYMBOLS)
    sig = {name: list(inspect.signature(getattr(reg.HipRegistration, name)).parameters) for name in
           ("closed_map_diff_configure", "closed_map_diff", "closed_map_diff_info", "closed_map_diff_counts", "closed_map_read_gone")}
    assert sig == {"closed_map_diff_configure": ["self", "cfg", "over"],
                   "closed_map_diff": ["self", "points", "pose", "accumulate", "want_ids"], "closed_map_diff_info": ["self"],
                   "closed_map_diff_counts": ["self", "first", "count"],
                   "closed_map_read_gone": ["self", "lo", "hi", "min_through", "gone_ratio"]}
    diff = inspect.signature(reg.HipRegistration.closed_map_diff).parameters
    assert diff["accumulate"].default is False and diff["want_ids"].default is False
