"""The carve of the closed map without a GPU: the ctypes mirrors of tloam_closed_map_carve_config /
_info against the C header, the defaults, the entry points in the built library and the Python methods."""
import pytest

import abi_kit
from tloam_amd import map_io
from tloam_amd import registration as reg

CARVE_SYMBOLS = ("tloam_closed_map_carve_default_config", "tloam_closed_map_carve_configure", "tloam_closed_map_get_carve_info",
                 "tloam_closed_map_carve", "tloam_closed_map_read_misses", "tloam_closed_map_read_carved")


def test_carve_struct_layout_matches_the_c_header():
    """(every field of both mirrors against the header: tests/test_abi_header.py)"""
    assert abi_kit.sizes("tloam_closed_map_carve_config", "tloam_closed_map_carve_info") == [32, 64]
    assert abi_kit.offsets("tloam_closed_map_carve_config") == [0, 8, 16, 24, 28]
    assert abi_kit.constants("TLOAM_ABI_VERSION") == [8]   # additive: the ABI stays 8


def test_carve_defaults():
    cfg = reg.default_closed_map_carve_config()
    assert (cfg.max_range, cfg.end_margin, cfg.radius, cfg.ray_mask, cfg.reserved0) == (60.0, 1.0, 0.25, 0, 0)
    over = reg.default_closed_map_carve_config(max_range=20.0, end_margin=0.0, radius=float("inf"), ray_mask=0x0F)
    assert (over.max_range, over.end_margin, over.radius, over.ray_mask) == (20.0, 0.0, float("inf"), 0x0F)
    with pytest.raises(KeyError):
        reg.default_closed_map_carve_config(min_miss=3)
    import inspect
    d = {k: p.default for k, p in inspect.signature(reg.HipRegistration.closed_map_read_carved).parameters.items()}
    assert (d["lo"], d["hi"], d["min_count"], d["min_miss"], d["miss_ratio"]) == (None, None, 1, 3, 1.0)


def test_carve_symbols_are_exported():
    abi_kit.assert_exported(CARVE_SYMBOLS)
    for name in ("closed_map_carve_configure", "closed_map_carve", "closed_map_carve_info", "closed_map_misses",
                 "closed_map_read_carved"):
        assert callable(getattr(reg.HipRegistration, name))
    assert callable(map_io.write_carved_closed_map_pcd)
