"""The localisation in the closed map without a GPU: the ctypes mirrors of
tloam_closed_map_localise_config / _info / _record against the C header, the defaults, the entry points in the built library and
the Python methods."""
import inspect

import pytest

import abi_kit
from tloam_amd import registration as reg

LOCALISE_SYMBOLS = ("tloam_closed_map_localise_default_config", "tloam_closed_map_localise_configure", "tloam_closed_map_localise",
                    "tloam_closed_map_localise_log", "tloam_closed_map_linearise")


def test_localise_struct_layout_matches_the_c_header():
    """(every field of the three mirrors against the header: tests/test_abi_header.py)"""
    assert abi_kit.sizes("tloam_closed_map_localise_config", "tloam_closed_map_localise_info",
                         "tloam_closed_map_localise_record") == [72, 40, 208]
    assert abi_kit.constants("TLOAM_LOCALISE_CONVERGED", "TLOAM_LOCALISE_MAX_ITERATIONS", "TLOAM_LOCALISE_DEGENERATE") \
        == [reg.LOCALISE_CONVERGED, reg.LOCALISE_MAX_ITERATIONS, reg.LOCALISE_DEGENERATE] == [0, 1, 2]
    assert abi_kit.constants("TLOAM_ABI_VERSION") == [8]   # additive: the ABI stays 8


def test_localise_defaults():
    cfg = reg.default_closed_map_localise_config()
    assert [getattr(cfg, f) for f, _ in cfg._fields_] == [1.0, 0.7, 0.1, float("inf"), 0.05, 1e-6, 1e-7, 1e-9, 20, 50]
    assert reg.default_closed_map_localise_config(max_iterations=5, shrink=0.5).max_iterations == 5
    with pytest.raises(KeyError):
        reg.default_closed_map_localise_config(min_points=3)


def test_localise_symbols_are_exported():
    abi_kit.assert_exported(LOCALISE_SYMBOLS)
    sig = {name: list(inspect.signature(getattr(reg.HipRegistration, name)).parameters) for name in
           ("closed_map_localise_configure", "closed_map_localise", "closed_map_localise_log", "closed_map_linearise")}
    assert sig == {"closed_map_localise_configure": ["self", "cfg", "over"], "closed_map_localise": ["self", "points", "prior"],
                   "closed_map_localise_log": ["self"], "closed_map_linearise": ["self", "points", "pose", "tau"]}
