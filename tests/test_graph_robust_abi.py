"""The robust mode of the pose graph without a GPU: the ctypes mirrors of tloam_graph_robust_config /
_info against the C header, the defaults, and the entry points in the built library."""
import ctypes as C

import pytest

import abi_kit
from tloam_amd import registration as reg

ROBUST_SYMBOLS = ("tloam_graph_robust_default_config", "tloam_graph_robust_configure", "tloam_graph_solve_robust",
                  "tloam_graph_read_loop_scales", "tloam_graph_get_robust_info")


def test_graph_robust_struct_layout_matches_the_c_header():
    """(every field of both mirrors against the header: tests/test_abi_header.py)"""
    assert abi_kit.sizes("tloam_graph_robust_config", "tloam_graph_robust_info") == [24, 72]
    assert abi_kit.offsets("tloam_graph_robust_config") == [0, 4, 8, 16]
    assert abi_kit.constants("TLOAM_GRAPH_ROBUST_STOP_OFF", "TLOAM_GRAPH_ROBUST_STOP_ALL_INLIERS", "TLOAM_GRAPH_ROBUST_STOP_BINARY",
                             "TLOAM_GRAPH_ROBUST_STOP_OUTER_LIMIT", "TLOAM_ABI_VERSION") == [0, 1, 2, 3, 8]   # additive: the ABI stays 8
    assert reg.GRAPH_ROBUST_STOP == {0: "off", 1: "all_inliers", 2: "binary", 3: "outer_limit"}


def test_the_abi_version_is_still_8_and_the_graph_structs_are_unchanged():
    assert reg.load_library().tloam_abi_version() == 8
    assert C.sizeof(reg.GraphConfig) == 56 and C.sizeof(reg.GraphInfo) == 80 and C.sizeof(reg.GraphEdge) == 192


def test_graph_robust_defaults():
    cfg = reg.default_graph_robust_config()
    assert (cfg.enabled, cfg.max_outer, cfg.noise_chi2, cfg.mu_factor) == (0, 100, 36.0, 1.4)
    over = reg.default_graph_robust_config(enabled=1, noise_chi2=16.81, mu_factor=2.0, max_outer=7)
    assert (over.enabled, over.max_outer, over.noise_chi2, over.mu_factor) == (1, 7, 16.81, 2.0)
    with pytest.raises(KeyError):
        reg.default_graph_robust_config(chi2=9.0)


def test_graph_robust_symbols_are_exported():
    abi_kit.assert_exported(ROBUST_SYMBOLS)
    for name in ("graph_robust_configure", "graph_solve_robust", "graph_read_loop_scales", "graph_robust_info"):
        assert callable(getattr(reg.HipRegistration, name))
