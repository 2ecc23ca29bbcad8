"""The batched localiser and the relocalisation without a GPU: the ctypes mirrors of
tloam_closed_map_relocalise_config / _info / _hypothesis against the C header, the defaults, the entry points in the built
library and the Python methods."""
import ctypes as C
import inspect

import pytest

import abi_kit
from tloam_amd import registration as reg

SYMBOLS = ("tloam_closed_map_localise_batch", "tloam_closed_map_localise_batch_log", "tloam_closed_map_relocalise_default_config",
           "tloam_closed_map_relocalise_configure", "tloam_closed_map_relocalise", "tloam_closed_map_relocalise_hypotheses")


def test_relocalise_struct_layout_matches_the_c_header():
    """(every field of the three mirrors against the header: tests/test_abi_header.py)"""
    assert abi_kit.sizes("tloam_closed_map_relocalise_config", "tloam_closed_map_relocalise_info",
                         "tloam_closed_map_relocalise_hypothesis") == [32, 88, 328]
    assert abi_kit.constants("TLOAM_RELOCALISE_FOUND", "TLOAM_RELOCALISE_NOT_FOUND") \
        == [reg.RELOCALISE_FOUND, reg.RELOCALISE_NOT_FOUND] == [0, 1]
    assert abi_kit.constants("TLOAM_ABI_VERSION") == [8]   # additive: the ABI stays 8


def test_relocalise_defaults():
    cfg = reg.default_closed_map_relocalise_config()
    assert [getattr(cfg, f) for f, _ in cfg._fields_] == [8, 0, float("inf"), 0.5, float("inf")]
    assert reg.default_closed_map_relocalise_config(num_candidates=3, max_dist=0.4).num_candidates == 3
    with pytest.raises(KeyError):
        reg.default_closed_map_relocalise_config(max_iterations=3)
    # default_config fills every field, the reserved one included
    L = reg.load_library()
    raw = reg.ClosedMapRelocaliseConfig()
    C.memset(C.byref(raw), 0xAB, C.sizeof(raw))
    L.tloam_closed_map_relocalise_default_config(C.byref(raw))
    assert bytes(raw) == bytes(cfg)
    assert reg.LOCALISE_MAX_BATCH == 32


def test_relocalise_symbols_are_exported():
    abi_kit.assert_exported(SYMBOLS)
    names = ("closed_map_localise_batch", "closed_map_localise_batch_log", "closed_map_relocalise_configure",
             "closed_map_relocalise", "closed_map_relocalise_hypotheses")
    sig = {name: list(inspect.signature(getattr(reg.HipRegistration, name)).parameters) for name in names}
    assert sig == {"closed_map_localise_batch": ["self", "points", "priors"], "closed_map_localise_batch_log": ["self", "h"],
                   "closed_map_relocalise_configure": ["self", "cfg", "over"], "closed_map_relocalise": ["self", "points"],
                   "closed_map_relocalise_hypotheses": ["self"]}
