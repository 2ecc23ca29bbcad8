"""The closed map's extension without a GPU: the ctypes mirror of tloam_closed_map_extend_info against
the C header, the entry points in the built library and the Python methods."""
import inspect

import abi_kit
from tloam_amd import registration as reg

EXTEND_SYMBOLS = ("tloam_closed_map_extend", "tloam_closed_map_get_extend_info")


def test_extend_struct_layout_matches_the_c_header():
    """(every field of the mirror against the header: tests/test_abi_header.py)"""
    assert abi_kit.sizes("tloam_closed_map_extend_info") == [120]
    assert abi_kit.constants("TLOAM_CLOSED_MAP_POSES_STORED", "TLOAM_CLOSED_MAP_POSES_CORRECTED",
                             "TLOAM_CLOSED_MAP_POSES_CALLER") == [0, 1, 2]
    assert abi_kit.constants("TLOAM_ABI_VERSION") == [8]   # additive: the ABI stays 8
    assert set(reg.ClosedMapExtendInfo().as_dict()) == set(abi_kit.header_structs()["tloam_closed_map_extend_info"])


def test_extend_symbols_are_exported():
    abi_kit.assert_exported(EXTEND_SYMBOLS)
    sig = {name: list(inspect.signature(getattr(reg.HipRegistration, name)).parameters) for name in
           ("closed_map_extend", "closed_map_extend_info")}
    assert sig == {"closed_map_extend": ["self", "pose_source", "poses"], "closed_map_extend_info": ["self"]}
    ext = inspect.signature(reg.HipRegistration.closed_map_extend).parameters
    assert ext["pose_source"].default == 0 and ext["poses"].default is None
