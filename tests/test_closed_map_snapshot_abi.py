"""The closed map's snapshot without a GPU: the ctypes mirror of tloam_closed_map_snapshot_info against the
C header, the entry points in the built library and the Python methods."""
import ctypes as C
import inspect

import abi_kit
from tloam_amd import map_io, registration as reg

SYMBOLS = ("tloam_closed_map_save_size", "tloam_closed_map_save", "tloam_closed_map_probe", "tloam_closed_map_load")


def test_snapshot_struct_layout_matches_the_c_header():
    """(every field of the mirror against the header: tests/test_abi_header.py)"""
    assert abi_kit.sizes("tloam_closed_map_snapshot_info") == [112]
    assert abi_kit.constants("TLOAM_SNAPSHOT_CLOUDS", "TLOAM_SNAPSHOT_FORMAT_VERSION") == [reg.SNAPSHOT_CLOUDS, 1] == [1, 1]
    assert abi_kit.constants("TLOAM_ABI_VERSION") == [8]   # additive: the ABI stays 8


def test_snapshot_symbols_are_exported():
    assert reg.load_library().tloam_abi_version() == 8
    abi_kit.assert_exported(SYMBOLS)
    sig = {name: list(inspect.signature(getattr(reg.HipRegistration, name)).parameters) for name in ("closed_map_save", "closed_map_load")}
    assert sig == {"closed_map_save": ["self", "clouds"], "closed_map_load": ["self", "blob"]}
    assert inspect.signature(reg.HipRegistration.closed_map_save).parameters["clouds"].default is False
    assert list(inspect.signature(reg.closed_map_probe).parameters) == ["blob"]
    assert list(inspect.signature(map_io.save_closed_map).parameters) == ["path", "H", "clouds"]
    assert list(inspect.signature(map_io.load_closed_map).parameters) == ["path", "H"]


def test_snapshot_calls_refuse_null_arguments_without_a_context():
    L = reg.load_library()
    info, n = reg.ClosedMapSnapshotInfo(), C.c_size_t(7)
    assert L.tloam_closed_map_probe(None, 0, C.byref(info)) == -1
    assert L.tloam_closed_map_probe(b"\0" * 8, 8, None) == -1
    assert L.tloam_closed_map_save_size(None, 0, C.byref(n)) == -1
    assert L.tloam_closed_map_save(None, 0, None, 0, C.byref(n)) == -1
    assert L.tloam_closed_map_load(None, b"\0" * 8, 8, None) == -1
