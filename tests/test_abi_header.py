"""The whole of include/tloam_hip.h against tloam_amd/abi.py, without a GPU: every struct typedef has one ctypes mirror with the
header's field names in the header's order and gcc's sizeof, offsetof and member sizes; every declared function has one
SIGNATURES line and is exported by the built library.  (Two neighbours of equal size swapped in a mirror change no size and no
offset: the name order is what catches them.)"""
import ctypes as C
import inspect

import abi_kit
from tloam_amd import abi
from tloam_amd import registration as reg

MIRRORS = [c for c in vars(abi).values() if inspect.isclass(c) and issubclass(c, abi.Struct) and c is not abi.Struct]


def test_every_struct_typedef_has_exactly_one_mirror():
    header = abi_kit.header_structs()
    assert "tloam_ctx" not in header and "tloam_status" not in header   # the opaque handle; an enum
    names = [c._c_name_ for c in MIRRORS]
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    assert set(names) == set(header), (sorted(set(header) - set(names)), sorted(set(names) - set(header)))
    assert len(header) >= 46   # (a parse that finds nothing must not pass)
    for c in MIRRORS:
        assert getattr(reg, c.__name__) is c   # registration re-exports the mirror itself


def test_every_mirror_has_the_headers_field_names_in_order():
    header = abi_kit.header_structs()
    wrong = {c._c_name_: ([f for f, _ in c._fields_], header[c._c_name_]) for c in MIRRORS
             if [f for f, _ in c._fields_] != header[c._c_name_]}
    assert not wrong, wrong


def test_every_mirror_has_the_c_layout():
    wrong, checked = [], 0
    for c in MIRRORS:
        name, fields = c._c_name_, abi_kit.header_structs()[c._c_name_]
        got = (abi_kit.sizes(name), abi_kit.offsets(name), abi_kit.member_sizes(name))
        want = ([C.sizeof(c)], [getattr(c, f).offset for f in fields], [getattr(c, f).size for f in fields])
        if got != want:
            wrong.append((name, got, want))
        checked += 1 + 2 * len(fields)
    assert not wrong, wrong
    assert len(MIRRORS) >= 46 and checked >= 866


def test_signatures_are_the_declared_functions_and_all_are_exported():
    declared = abi_kit.declared_functions()
    assert len(declared) >= 160
    assert set(abi.SIGNATURES) == declared, (sorted(declared - set(abi.SIGNATURES)), sorted(set(abi.SIGNATURES) - declared))
    assert reg.EXPORTED_SYMBOLS == tuple(abi.SIGNATURES) and reg.SIGNATURES is abi.SIGNATURES
    assert declared <= abi_kit.exported(), sorted(declared - abi_kit.exported())
    L = reg.load_library()
    for name, (res, args) in abi.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
