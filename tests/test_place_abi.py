"""Place recognition without a GPU: the ctypes mirrors of tloam_place_config / _info / _loop against the
C header, the defaults (and the restatement's), the new entry points in the built library, and null arguments.  The invalid
configurations need a context, hence a device: tests/test_gpu_place.py."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from tloam_amd import registration as reg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PLACE_SYMBOLS = ("tloam_place_default_config", "tloam_place_configure", "tloam_place_get_info", "tloam_place_read_keyframes",
                 "tloam_place_read_loops", "tloam_place_add_scan", "tloam_place_describe")


def _probe(structs):
    """sizeof and offsetof of every field of `structs` ({C name: ctypes class}) as the C compiler lays them out"""
    lines = []
    for cname, cls in structs.items():
        lines.append(f'  printf("%zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'  printf("%zu\\n", offsetof({cname}, {f}));')
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "tloam_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c"); exe = os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        return list(map(int, subprocess.check_output([exe]).split()))


def test_place_struct_layouts_match_the_c_header():
    structs = {"tloam_place_config": reg.PlaceConfig, "tloam_place_info": reg.PlaceInfo, "tloam_place_loop": reg.PlaceLoop}
    want = []
    for cls in structs.values():
        want.append(C.sizeof(cls))
        want += [getattr(cls, f).offset for f, _ in cls._fields_]
    got = _probe(structs)
    assert got == want
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
    L = reg.load_library()
    for name in PLACE_SYMBOLS:
        assert name in reg.EXPORTED_SYMBOLS
        getattr(L, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", reg.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(PLACE_SYMBOLS) <= exported


def test_null_arguments_are_refused():
    L = reg.load_library()
    info = reg.PlaceInfo()
    assert L.tloam_place_get_info(None, C.byref(info)) == -1
    assert L.tloam_place_read_keyframes(None, 0, 0, None, None, None, None, None) == -1
    assert L.tloam_place_read_loops(None, 0, 0, None) == -1
    assert L.tloam_place_add_scan(None, None, 0, None, 0, None) == -1
    assert L.tloam_place_describe(None, None, None, 0, None, None, None) == -1
