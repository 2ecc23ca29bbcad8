"""The closed map's snapshot without a GPU: the ctypes mirror of tloam_closed_map_snapshot_info against the
C header, the entry points in the built library and the Python methods."""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

from tloam_amd import map_io, registration as reg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tloam_closed_map_save_size", "tloam_closed_map_save", "tloam_closed_map_probe", "tloam_closed_map_load")
FIELDS = ("format_version", "flags", "n_keyframes_database", "n_keyframes_map", "n_voxels", "n_points", "has_carve", "has_surfels",
          "has_clouds", "n_rings", "n_sectors", "reserved0", "cloud_points", "voxel", "origin", "bytes")


def test_snapshot_struct_layout_matches_the_c_header():
    name, cls = "tloam_closed_map_snapshot_info", reg.ClosedMapSnapshotInfo
    exprs = [f"sizeof({name})"] + [f"offsetof({name}, {f})" for f in FIELDS]
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "tloam_hip.h"
int main(void) {
  size_t v[] = {%s};
  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%%zu ", v[i]);
  printf("%%d %%d %%d\n", TLOAM_SNAPSHOT_CLOUDS, TLOAM_SNAPSHOT_FORMAT_VERSION, TLOAM_ABI_VERSION);
  return 0;
}''' % ", ".join(exprs)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c"); exe = os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = list(map(int, subprocess.check_output([exe]).split()))
    assert [n for n, _ in cls._fields_] == list(FIELDS)
    assert vals[:-3] == [C.sizeof(cls)] + [getattr(cls, f).offset for f in FIELDS]
    assert vals[0] == 112
    assert vals[-3:-1] == [reg.SNAPSHOT_CLOUDS, 1] == [1, 1]
    assert vals[-1] == 8   # additive: the ABI stays 8


def test_snapshot_symbols_are_exported():
    L = reg.load_library()
    assert L.tloam_abi_version() == 8
    for name in SYMBOLS:
        assert name in reg.EXPORTED_SYMBOLS
        getattr(L, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", reg.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= exported
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
