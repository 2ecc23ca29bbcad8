"""The closed map's extension without a GPU: the ctypes mirror of tloam_closed_map_extend_info against
the C header, the entry points in the built library and the Python methods."""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

from tloam_amd import registration as reg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTEND_SYMBOLS = ("tloam_closed_map_extend", "tloam_closed_map_get_extend_info")
INFO_FIELDS = ("first_keyframe", "n_keyframes", "added_keyframes", "empty_keyframes", "overflow_keyframes", "points", "new_voxels",
               "touched_voxels", "rays", "skipped_rays", "steps", "tested", "misses", "solved_voxels", "grown", "launches")


def test_extend_struct_layout_matches_the_c_header():
    name, cls = "tloam_closed_map_extend_info", reg.ClosedMapExtendInfo
    exprs = [f"sizeof({name})"] + [f"offsetof({name}, {f})" for f in INFO_FIELDS]
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "tloam_hip.h"
int main(void) {
  size_t v[] = {%s};
  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%%zu ", v[i]);
  printf("%%d %%d %%d %%d\n", TLOAM_CLOSED_MAP_POSES_STORED, TLOAM_CLOSED_MAP_POSES_CORRECTED, TLOAM_CLOSED_MAP_POSES_CALLER,
         TLOAM_ABI_VERSION);
  return 0;
}''' % ", ".join(exprs)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c"); exe = os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = list(map(int, subprocess.check_output([exe]).split()))
    assert [n for n, _ in cls._fields_] == list(INFO_FIELDS)
    assert vals[:-4] == [C.sizeof(cls)] + [getattr(cls, f).offset for f in INFO_FIELDS]
    assert vals[0] == 120
    assert vals[-4:-1] == [0, 1, 2]
    assert vals[-1] == 8   # additive: the ABI stays 8
    assert set(reg.ClosedMapExtendInfo().as_dict()) == set(INFO_FIELDS)


def test_extend_symbols_are_exported():
    L = reg.load_library()
    for name in EXTEND_SYMBOLS:
        assert name in reg.EXPORTED_SYMBOLS
        getattr(L, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", reg.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(EXTEND_SYMBOLS) <= exported
    sig = {name: list(inspect.signature(getattr(reg.HipRegistration, name)).parameters) for name in
           ("closed_map_extend", "closed_map_extend_info")}
    assert sig == {"closed_map_extend": ["self", "pose_source", "poses"], "closed_map_extend_info": ["self"]}
    ext = inspect.signature(reg.HipRegistration.closed_map_extend).parameters
    assert ext["pose_source"].default == 0 and ext["poses"].default is None
