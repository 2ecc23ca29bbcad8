"""The ray-cast of the closed map without a GPU: the ctypes mirrors of tloam_closed_map_raycast_config /
_info against the C header, the defaults, the entry points in the built library and the Python methods."""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

import pytest

from tloam_amd import raycast as RC
from tloam_amd import registration as reg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAYCAST_SYMBOLS = ("tloam_closed_map_raycast_default_config", "tloam_closed_map_raycast_configure",
                   "tloam_closed_map_get_raycast_info", "tloam_closed_map_raycast")
CFG_FIELDS = ("max_range", "radius_cells", "min_count", "min_miss", "miss_ratio", "planes", "carve_gate")
INFO_FIELDS = ("rays", "skipped", "missed", "hits_centroid", "hits_plane", "steps", "tested", "launches", "prepared")


def test_raycast_struct_layout_matches_the_c_header():
    structs = (("tloam_closed_map_raycast_config", CFG_FIELDS, reg.ClosedMapRaycastConfig),
               ("tloam_closed_map_raycast_info", INFO_FIELDS, reg.ClosedMapRaycastInfo))
    exprs = [f"sizeof({name})" for name, _, _ in structs] + [f"offsetof({name}, {f})" for name, fields, _ in structs for f in fields]
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "tloam_hip.h"
int main(void) {
  size_t v[] = {%s};
  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%%zu ", v[i]);
  printf("%%d %%d %%d %%d %%d\n", TLOAM_RAYCAST_SKIPPED, TLOAM_RAYCAST_MISS, TLOAM_RAYCAST_HIT_CENTROID, TLOAM_RAYCAST_HIT_PLANE,
         TLOAM_ABI_VERSION);
  return 0;
}''' % ", ".join(exprs)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c"); exe = os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = list(map(int, subprocess.check_output([exe]).split()))
    for _, fields, cls in structs:
        assert [n for n, _ in cls._fields_] == list(fields)
    want = [C.sizeof(cls) for _, _, cls in structs] + [getattr(cls, f).offset for _, fields, cls in structs for f in fields]
    assert vals[:-5] == want
    assert vals[:2] == [48, 64]
    assert vals[-5:-1] == [reg.RAYCAST_SKIPPED, reg.RAYCAST_MISS, reg.RAYCAST_HIT_CENTROID, reg.RAYCAST_HIT_PLANE] == [0, 1, 2, 3]
    assert (RC.RAYCAST_SKIPPED, RC.RAYCAST_MISS, RC.RAYCAST_HIT_CENTROID, RC.RAYCAST_HIT_PLANE) == (0, 1, 2, 3)
    assert vals[-1] == 8   # additive: the ABI stays 8


def test_raycast_defaults():
    cfg = reg.default_closed_map_raycast_config()
    assert [getattr(cfg, f) for f in CFG_FIELDS] == [120.0, 0.75, 1, 3, 1.0, 1, 0]
    diff = reg.default_closed_map_diff_config()
    assert (cfg.min_miss, cfg.miss_ratio, cfg.carve_gate) == (diff.min_miss, diff.miss_ratio, diff.carve_gate)   # the diff's gate
    assert reg.default_closed_map_raycast_config(planes=2, carve_gate=1).planes == 2
    with pytest.raises(KeyError):
        reg.default_closed_map_raycast_config(end_margin=1.0)


def test_raycast_symbols_are_exported():
    L = reg.load_library()
    for name in RAYCAST_SYMBOLS:
        assert name in reg.EXPORTED_SYMBOLS
        getattr(L, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", reg.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(RAYCAST_SYMBOLS) <= exported
    sig = {name: list(inspect.signature(getattr(reg.HipRegistration, name)).parameters) for name in
           ("closed_map_raycast_configure", "closed_map_raycast", "closed_map_raycast_info")}
    assert sig == {"closed_map_raycast_configure": ["self", "cfg", "over"],
                   "closed_map_raycast": ["self", "ends", "pose", "want_ids"], "closed_map_raycast_info": ["self"]}
    assert inspect.signature(reg.HipRegistration.closed_map_raycast).parameters["want_ids"].default is False
    assert list(inspect.signature(RC.lidar_pattern).parameters) == ["rings", "n_az", "elev_lo", "elev_hi", "length"]
    assert list(inspect.signature(RC.scan_check).parameters) == ["H", "points", "pose", "extend"]
    assert inspect.signature(RC.scan_check).parameters["extend"].default == 2.0
