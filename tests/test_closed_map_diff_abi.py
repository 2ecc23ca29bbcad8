"""The diff of a scan against the closed map without a GPU: the ctypes mirrors of
tloam_closed_map_diff_config / _info against the C header, the defaults, the entry points in the built library and the Python
methods."""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

import pytest

from tloam_amd import registration as reg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIFF_SYMBOLS = ("tloam_closed_map_diff_default_config", "tloam_closed_map_diff_configure", "tloam_closed_map_get_diff_info",
                "tloam_closed_map_diff", "tloam_closed_map_read_diff", "tloam_closed_map_read_gone")
CFG_FIELDS = ("max_range", "end_margin", "radius", "plane_tol", "near", "min_miss", "miss_ratio", "carve_gate", "reserved0")
INFO_FIELDS = ("n_points", "n_invalid", "n_surface", "n_occupied", "n_new", "rays", "skipped_rays", "steps", "tested", "through",
               "voxels_through", "voxels_hit", "scans", "launches", "prepared", "cleared", "reserved0")


def test_diff_struct_layout_matches_the_c_header():
    structs = (("tloam_closed_map_diff_config", CFG_FIELDS, reg.ClosedMapDiffConfig),
               ("tloam_closed_map_diff_info", INFO_FIELDS, reg.ClosedMapDiffInfo))
    exprs = [f"sizeof({name})" for name, _, _ in structs] + [f"offsetof({name}, {f})" for name, fields, _ in structs for f in fields]
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "tloam_hip.h"
int main(void) {
  size_t v[] = {%s};
  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%%zu ", v[i]);
  printf("%%d %%d %%d %%d %%d %%d\n", TLOAM_DIFF_INVALID, TLOAM_DIFF_SURFACE, TLOAM_DIFF_OCCUPIED, TLOAM_DIFF_NEW,
         TLOAM_DIFF_ACCUMULATE, TLOAM_ABI_VERSION);
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
    assert vals[:-6] == want
    assert vals[:2] == [64, 120]
    assert vals[-6:-2] == [reg.DIFF_INVALID, reg.DIFF_SURFACE, reg.DIFF_OCCUPIED, reg.DIFF_NEW] == [0, 1, 2, 3]
    assert vals[-2] == reg.DIFF_ACCUMULATE == 1
    assert vals[-1] == 8   # additive: the ABI stays 8


def test_diff_defaults():
    cfg = reg.default_closed_map_diff_config()
    assert [getattr(cfg, f) for f in CFG_FIELDS] == [60.0, 1.0, 0.25, 0.1, 0.5, 3, 1.0, 0, 0]
    carve, loc = reg.default_closed_map_carve_config(), reg.default_closed_map_localise_config()
    assert (cfg.max_range, cfg.end_margin, cfg.radius) == (carve.max_range, carve.end_margin, carve.radius)
    assert cfg.plane_tol == loc.min_residual
    assert reg.default_closed_map_diff_config(max_range=20.0, carve_gate=1).carve_gate == 1
    with pytest.raises(KeyError):
        reg.default_closed_map_diff_config(ray_mask=3)
    gone = inspect.signature(reg.HipRegistration.closed_map_read_gone).parameters
    assert (gone["min_through"].default, gone["gone_ratio"].default) == (3, 1.0)


def test_diff_symbols_are_exported():
    L = reg.load_library()
    for name in DIFF_SYMBOLS:
        assert name in reg.EXPORTED_SYMBOLS
        getattr(L, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", reg.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(DIFF_SYMBOLS) <= exported
    sig = {name: list(inspect.signature(getattr(reg.HipRegistration, name)).parameters) for name in
           ("closed_map_diff_configure", "closed_map_diff", "closed_map_diff_info", "closed_map_diff_counts", "closed_map_read_gone")}
    assert sig == {"closed_map_diff_configure": ["self", "cfg", "over"],
                   "closed_map_diff": ["self", "points", "pose", "accumulate", "want_ids"], "closed_map_diff_info": ["self"],
                   "closed_map_diff_counts": ["self", "first", "count"],
                   "closed_map_read_gone": ["self", "lo", "hi", "min_through", "gone_ratio"]}
    diff = inspect.signature(reg.HipRegistration.closed_map_diff).parameters
    assert diff["accumulate"].default is False and diff["want_ids"].default is False
