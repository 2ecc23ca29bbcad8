"""The free space of the closed map without a GPU: the ctypes mirrors of tloam_closed_map_free_config /
_info against the C header, the defaults, the entry points in the built library and the Python methods."""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

import pytest

from tloam_amd import map_io
from tloam_amd import registration as reg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREE_SYMBOLS = ("tloam_closed_map_free_default_config", "tloam_closed_map_free_configure", "tloam_closed_map_get_free_info",
                "tloam_closed_map_free_reset", "tloam_closed_map_free_add_keyframes", "tloam_closed_map_free_add_scan",
                "tloam_closed_map_occupancy", "tloam_closed_map_read_free", "tloam_closed_map_free_columns",
                "tloam_closed_map_read_free_words")
CFG_FIELDS = ("max_range", "end_margin", "max_bytes", "min_count", "min_miss", "miss_ratio", "ray_mask", "carve_gate")
INFO_FIELDS = ("lo_cells", "n_bricks", "bytes", "keyframes", "scans", "free_cells", "bricks_nonzero", "rays", "skipped_rays",
               "cells_marked", "cells_outside", "launches", "reserved0")


def test_free_struct_layout_matches_the_c_header():
    structs = (("tloam_closed_map_free_config", CFG_FIELDS, reg.FreeConfig), ("tloam_closed_map_free_info", INFO_FIELDS, reg.FreeInfo))
    exprs = [f"sizeof({name})" for name, _, _ in structs] + [f"offsetof({name}, {f})" for name, fields, _ in structs for f in fields]
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "tloam_hip.h"
int main(void) {
  size_t v[] = {%s};
  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%%zu ", v[i]);
  printf("%%d %%d %%d %%d %%d\n", TLOAM_OCCUPANCY_INVALID, TLOAM_OCCUPANCY_UNKNOWN, TLOAM_OCCUPANCY_FREE, TLOAM_OCCUPANCY_OCCUPIED,
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
    assert vals[:2] == [56, 128]
    assert vals[-5:-1] == [reg.OCCUPANCY_INVALID, reg.OCCUPANCY_UNKNOWN, reg.OCCUPANCY_FREE, reg.OCCUPANCY_OCCUPIED] == [0, 1, 2, 3]
    assert vals[-1] == 8   # additive: the ABI stays 8
    assert reg.load_library().tloam_abi_version() == 8


def test_free_defaults():
    cfg = reg.default_closed_map_free_config()
    assert [getattr(cfg, f) for f in CFG_FIELDS] == [60.0, 1.0, 1 << 30, 1, 3, 1.0, 0, 0]
    carve, diff = reg.default_closed_map_carve_config(), reg.default_closed_map_diff_config()
    assert (cfg.max_range, cfg.end_margin, cfg.ray_mask) == (carve.max_range, carve.end_margin, carve.ray_mask)   # the carve's rays
    assert (cfg.min_miss, cfg.miss_ratio, cfg.carve_gate) == (diff.min_miss, diff.miss_ratio, diff.carve_gate)     # the diff's gate
    assert reg.default_closed_map_free_config(carve_gate=1, max_bytes=4096).max_bytes == 4096
    with pytest.raises(KeyError):
        reg.default_closed_map_free_config(radius=1.0)
    info = reg.FreeInfo().as_dict()
    assert list(info) == list(INFO_FIELDS) and info["lo_cells"] == (0, 0, 0) and info["n_bricks"] == (0, 0, 0)


def test_free_symbols_are_exported():
    L = reg.load_library()
    for name in FREE_SYMBOLS:
        assert name in reg.EXPORTED_SYMBOLS
        getattr(L, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", reg.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(FREE_SYMBOLS) <= exported
    names = ("closed_map_free_configure", "closed_map_free_reset", "closed_map_free_add_keyframes", "closed_map_free_add_scan",
             "closed_map_free_info", "closed_map_free_build", "closed_map_occupancy", "closed_map_free_cells",
             "closed_map_free_columns")
    sig = {name: list(inspect.signature(getattr(reg.HipRegistration, name)).parameters) for name in names}
    assert sig == {"closed_map_free_configure": ["self", "cfg", "over"], "closed_map_free_reset": ["self", "lo_cells", "hi_cells"],
                   "closed_map_free_add_keyframes": ["self"], "closed_map_free_add_scan": ["self", "points", "pose"],
                   "closed_map_free_info": ["self"], "closed_map_free_build": ["self", "lo_cells", "hi_cells"],
                   "closed_map_occupancy": ["self", "points", "pose", "want_ids"], "closed_map_free_cells": ["self", "lo", "hi"],
                   "closed_map_free_columns": ["self", "z_lo", "z_hi", "min_free"]}
    assert inspect.signature(reg.HipRegistration.closed_map_occupancy).parameters["pose"].default is None
    assert inspect.signature(reg.HipRegistration.closed_map_free_columns).parameters["min_free"].default == 1
    assert list(inspect.signature(map_io.write_free_pcd).parameters) == ["path", "H", "lo", "hi", "ascii"]
