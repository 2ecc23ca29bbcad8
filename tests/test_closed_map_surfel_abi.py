"""The surfels of the closed map without a GPU: the ctypes mirrors of tloam_closed_map_surfel_config /
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
SURFEL_SYMBOLS = ("tloam_closed_map_surfel_default_config", "tloam_closed_map_surfel_configure", "tloam_closed_map_get_surfel_info",
                  "tloam_closed_map_surfels", "tloam_closed_map_read_moments", "tloam_closed_map_read_surfels",
                  "tloam_closed_map_read_surfels_box")


def test_surfel_struct_layout_matches_the_c_header():
    cfg_fields = ("min_points", "reserved0")
    info_fields = ("n_keyframes", "n_points", "orphan_points", "solved_voxels", "launches", "reserved0")
    offs = ", ".join([f"offsetof(tloam_closed_map_surfel_config, {f})" for f in cfg_fields] +
                     [f"offsetof(tloam_closed_map_surfel_info, {f})" for f in info_fields])
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "tloam_hip.h"
int main(void) {
  size_t v[] = {sizeof(tloam_closed_map_surfel_config), sizeof(tloam_closed_map_surfel_info), %s};
  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%%zu ", v[i]);
  printf("%%d\n", TLOAM_ABI_VERSION);
  return 0;
}''' % offs
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c"); exe = os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = list(map(int, subprocess.check_output([exe]).split()))
    M, I = reg.ClosedMapSurfelConfig, reg.ClosedMapSurfelInfo
    assert [n for n, _ in M._fields_] == list(cfg_fields) and [n for n, _ in I._fields_] == list(info_fields)
    want = [C.sizeof(M), C.sizeof(I)] + [getattr(M, f).offset for f in cfg_fields] + [getattr(I, f).offset for f in info_fields]
    assert vals[:-1] == want
    assert vals[:4] == [8, 40, 0, 4] and vals[4:10] == [0, 8, 16, 24, 32, 36]
    assert vals[-1] == 8   # additive: the ABI stays 8


def test_surfel_defaults():
    cfg = reg.default_closed_map_surfel_config()
    assert (cfg.min_points, cfg.reserved0) == (5, 0)
    assert reg.default_closed_map_surfel_config(min_points=3).min_points == 3
    with pytest.raises(KeyError):
        reg.default_closed_map_surfel_config(min_planarity=0.1)
    d = {k: p.default for k, p in inspect.signature(reg.HipRegistration.closed_map_read_surfels_box).parameters.items()}
    assert (d["lo"], d["hi"], d["min_count"], d["max_sigma"], d["min_planarity"]) == (None, None, 1, float("inf"), 0.05)


def test_surfel_symbols_are_exported():
    L = reg.load_library()
    for name in SURFEL_SYMBOLS:
        assert name in reg.EXPORTED_SYMBOLS
        getattr(L, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", reg.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SURFEL_SYMBOLS) <= exported
    for name in ("closed_map_surfel_configure", "closed_map_surfels", "closed_map_surfel_info", "closed_map_moments",
                 "closed_map_read_surfels", "closed_map_read_surfels_box"):
        assert callable(getattr(reg.HipRegistration, name))
    for name in ("write_surfel_pcd", "read_surfel_pcd", "write_closed_map_surfel_pcd"):
        assert callable(getattr(map_io, name))
