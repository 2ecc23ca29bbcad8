"""The carve of the closed map without a GPU: the ctypes mirrors of tloam_closed_map_carve_config /
_info against the C header, the defaults, the entry points in the built library and the Python methods."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from tloam_amd import map_io
from tloam_amd import registration as reg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARVE_SYMBOLS = ("tloam_closed_map_carve_default_config", "tloam_closed_map_carve_configure", "tloam_closed_map_get_carve_info",
                 "tloam_closed_map_carve", "tloam_closed_map_read_misses", "tloam_closed_map_read_carved")


def test_carve_struct_layout_matches_the_c_header():
    cfg_fields = ("max_range", "end_margin", "radius", "ray_mask", "reserved0")
    info_fields = ("n_keyframes", "n_rays", "skipped_rays", "steps", "tested", "misses", "voxels_missed", "launches", "reserved0")
    offs = ", ".join([f"offsetof(tloam_closed_map_carve_config, {f})" for f in cfg_fields] +
                     [f"offsetof(tloam_closed_map_carve_info, {f})" for f in info_fields])
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "tloam_hip.h"
int main(void) {
  size_t v[] = {sizeof(tloam_closed_map_carve_config), sizeof(tloam_closed_map_carve_info), %s};
  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%%zu ", v[i]);
  printf("%%d\n", TLOAM_ABI_VERSION);
  return 0;
}''' % offs
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c"); exe = os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = list(map(int, subprocess.check_output([exe]).split()))
    M, I = reg.ClosedMapCarveConfig, reg.ClosedMapCarveInfo
    assert [n for n, _ in M._fields_] == list(cfg_fields) and [n for n, _ in I._fields_] == list(info_fields)
    want = [C.sizeof(M), C.sizeof(I)] + [getattr(M, f).offset for f in cfg_fields] + [getattr(I, f).offset for f in info_fields]
    assert vals[:-1] == want
    assert vals[:7] == [32, 64, 0, 8, 16, 24, 28]
    assert vals[-1] == 8   # additive: the ABI stays 8


def test_carve_defaults():
    cfg = reg.default_closed_map_carve_config()
    assert (cfg.max_range, cfg.end_margin, cfg.radius, cfg.ray_mask, cfg.reserved0) == (60.0, 1.0, 0.25, 0, 0)
    over = reg.default_closed_map_carve_config(max_range=20.0, end_margin=0.0, radius=float("inf"), ray_mask=0x0F)
    assert (over.max_range, over.end_margin, over.radius, over.ray_mask) == (20.0, 0.0, float("inf"), 0x0F)
    with pytest.raises(KeyError):
        reg.default_closed_map_carve_config(min_miss=3)
    import inspect
    d = {k: p.default for k, p in inspect.signature(reg.HipRegistration.closed_map_read_carved).parameters.items()}
    assert (d["lo"], d["hi"], d["min_count"], d["min_miss"], d["miss_ratio"]) == (None, None, 1, 3, 1.0)


def test_carve_symbols_are_exported():
    L = reg.load_library()
    for name in CARVE_SYMBOLS:
        assert name in reg.EXPORTED_SYMBOLS
        getattr(L, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", reg.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(CARVE_SYMBOLS) <= exported
    for name in ("closed_map_carve_configure", "closed_map_carve", "closed_map_carve_info", "closed_map_misses",
                 "closed_map_read_carved"):
        assert callable(getattr(reg.HipRegistration, name))
    assert callable(map_io.write_carved_closed_map_pcd)
