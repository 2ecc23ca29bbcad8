"""The localisation in the closed map without a GPU: the ctypes mirrors of
tloam_closed_map_localise_config / _info / _record against the C header, the defaults, the entry points in the built library and
the Python methods."""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

import pytest

from tloam_amd import registration as reg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOCALISE_SYMBOLS = ("tloam_closed_map_localise_default_config", "tloam_closed_map_localise_configure", "tloam_closed_map_localise",
                    "tloam_closed_map_localise_log", "tloam_closed_map_linearise")
CFG_FIELDS = ("max_residual0", "shrink", "min_residual", "max_sigma", "min_planarity", "step_tol_t", "step_tol_r", "min_pivot_ratio",
              "max_iterations", "min_matches")
INFO_FIELDS = ("status", "iterations", "matched", "used", "rms", "launches", "prepared")
REC_FIELDS = ("pose_colmajor", "tau", "cost", "d", "matched", "used")


def test_localise_struct_layout_matches_the_c_header():
    structs = (("tloam_closed_map_localise_config", CFG_FIELDS, reg.ClosedMapLocaliseConfig),
               ("tloam_closed_map_localise_info", INFO_FIELDS, reg.ClosedMapLocaliseInfo),
               ("tloam_closed_map_localise_record", REC_FIELDS, reg.ClosedMapLocaliseRecord))
    exprs = [f"sizeof({name})" for name, _, _ in structs] + [f"offsetof({name}, {f})" for name, fields, _ in structs for f in fields]
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "tloam_hip.h"
int main(void) {
  size_t v[] = {%s};
  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%%zu ", v[i]);
  printf("%%d %%d %%d %%d\n", TLOAM_LOCALISE_CONVERGED, TLOAM_LOCALISE_MAX_ITERATIONS, TLOAM_LOCALISE_DEGENERATE, TLOAM_ABI_VERSION);
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
    assert vals[:-4] == want
    assert vals[:3] == [72, 40, 208]
    assert vals[-4:-1] == [reg.LOCALISE_CONVERGED, reg.LOCALISE_MAX_ITERATIONS, reg.LOCALISE_DEGENERATE] == [0, 1, 2]
    assert vals[-1] == 8   # additive: the ABI stays 8


def test_localise_defaults():
    cfg = reg.default_closed_map_localise_config()
    assert [getattr(cfg, f) for f in CFG_FIELDS] == [1.0, 0.7, 0.1, float("inf"), 0.05, 1e-6, 1e-7, 1e-9, 20, 50]
    assert reg.default_closed_map_localise_config(max_iterations=5, shrink=0.5).max_iterations == 5
    with pytest.raises(KeyError):
        reg.default_closed_map_localise_config(min_points=3)


def test_localise_symbols_are_exported():
    L = reg.load_library()
    for name in LOCALISE_SYMBOLS:
        assert name in reg.EXPORTED_SYMBOLS
        getattr(L, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", reg.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(LOCALISE_SYMBOLS) <= exported
    sig = {name: list(inspect.signature(getattr(reg.HipRegistration, name)).parameters) for name in
           ("closed_map_localise_configure", "closed_map_localise", "closed_map_localise_log", "closed_map_linearise")}
    assert sig == {"closed_map_localise_configure": ["self", "cfg", "over"], "closed_map_localise": ["self", "points", "prior"],
                   "closed_map_localise_log": ["self"], "closed_map_linearise": ["self", "points", "pose", "tau"]}
