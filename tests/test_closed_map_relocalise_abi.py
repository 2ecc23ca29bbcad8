"""The batched localiser and the relocalisation without a GPU: the ctypes mirrors of
tloam_closed_map_relocalise_config / _info / _hypothesis against the C header, the defaults, the entry points in the built
library and the Python methods."""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

import pytest

from tloam_amd import registration as reg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tloam_closed_map_localise_batch", "tloam_closed_map_localise_batch_log", "tloam_closed_map_relocalise_default_config",
           "tloam_closed_map_relocalise_configure", "tloam_closed_map_relocalise", "tloam_closed_map_relocalise_hypotheses")
CFG_FIELDS = ("num_candidates", "reserved0", "max_dist", "min_used_ratio", "max_rms")
INFO_FIELDS = ("status", "n_hypotheses", "best", "launches", "keyframe", "shift", "reserved0", "dist", "yaw", "localise")
HYP_FIELDS = ("keyframe", "shift", "skipped", "dist", "yaw", "prior_colmajor", "pose_colmajor", "localise")


def test_relocalise_struct_layout_matches_the_c_header():
    structs = (("tloam_closed_map_relocalise_config", CFG_FIELDS, reg.ClosedMapRelocaliseConfig),
               ("tloam_closed_map_relocalise_info", INFO_FIELDS, reg.ClosedMapRelocaliseInfo),
               ("tloam_closed_map_relocalise_hypothesis", HYP_FIELDS, reg.ClosedMapRelocaliseHypothesis))
    exprs = [f"sizeof({name})" for name, _, _ in structs] + [f"offsetof({name}, {f})" for name, fields, _ in structs for f in fields]
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "tloam_hip.h"
int main(void) {
  size_t v[] = {%s};
  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%%zu ", v[i]);
  printf("%%d %%d %%d\n", TLOAM_RELOCALISE_FOUND, TLOAM_RELOCALISE_NOT_FOUND, TLOAM_ABI_VERSION);
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
    assert vals[:-3] == want
    assert vals[:3] == [32, 88, 328]
    assert vals[-3:-1] == [reg.RELOCALISE_FOUND, reg.RELOCALISE_NOT_FOUND] == [0, 1]
    assert vals[-1] == 8   # additive: the ABI stays 8


def test_relocalise_defaults():
    cfg = reg.default_closed_map_relocalise_config()
    assert [getattr(cfg, f) for f in CFG_FIELDS] == [8, 0, float("inf"), 0.5, float("inf")]
    assert reg.default_closed_map_relocalise_config(num_candidates=3, max_dist=0.4).num_candidates == 3
    with pytest.raises(KeyError):
        reg.default_closed_map_relocalise_config(max_iterations=3)
    # default_config fills every field, the reserved one included
    L = reg.load_library()
    raw = reg.ClosedMapRelocaliseConfig()
    C.memset(C.byref(raw), 0xAB, C.sizeof(raw))
    L.tloam_closed_map_relocalise_default_config(C.byref(raw))
    assert bytes(raw) == bytes(cfg)
    assert reg.LOCALISE_MAX_BATCH == 32


def test_relocalise_symbols_are_exported():
    L = reg.load_library()
    for name in SYMBOLS:
        assert name in reg.EXPORTED_SYMBOLS
        getattr(L, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", reg.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= exported
    names = ("closed_map_localise_batch", "closed_map_localise_batch_log", "closed_map_relocalise_configure",
             "closed_map_relocalise", "closed_map_relocalise_hypotheses")
    sig = {name: list(inspect.signature(getattr(reg.HipRegistration, name)).parameters) for name in names}
    assert sig == {"closed_map_localise_batch": ["self", "points", "priors"], "closed_map_localise_batch_log": ["self", "h"],
                   "closed_map_relocalise_configure": ["self", "cfg", "over"], "closed_map_relocalise": ["self", "points"],
                   "closed_map_relocalise_hypotheses": ["self"]}
