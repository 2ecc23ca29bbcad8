"""The robust mode of the pose graph without a GPU: the ctypes mirrors of tloam_graph_robust_config /
_info against the C header, the defaults, and the entry points in the built library."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from tloam_amd import registration as reg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROBUST_SYMBOLS = ("tloam_graph_robust_default_config", "tloam_graph_robust_configure", "tloam_graph_solve_robust",
                  "tloam_graph_read_loop_scales", "tloam_graph_get_robust_info")


def test_graph_robust_struct_layout_matches_the_c_header():
    cfg_fields = ("enabled", "max_outer", "noise_chi2", "mu_factor")
    info_fields = ("outer_iterations", "stop_reason", "gn_iterations", "cg_iterations", "rejected", "kept", "undecided",
                   "mu_first", "mu_last", "max_chi2_first")
    offs = ", ".join([f"offsetof(tloam_graph_robust_config, {f})" for f in cfg_fields] +
                     [f"offsetof(tloam_graph_robust_info, {f})" for f in info_fields])
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "tloam_hip.h"
int main(void) {
  size_t v[] = {sizeof(tloam_graph_robust_config), sizeof(tloam_graph_robust_info), %s};
  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%%zu ", v[i]);
  printf("%%d %%d %%d %%d %%d\n", TLOAM_GRAPH_ROBUST_STOP_OFF, TLOAM_GRAPH_ROBUST_STOP_ALL_INLIERS, TLOAM_GRAPH_ROBUST_STOP_BINARY,
         TLOAM_GRAPH_ROBUST_STOP_OUTER_LIMIT, TLOAM_ABI_VERSION);
  return 0;
}''' % offs
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c"); exe = os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = list(map(int, subprocess.check_output([exe]).split()))
    M, I = reg.GraphRobustConfig, reg.GraphRobustInfo
    assert [n for n, _ in M._fields_] == list(cfg_fields) and [n for n, _ in I._fields_] == list(info_fields)
    want = [C.sizeof(M), C.sizeof(I)] + [getattr(M, f).offset for f in cfg_fields] + [getattr(I, f).offset for f in info_fields]
    assert vals[:-5] == want
    assert vals[:6] == [24, 72, 0, 4, 8, 16]
    assert vals[-5:] == [0, 1, 2, 3, 8]   # the stop reasons; additive: the ABI stays 8
    assert reg.GRAPH_ROBUST_STOP == {0: "off", 1: "all_inliers", 2: "binary", 3: "outer_limit"}


def test_the_abi_version_is_still_8_and_the_graph_structs_are_unchanged():
    assert reg.load_library().tloam_abi_version() == 8
    assert C.sizeof(reg.GraphConfig) == 56 and C.sizeof(reg.GraphInfo) == 80 and C.sizeof(reg.GraphEdge) == 192


def test_graph_robust_defaults():
    cfg = reg.default_graph_robust_config()
    assert (cfg.enabled, cfg.max_outer, cfg.noise_chi2, cfg.mu_factor) == (0, 100, 36.0, 1.4)
    over = reg.default_graph_robust_config(enabled=1, noise_chi2=16.81, mu_factor=2.0, max_outer=7)
    assert (over.enabled, over.max_outer, over.noise_chi2, over.mu_factor) == (1, 7, 16.81, 2.0)
    with pytest.raises(KeyError):
        reg.default_graph_robust_config(chi2=9.0)


def test_graph_robust_symbols_are_exported():
    L = reg.load_library()
    for name in ROBUST_SYMBOLS:
        assert name in reg.EXPORTED_SYMBOLS
        getattr(L, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", reg.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ROBUST_SYMBOLS) <= exported
    for name in ("graph_robust_configure", "graph_solve_robust", "graph_read_loop_scales", "graph_robust_info"):
        assert callable(getattr(reg.HipRegistration, name))
