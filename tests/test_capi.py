"""CPU: the C-ABI shared library loads, exports every symbol include/tloam_hip.h declares, agrees on
struct layout, and its host-only entry points (SE(3) helpers, shard ranges) behave.  No GPU compute is
attempted here; on a machine without a gfx950 device tloam_create must FAIL loudly (TLOAM_E_HIP) --
there is no CPU fallback."""
import ctypes as C

import numpy as np
import pytest

import abi_kit
from oracle import binding as ob
from tloam_amd import registration as reg


def test_library_exports_every_declared_symbol():
    L = reg.load_library()
    names = abi_kit.declared_functions()
    assert len(names) >= 30
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/tloam_hip.h but not exported"
    assert set(reg.EXPORTED_SYMBOLS) == set(names)
    assert [L.tloam_abi_version()] == abi_kit.constants("TLOAM_ABI_VERSION") == [8]


def test_struct_layout_matches_the_c_header():
    """the oracle's TlsConfig and Stats (another library's binding) have the layout of the header's; the product's own mirrors,
    every field of them: tests/test_abi_header.py"""
    for name, S in (("tloam_tls_config", ob.TlsConfig), ("tloam_stats", ob.Stats), ("tloam_tls_config", reg.TlsConfig),
                    ("tloam_stats", reg.Stats), ("tloam_ctx_info", reg.CtxInfo)):
        fields = abi_kit.header_structs()[name]
        assert [f for f, _ in S._fields_] == fields
        assert abi_kit.sizes(name) == [C.sizeof(S)] and abi_kit.offsets(name) == [getattr(S, f).offset for f in fields], name


def test_default_config_is_the_shipped_yaml():
    cfg = reg.default_config()
    expect = dict(k_corr=10, factor_num=4, edge_dist_thres=1.0, edge_dir_thres=0.85, edge_maxnum=1200,
                  sphere_dist_thres=0.5, sphere_maxnum=200, planar_dist_thres=0.5, planar_maxnum=2500,
                  ground_dist_thres=0.5, ground_maxnum=2000, max_iterations=4, cost_threshold=5e-9,
                  gnc_factor=11.8, noise_bound=0.01, fitness_thres=0.02)   # lidar_odometry.yaml:23-39
    for k, v in expect.items():
        assert getattr(cfg, k) == v, k
        assert getattr(ob.make_config(), k) == v, k


def test_status_strings_and_factory():
    L = reg.load_library()
    assert L.tloam_status_string(0) == b"ok"
    assert b"rigid" in L.tloam_status_string(-3)
    with pytest.raises(ValueError, match="Other methods are not yet supported"):   # front_end.cpp:163
        reg.make_registration("NDT")


def test_create_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: covered by the -m gpu tests")
    h = C.c_void_p()
    cfg = reg.default_config()
    assert reg.load_library().tloam_create(C.byref(cfg), 0, C.byref(h)) == -4       # TLOAM_E_HIP
    with pytest.raises(reg.TloamHipError, match="no CPU fallback"):
        reg.HipRegistration()


def test_host_se3_helpers_match_the_oracle():
    rng = np.random.default_rng(3)
    for _ in range(20):
        x = np.concatenate([rng.normal(0, 2, 3), rng.normal(0, 0.8, 3)])
        d = np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 0.02, 3)])
        np.testing.assert_allclose(reg.se3_exp(x), ob.se3_exp(x), atol=1e-14)
        np.testing.assert_allclose(reg.se3_log(reg.se3_exp(x)), x, atol=1e-12)
        np.testing.assert_allclose(reg.se3_plus(x, d), ob.plus(x, d), atol=1e-13)
    bad = reg.se3_exp(x); bad[:3, :3] *= 1.01
    with pytest.raises(reg.TloamHipError, match="BAD_POSE"):
        reg.se3_log(bad)
    for v in (np.nan, np.inf, -np.inf):   # a non-finite translation passes Sophus' checks; here it is a bad pose too
        bad = reg.se3_exp(x); bad[1, 3] = v
        with pytest.raises(reg.TloamHipError, match="BAD_POSE"):
            reg.se3_log(bad)


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 1000, 1_000_003])
@pytest.mark.parametrize("nranks", [1, 2, 3, 8])
def test_shard_ranges_tile_the_index_space(n, nranks):
    prev = 0
    sizes = []
    for r in range(nranks):
        lo, hi = reg.shard_range(n, r, nranks)
        assert lo == prev and hi >= lo
        prev = hi
        sizes.append(hi - lo)
    assert prev == n
    assert max(sizes) - min(sizes) <= 1                 # contiguous, balanced blocks


def test_graft_entry_build_runs():
    """The driver's build check: __graft_entry__.build() compiles every extension and validates the library
    against the header (it once asserted a stale ABI number)."""
    import __graft_entry__ as g
    g.build()


def test_sizes_beyond_the_32_bit_slot_space_are_refused_at_the_header_level():
    """include/tloam_hip.h: at most 2^28 points per cloud / set / batch (TLOAM_E_INVALID).  Without a device the entry points
    answer TLOAM_E_HIP / refuse the context first; what can be checked here is that the bound is stated where a host reads it."""
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tloam_hip.h")).read()
    assert "2^28 points" in hdr and "TLOAM_E_INVALID at the entry point" in hdr
