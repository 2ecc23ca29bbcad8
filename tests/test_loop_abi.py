"""Loop verification without a GPU: the ctypes mirrors of tloam_loop_config / _info / _constraint against
the C header, the defaults, the new entry points in the built library, null arguments, and the numpy restatement's window and
T_rel.  Everything that needs a context needs a device: tests/test_gpu_loop.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from tloam_amd import registration as reg

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import abi_kit  # noqa: E402
import loop_np as LN  # noqa: E402

LOOP_SYMBOLS = ("tloam_loop_default_config", "tloam_loop_configure", "tloam_loop_get_info", "tloam_place_set_keyframe_clouds",
                "tloam_place_read_keyframe_clouds", "tloam_loop_verify_pending", "tloam_loop_verify_pair",
                "tloam_loop_read_constraints")


def test_loop_struct_layouts_match_the_c_header():
    """(every field of the three mirrors against the header: tests/test_abi_header.py)"""
    assert abi_kit.sizes("tloam_loop_config", "tloam_loop_info", "tloam_loop_constraint") == [152, 32, 632]
    assert C.sizeof(reg.LoopConfig) == 152 and C.sizeof(reg.LoopInfo) == 32 and C.sizeof(reg.LoopConstraint) == 632
    assert reg.LoopConfig.inlier_dist.offset == 16 and reg.LoopConfig.coarse.offset == 48   # explicit padding


def test_loop_defaults():
    c = reg.default_loop_config()
    assert (c.enabled, c.window, c.init_mode, c.reserved0, c.reserve_points) == (0, 2, 0, 0, 0)
    assert c.inlier_dist > 0 and 0 < c.min_overlap <= 1 and c.max_rmse > 0
    t = reg.default_config()
    for k in ("edge_dist_thres", "sphere_dist_thres", "planar_dist_thres", "ground_dist_thres"):
        assert getattr(c.coarse, k) > getattr(t, k), k
    for k, _ in reg.TlsConfig._fields_:
        if not k.endswith("dist_thres") and k != "max_iterations":
            assert getattr(c.coarse, k) == getattr(t, k), k
    o = reg.default_loop_config(enabled=1, window=3, min_overlap=0.4, coarse__max_iterations=6)
    assert (o.enabled, o.window, o.min_overlap, o.coarse.max_iterations) == (1, 3, 0.4, 6)
    with pytest.raises(KeyError):
        reg.default_loop_config(radius=1.0)
    with pytest.raises(KeyError):
        reg.default_loop_config(coarse__radius=1.0)


def test_loop_symbols_are_exported():
    abi_kit.assert_exported(LOOP_SYMBOLS)


def test_null_arguments_are_refused():
    L = reg.load_library()
    n, cfg, info, con = C.c_size_t(0), reg.default_loop_config(), reg.LoopInfo(), reg.LoopConstraint()
    k = C.c_int64(0)
    assert L.tloam_loop_configure(None, C.byref(cfg)) == -1
    assert L.tloam_loop_get_info(None, C.byref(info)) == -1
    assert L.tloam_place_set_keyframe_clouds(None, 0, None, None, None, None) == -1
    assert L.tloam_place_read_keyframe_clouds(None, 0, 0, 0, 0, C.byref(n), None) == -1
    assert L.tloam_loop_verify_pending(None, C.byref(k)) == -1
    assert L.tloam_loop_verify_pair(None, 1, 0, None, C.byref(con)) == -1
    assert L.tloam_loop_read_constraints(None, 0, 0, C.byref(con)) == -1
    L.tloam_loop_default_config(None)   # (no crash)


def test_window_rule():
    assert LN.window(10, 4, 2) == [2, 3, 4, 5, 6]
    assert LN.window(10, 1, 2) == [0, 1, 2, 3]
    assert LN.window(5, 4, 2) == [2, 3, 4]
    assert LN.window(6, 4, 3) == [1, 2, 3, 4, 5]
    assert LN.window(3, 0, 0) == [0]


def test_t_rel_is_the_relative_pose():
    r = np.random.default_rng(5)
    def pose():
        a = r.uniform(-np.pi, np.pi)
        T = np.eye(4)
        T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        T[:3, 3] = r.uniform(-20, 20, 3)
        return T
    A, B = pose(), pose()
    np.testing.assert_allclose(LN.t_rel(A, B), np.linalg.inv(A) @ B, atol=1e-12)
    p = r.uniform(-5, 5, (7, 3))
    np.testing.assert_allclose(LN.move(B, p), (B[:3, :3] @ p.T).T + B[:3, 3], atol=1e-12)
    ov, rmse, inl, pts = LN.score([p, p[:0], p[:3], p[:0]], [p, p[:0], p[:3] + 0.01, p[:0]], np.eye(4), 0.1)
    assert (inl, pts) == (10, 10) and ov == 1.0 and abs(rmse - np.sqrt(3 * 3e-4 / 10)) < 1e-12
