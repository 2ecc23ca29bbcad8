"""The deskew of the odometry frame without a GPU: the ctypes mirrors of tloam_deskew_config / _info
against the C header, the defaults, the new entry points in the built library, properties of the numpy restatement
(tests/deskew_np.py) the device is checked against, and the swept-scan generator (tloam_amd/synth_sweep.py)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import abi_kit  # noqa: E402
import deskew_np as D  # noqa: E402
from tloam_amd import registration as reg  # noqa: E402
from tloam_amd import synth_hdl64 as G  # noqa: E402
from tloam_amd import synth_sweep as SW  # noqa: E402
from tloam_amd.synth import se3_exp_np  # noqa: E402

DESKEW_SYMBOLS = ("tloam_deskew_default_config", "tloam_deskew_configure", "tloam_deskew_get_info",
                  "tloam_odometry_frame_timed", "tloam_deskew_scan")
XI = np.array([0.8, 0.05, -0.02, 0.004, -0.006, 0.03])   # a frame's motion: 0.8 m and 0.03 rad of yaw


def test_deskew_struct_layout_matches_the_c_header():
    """(every field of both mirrors against the header: tests/test_abi_header.py)"""
    assert abi_kit.sizes("tloam_deskew_config", "tloam_deskew_info") == [32, 200]
    assert abi_kit.offsets("tloam_deskew_config") == [0, 4, 8, 12, 16, 24]


def test_deskew_defaults():
    cfg = reg.default_deskew_config()
    assert (cfg.enabled, cfg.time_source, cfg.direction, cfg.start_azimuth, cfg.ref_fraction) == (0, 0, 1, 0.0, 0.0)
    over = reg.default_deskew_config(enabled=1, time_source=1, direction=-1, start_azimuth=0.5, ref_fraction=0.25)
    assert (over.enabled, over.time_source, over.direction, over.start_azimuth, over.ref_fraction) == (1, 1, -1, 0.5, 0.25)
    with pytest.raises(KeyError):
        reg.default_deskew_config(period=0.1)


def test_deskew_symbols_are_exported():
    abi_kit.assert_exported(DESKEW_SYMBOLS)


def scan_like(rng, n):
    """returns around a sensor: ranges 2-80 m, every azimuth, a few rings' elevations"""
    az = rng.uniform(-np.pi, np.pi, n)
    el = rng.uniform(-0.4, 0.05, n)
    r = rng.uniform(2.0, 80.0, n)
    return np.column_stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)])


def test_identity_motion_or_zero_time_gives_the_input_bits():
    rng = np.random.default_rng(1)
    p = scan_like(rng, 5000)
    p[7] = [np.nan, 1.0, 2.0]
    p[8] = [3.0, np.inf, 1.0]
    assert D.deskew(p, np.eye(4)).tobytes() == p.tobytes()
    assert D.deskew(p, np.eye(4), times=rng.uniform(-0.05, 0.05, len(p))).tobytes() == p.tobytes()
    M = se3_exp_np(XI)
    out = D.deskew(p, M, times=np.zeros(len(p)))
    assert out.tobytes() == p.tobytes()
    # non-finite returns are copied whatever their time; the others move
    t = rng.uniform(0.01, 0.05, len(p))
    out = D.deskew(p, M, times=t)
    assert out[7:9].tobytes() == p[7:9].tobytes()
    assert np.all(np.abs(np.delete(out, [7, 8], axis=0) - np.delete(p, [7, 8], axis=0)).max(axis=1) > 0)
    # a return on the +x axis has azimuth 0: s == 0 in azimuth mode with start 0 and ref 0
    q = np.array([[12.0, 0.0, -1.0], [0.0, 12.0, -1.0]])
    out = D.deskew(q, M)
    assert out[0].tobytes() == q[0].tobytes() and not np.array_equal(out[1], q[1])


@pytest.mark.parametrize("seed", (2, 3))
def test_timed_deskew_undoes_the_distortion(seed):
    rng = np.random.default_rng(seed)
    M = se3_exp_np(XI * rng.uniform(0.5, 1.5))
    truth = scan_like(rng, 2000)
    t = rng.uniform(-0.1, 0.1, len(truth))
    raw = D.distort(truth, M, t / 0.1)
    out = D.deskew(raw, M, times=t, scan_period=0.1)
    assert np.abs(out - truth).max() < 1e-12
    assert np.abs(raw - truth).max() > 0.1


def test_bad_times_are_refused():
    p = scan_like(np.random.default_rng(4), 10)
    for bad in (np.nan, np.inf, 0.2000001, -0.25):
        t = np.zeros(10)
        t[3] = bad
        with pytest.raises(ValueError):
            D.sweep_s(p, times=t, scan_period=0.1)
    t = np.zeros(10); t[3] = 0.2
    assert D.sweep_s(p, times=t, scan_period=0.1)[3] == 2.0


@pytest.mark.parametrize("direction", (1, -1))
@pytest.mark.parametrize("start", (0.0, 1.0, -2.5))
def test_azimuth_wraps_at_the_start(direction, start):
    eps = 1e-6
    az = np.array([start + eps, start - eps, start + np.pi / 2, start - np.pi / 2, start + np.pi])
    p = np.column_stack([10 * np.cos(az), 10 * np.sin(az), np.zeros(len(az))])
    s = D.sweep_s(p, direction=direction, start_azimuth=start)
    assert np.all((s >= 0.0) & (s < 1.0))
    just_after, just_before = (s[0], s[1]) if direction == 1 else (s[1], s[0])
    assert just_after < 1e-6 and just_before > 1.0 - 1e-6
    quarter, three_quarters = (s[2], s[3]) if direction == 1 else (s[3], s[2])
    assert abs(quarter - 0.25) < 1e-12 and abs(three_quarters - 0.75) < 1e-12
    assert abs(s[4] - 0.5) < 1e-12
    s_ref = D.sweep_s(p, direction=direction, start_azimuth=start, ref_fraction=0.3)
    assert np.abs(s_ref - (s - 0.3)).max() < 1e-15


@pytest.mark.parametrize("a,b", ((0.0, 0.5), (0.25, 1.0), (0.9, 0.1)))
def test_changing_the_reference_fraction_is_a_rigid_motion(a, b):
    rng = np.random.default_rng(5)
    p = scan_like(rng, 3000)
    M = se3_exp_np(XI)
    out_a = D.deskew(p, M, ref_fraction=a)
    out_b = D.deskew(p, M, ref_fraction=b)
    T = se3_exp_np((a - b) * XI)
    assert np.abs(out_a @ T[:3, :3].T + T[:3, 3] - out_b).max() < 1e-11


def test_generator_with_zero_twist_is_the_scan_bit_for_bit():
    W = G.make_street(3)
    pose = G.trajectory(5, seed=3)[4]
    for kw in (dict(seed=3004), dict(seed=11, nan_inf=6, far_wall=True, rings=np.arange(0, 64, 4), n_az=600)):
        ref_p, ref_ring = G.scan(W, pose, **kw)
        p, ring, t, hits = SW.sweep_scan(W, pose, np.zeros(6), **kw)
        assert p.tobytes() == ref_p.tobytes()
        assert ring.tobytes() == ref_ring.tobytes()
        assert len(t) == len(p) == len(hits)
    # zero twist: every return's world hit is the scan's point by the pose (before the float32 rounding)
    p, _, _, hits = SW.sweep_scan(W, pose, np.zeros(6), noise=0.0)
    assert np.abs(p @ pose[:3, :3].T + pose[:3, 3] - hits).max() < 1e-4


@pytest.mark.parametrize("ref", (0.0, 0.5))
def test_restated_deskew_of_a_swept_scan_lies_on_the_world_hits(ref):
    W = G.make_street(1)
    xi = np.array([0.8, 0.0, 0.0, 0.0, 0.0, 0.03])
    pose = SW.trajectory(3, xi)[2]
    p, ring, t, hits = SW.sweep_scan(W, pose, xi, ref=ref, noise=0.0, seed=7)
    assert np.all(np.diff(ring) >= 0)   # ring by ring
    assert np.abs(t).max() <= 0.1
    M = se3_exp_np(xi)
    to_world = lambda q: q @ pose[:3, :3].T + pose[:3, 3]  # noqa: E731
    for out in (D.deskew(p, M, ref_fraction=ref), D.deskew(p, M, times=t)):
        assert np.abs(to_world(out) - hits).max() < 1e-4
    assert np.abs(to_world(p) - hits).max() > 0.1   # without the correction
