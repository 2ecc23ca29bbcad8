"""tloam_segment (the segmentation node on the device, tl_seg.hip) against the numpy restatement
(tests/segmentation_np.py): index lists equal in content and order, boxes bit for bit."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import segmentation_np as S  # noqa: E402
import make_seg_golden as MG  # noqa: E402
from tloam_amd import synth_hdl64 as G  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("ground", "object", "segmented", "label", "edge", "general")


@pytest.fixture(scope="module")
def H(hip_module):
    return hip_module.HipRegistration()


def fresh(reg):
    return reg.HipRegistration()


def assert_same(dev, ref, what=""):
    assert dev["status"] == ref["status"], what
    np.testing.assert_array_equal(dev["ring"], ref["ring"], err_msg=f"{what} ring")
    for k in KEYS:
        np.testing.assert_array_equal(dev[k], np.asarray(ref[k]), err_msg=f"{what} {k}")
    assert dev["boxes"].shape == np.asarray(ref["boxes"]).shape, what
    assert dev["boxes"].tobytes() == np.asarray(ref["boxes"], np.float64).tobytes(), f"{what} boxes"


@pytest.mark.parametrize("seed", MG.SEEDS)
def test_golden_scans(hip_module, seed):
    """~120 k returns each (with six NaN / Inf injections): the first frame of a context against the golden file.  The
    restatement's margin report for these scenes is empty (make_seg_golden asserts it)."""
    g = np.load(os.path.join(HERE, "golden", f"seg_{seed}.npz"))
    xyz = MG.golden_scan(seed)
    assert MG.digest(xyz) == str(g["digest"])
    dev = fresh(hip_module).segment(xyz)
    ref = {k: g[k] for k in KEYS + ("boxes",)}
    ref["ring"] = g["ring"].astype(np.int32)
    ref["status"] = 0
    assert_same(dev, ref, f"seed {seed}")
    # the reference's own DCVC loop against the components the device computes (declared deviation): shown, not hidden
    print(f"seed {seed}: literal DCVC partition differs from the components: {bool(g['literal_differs'])}")


def test_second_call_follows_min_polar_zero(hip_module):
    xyz = MG.golden_scan(1)
    R = fresh(hip_module)
    a = R.segment(xyz)
    b = R.segment(xyz)
    assert_same(a, S.segment(xyz, first_frame=True), "first call")
    ref = S.segment(xyz, first_frame=False)
    assert not ref["margins"]
    assert_same(b, ref, "second call")


def test_runs_and_contexts_give_the_same_bits(hip_module, H):
    xyz = MG.golden_scan(2)
    R1, R2 = fresh(hip_module), fresh(hip_module)
    a1, a2 = R1.segment(xyz), R1.segment(xyz)
    b1, b2 = R2.segment(xyz), R2.segment(xyz)
    for x, y in ((a1, b1), (a2, b2)):
        for k in ("ring",) + KEYS:
            np.testing.assert_array_equal(x[k], y[k])
        assert x["boxes"].tobytes() == y["boxes"].tobytes()


def test_non_finite_and_far_returns(hip_module):
    """an enclosing wall at 130 m (returns beyond sensorMaxRange: polarCor (0, 0, 0), one voxel) and 40 NaN / Inf"""
    W = G.make_street(5)
    xyz = G.scan(W, G.trajectory(1)[0], seed=5, far_wall=True, nan_inf=40)[0]
    ref = S.segment(xyz, first_frame=True)
    assert not ref["margins"], ref["margins"][:5]
    assert (ref["ring"] == -1).sum() >= 40
    assert_same(fresh(hip_module).segment(xyz), ref, "far / non-finite")


def test_empty_and_all_near_scans(hip_module):
    R = fresh(hip_module)
    e = R.segment(np.zeros((0, 3)))
    assert e["status"] == -2 and all(len(e[k]) == 0 for k in KEYS) and len(e["boxes"]) == 0
    rng = np.random.default_rng(3)
    near = rng.uniform(-5, 5, (5000, 3)).astype(np.float32).astype(np.float64)   # every norm below 9 m
    o = R.segment(near)
    assert o["status"] == -2
    assert (o["ring"] == -1).all()
    assert all(len(o[k]) == 0 for k in KEYS)


def test_vlp16_config_is_invalid(hip_module, H):
    xyz = MG.golden_scan(0)[:1000]
    with pytest.raises(hip_module.TloamHipError, match="TLOAM_E_INVALID"):
        H.segment(xyz, hip_module.default_seg_config(sensor_model=16))
    with pytest.raises(hip_module.TloamHipError, match="TLOAM_E_INVALID"):
        H.segment(xyz, hip_module.default_seg_config(quadrant=2))


def test_one_oversized_ring(hip_module):
    """ring 60 (+0.8 deg: walls and cars) fired with 40000 azimuth steps instead of 1900: a segmented ring of more than
    10 k points, sectors of some 2 k entries"""
    W = G.make_street(0)
    T = G.trajectory(1)[0]
    base, ring = G.scan(W, T, seed=8)
    big, _ = G.scan(W, T, seed=9, n_az=40000, rings=[60])
    xyz = np.concatenate([base[ring < 60], big, base[ring > 60]])
    ref = S.segment(xyz, first_frame=True)
    assert not ref["margins"], ref["margins"][:5]
    seg_ring = ref["ring"][ref["segmented"]]
    assert np.bincount(seg_ring, minlength=64).max() > 10000
    assert_same(fresh(hip_module).segment(xyz), ref, "oversized ring")


def test_replay_with_the_device_segmenter(hip_module):
    """six ray-cast frames along the generator's trajectory, replayed with segmenter="device": the poses follow the
    generator.  Measured on the MI355X: worst translation error 0.038 m over the six frames; the bound is four times that."""
    from tloam_amd import replay
    scans, poses = G.sequence(6, seed=3)
    R = fresh(hip_module)
    est, stats = replay.replay(R, scans, segmenter="device")
    assert stats["frames"] == 6
    T0inv = np.linalg.inv(poses[0])
    worst = 0.0
    for f in range(6):
        truth = T0inv @ poses[f]
        worst = max(worst, float(np.linalg.norm(est[f][:3, 3] - truth[:3, 3])))
    print("replay(segmenter='device'): worst translation error", worst, "m over", stats)
    assert worst < 0.15
