"""tloam_segment on the named small scenes of tests/seg_scenes.py: the quirk branches of tl_seg.hip
reached on purpose, every non-default SegConfig field, small inputs, many clusters, reused buffers.  Everything is compared
with the numpy restatement by test_gpu_segmentation.assert_same: status, ring, the six index lists in content and order, the
boxes bit for bit.  tests/test_seg_scenes.py shows on the CPU that each scene reaches its branch with an empty margin report."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import segmentation_np as S  # noqa: E402
import seg_scenes as SC  # noqa: E402
import make_seg_golden as MG  # noqa: E402
from test_gpu_segmentation import KEYS, assert_same, fresh  # noqa: E402

pytestmark = pytest.mark.gpu

NO_SCAN = np.zeros((0, 3))


def later_frame(R):
    """a call on an empty scan publishes nothing and still counts: the context's next frame is not its first"""
    assert R.segment(NO_SCAN)["status"] == S.STATUS_TOO_FEW


def same_bits(a, b, what):
    assert a["status"] == b["status"], what
    for k in ("ring",) + KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what} {k}")
    assert a["boxes"].tobytes() == b["boxes"].tobytes(), f"{what} boxes"


def run(reg, R, name, over=None):
    sc = SC.scene(name)
    return R.segment(sc.xyz, SC.seg_config(reg, SC.cfg_of(sc.over if over is None else over)))


@pytest.mark.parametrize("name", SC.NAMES)
def test_scene(hip_module, name):
    sc = SC.scene(name)
    ref = SC.reference(name)
    assert not ref["margins"] and ref["status"] == sc.status
    R = fresh(hip_module)
    if not sc.first_frame:
        later_frame(R)
    assert_same(run(hip_module, R, name), ref, name)


@pytest.mark.parametrize("name", SC.DETERMINISM_SCENES)
def test_long_chains_and_many_clusters_give_the_same_bits(hip_module, name):
    """three runs in one context and two in another: the first frames agree, the later frames agree (the unions race for
    their links, the roots and every list must not show it)"""
    A, B = fresh(hip_module), fresh(hip_module)
    a1, a2, a3 = (run(hip_module, A, name) for _ in range(3))
    b1, b2 = (run(hip_module, B, name) for _ in range(2))
    same_bits(a1, b1, f"{name}: first frames of two contexts")
    same_bits(a2, a3, f"{name}: second and third frame of one context")
    same_bits(a2, b2, f"{name}: second frames of two contexts")
    assert_same(a1, SC.reference(name), f"{name} first frame")
    assert_same(a3, SC.reference(name, False), f"{name} third frame")


@pytest.mark.parametrize("case", ["increment_runs_out", "above_the_cap"])
def test_refused_polar_bounds(hip_module, case):
    """an increment startR - step deltaR that reaches 0 before maxPolar (the reference's loop would not end), and a table of
    more than kSegMaxBounds entries (a declared limit): TLOAM_E_INVALID.  The refused frame counts: the next is a later frame"""
    over, ref_status, dev_status = SC.BOUNDS_CASES[case]
    assert dev_status == S.STATUS_INVALID and SC.bounds_reference(case)["status"] == ref_status
    assert (SC.bound_count(case) is None) if case == "increment_runs_out" else SC.bound_count(case) > SC.MAX_BOUNDS
    R = fresh(hip_module)
    with pytest.raises(hip_module.TloamHipError, match="TLOAM_E_INVALID"):
        run(hip_module, R, SC.BOUNDS_SCENE, over)
    ref = SC.reference(SC.BOUNDS_SCENE, False)
    assert not ref["margins"]
    assert_same(run(hip_module, R, SC.BOUNDS_SCENE), ref, f"after {case}")


def test_no_object_point_comes_before_the_polar_bounds(hip_module):
    """objectSegmentation returns on an empty object_scan before convertToPolar (:1088-1092): an increment that would run out
    is never looked at, the node publishes nothing -- status -2 with ring, ground and object, not TLOAM_E_INVALID"""
    sc = SC.scene(SC.NO_OBJECT_SCENE)
    over = dict(sc.over, deltaR=SC.BOUNDS_CASES["increment_runs_out"][0]["deltaR"])
    ref = S.segment(sc.xyz, SC.cfg_of(over), True)
    assert ref["status"] == S.STATUS_TOO_FEW and len(ref["object"]) == 0 and not ref["margins"]
    assert_same(run(hip_module, fresh(hip_module), SC.NO_OBJECT_SCENE, over), ref, "no object point")


def test_large_polar_bounds_table(hip_module):
    over = SC.BOUNDS_CASES["large_table"][0]
    assert 2000 <= SC.bound_count("large_table") <= SC.MAX_BOUNDS - 1
    ref = SC.bounds_reference("large_table")
    assert not ref["margins"] and ref["status"] == S.STATUS_OK
    assert_same(run(hip_module, fresh(hip_module), SC.BOUNDS_SCENE, over), ref, "large table")


@pytest.fixture(scope="module")
def golden_later_frame():
    ref = S.segment(MG.golden_scan(0), first_frame=False)
    assert ref["status"] == 0 and not ref["margins"]
    return ref


def test_small_scans_after_a_large_one_reuse_its_buffers(hip_module, golden_later_frame):
    """golden scan 0 (120 k returns), three small scenes, golden scan 0 again, in one context: the small frames run in
    buffers (marks, curvature, sorted entries, general entries, hash table) the large one left full"""
    g = np.load(os.path.join(HERE, "golden", "seg_0.npz"))
    xyz = MG.golden_scan(0)
    assert MG.digest(xyz) == str(g["digest"])
    first = {k: g[k] for k in KEYS + ("boxes",)}
    first.update(ring=g["ring"].astype(np.int32), status=0)
    R = fresh(hip_module)
    assert_same(R.segment(xyz), first, "golden scan 0, first frame")
    for name in SC.REUSE_SCENES:
        ref = SC.reference(name, False)
        assert not ref["margins"]
        assert_same(run(hip_module, R, name), ref, f"{name} after the large scan")
    last = R.segment(xyz)
    for k in ("ring", "ground", "object"):      # what minPolar does not touch is the golden file's
        np.testing.assert_array_equal(last[k], first[k], err_msg=k)
    assert_same(last, golden_later_frame, "golden scan 0, fifth frame")


def test_box_capacity_one_short(hip_module):
    """tloam_segment with room for one box fewer than there are clusters: n_boxes reports them all, the boxes that fit are
    right, the row after them is not written"""
    reg = hip_module
    sc = SC.scene(SC.BOX_SCENE)
    ref = SC.reference(SC.BOX_SCENE)
    K = len(ref["boxes"])
    assert K >= 2 and not ref["margins"]
    R = fresh(reg)
    cfg = SC.seg_config(reg, SC.cfg_of(sc.over))
    a = np.ascontiguousarray(sc.xyz, np.float64)
    n = len(a)
    ring = np.zeros(n, np.int32)
    lists = {k: np.zeros(n, np.int32) for k in KEYS}
    cnt = {k: C.c_size_t(0) for k in ("ground", "object", "segmented", "edge", "general", "boxes")}
    guard = -12345.0
    boxes = np.full((K + 1, 6), guard)
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))    # noqa: E731
    rc = R.L.tloam_segment(R.h, C.byref(cfg), dp(a), n, ip(ring), ip(lists["ground"]), C.byref(cnt["ground"]),
                           ip(lists["object"]), C.byref(cnt["object"]), ip(lists["segmented"]), ip(lists["label"]),
                           C.byref(cnt["segmented"]), ip(lists["edge"]), C.byref(cnt["edge"]), ip(lists["general"]),
                           C.byref(cnt["general"]), dp(boxes), K - 1, C.byref(cnt["boxes"]))
    assert rc == 0
    assert cnt["boxes"].value == K
    assert boxes[: K - 1].tobytes() == np.asarray(ref["boxes"][: K - 1], np.float64).tobytes()
    assert (boxes[K - 1:] == guard).all()
    np.testing.assert_array_equal(lists["segmented"][: cnt["segmented"].value], ref["segmented"])
    np.testing.assert_array_equal(lists["label"][: cnt["segmented"].value], ref["label"])
