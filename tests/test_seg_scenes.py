"""The scenes of tests/seg_scenes.py on the numpy restatement (CPU): every scene has an empty margin report -- no point is
excluded from the device comparison (tests/test_gpu_segmentation_edges.py) --, reaches the branch it is named for, and gets
the status it declares.  Keeps the GPU file from going vacuous when a generator changes."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import segmentation_np as S  # noqa: E402
import seg_scenes as SC  # noqa: E402


@pytest.mark.parametrize("name", SC.NAMES)
def test_scene(name):
    sc = SC.scene(name)
    cfg = SC.cfg_of(sc.over)
    out = SC.reference(name)
    assert len(sc.xyz) <= SC.MAX_RETURNS
    assert np.array_equal(sc.xyz, SC.f32(sc.xyz), equal_nan=True)
    assert out["margins"] == [], out["margins"][:5]
    assert out["status"] == sc.status
    assert sc.witness(sc.xyz, cfg, sc.first_frame, out)


@pytest.mark.parametrize("name", SC.NAMES)
def test_components_are_the_undirected_neighbour_edges(name):
    """dcvc_components' shortcut (a voxel's points joined through its first member) against every point's own searchKNN
    edges: a point that does not see its own voxel (pitch row height + 1, azimuth column above 300) is a node of its own"""
    sc = SC.scene(name)
    out = SC.reference(name)
    if len(out["object"]) == 0:
        assert sc.status == S.STATUS_TOO_FEW
        return
    V = SC.object_voxels(sc.xyz, SC.cfg_of(sc.over), sc.first_frame, out)
    np.testing.assert_array_equal(S.canonical(S.dcvc_components(V)), S.canonical(SC.components_plain(V)))


def test_scene_names_cover_every_family():
    fam = {n.split("_")[0] for n in SC.NAMES}
    assert {"front", "ground", "polar", "chain", "clusters", "edges"} <= fam


def test_config_mapping_names_every_field():
    """seg_config passes each SegCfg field under the binding's name: a stand-in binding records what it is given"""
    import dataclasses

    class Reg:
        @staticmethod
        def default_seg_config(**over):
            return over
    cfg = S.SegCfg(**{f.name: (f.default + 1 if f.name not in ("sensorModel", "quadrant") else f.default)
                      for f in dataclasses.fields(S.SegCfg)})
    got = SC.seg_config(Reg, cfg)
    assert len(got) == len(dataclasses.fields(S.SegCfg))
    assert sorted(got.values()) == sorted(dataclasses.asdict(cfg).values())
    assert got["num_sec"] == cfg.numSec and got["ring_min_num"] == cfg.ringMinNum and got["delta_a"] == cfg.deltaA
    assert got["delta_r"] == cfg.deltaR and got["start_r"] == cfg.startR and got["min_seg"] == cfg.minSeg
    assert got["sensor_height"] == cfg.sensorHeight and got["init_angle"] == cfg.initAngle
    assert got["vertical_res"] == cfg.verticalRes and got["ground_seed_num"] == cfg.ground_seed_num
    assert got["max_iter"] == cfg.maxIter and got["delta_p"] == cfg.deltaP


def test_bounds_cases():
    """the polarBounds tables of tests/test_gpu_segmentation_edges.py's refusals: an increment that runs out (the restatement
    refuses too), a table above kSegMaxBounds (only the device refuses), and one of 2000 to 4095 entries"""
    assert SC.bounds_reference("increment_runs_out")["status"] == S.STATUS_INVALID
    assert SC.bound_count("increment_runs_out") is None
    assert SC.bound_count("above_the_cap") > SC.MAX_BOUNDS
    assert 2000 <= SC.bound_count("large_table") <= SC.MAX_BOUNDS - 1
    for case in ("above_the_cap", "large_table"):
        ref = SC.bounds_reference(case)
        assert ref["status"] == S.STATUS_OK and ref["margins"] == []


@pytest.mark.parametrize("name", sorted({SC.BOUNDS_SCENE, *SC.REUSE_SCENES, *SC.DETERMINISM_SCENES}))
def test_scenes_run_as_later_frames(name):
    """the scenes the GPU file also runs after another call (minPolar / maxPolar start at 0.0): no margin there either"""
    ref = SC.reference(name, False)
    assert ref["status"] == SC.scene(name).status and ref["margins"] == []
