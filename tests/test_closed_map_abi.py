"""The closed map without a GPU: the ctypes mirrors of tloam_closed_map_config / _info against the C
header, the defaults, the entry points in the built library, and that its inputs restate as the contract says: the voxel map's
restatement (tests/voxel_map_np.py) fed each keyframe's transformed concatenation."""
import numpy as np
import pytest

import abi_kit
import voxel_map_np as VN
from tloam_amd import registration as reg

CLOSED_MAP_SYMBOLS = ("tloam_closed_map_default_config", "tloam_closed_map_configure", "tloam_closed_map_get_info",
                      "tloam_closed_map_build", "tloam_closed_map_read", "tloam_closed_map_read_box",
                      "tloam_closed_map_read_poses", "tloam_graph_correct_pose")


def test_closed_map_struct_layout_matches_the_c_header():
    """(every field of both mirrors against the header: tests/test_abi_header.py)"""
    assert abi_kit.sizes("tloam_closed_map_config", "tloam_closed_map_info") == [48, 64]
    assert abi_kit.offsets("tloam_closed_map_config") == [0, 8, 32, 36, 40]
    assert abi_kit.constants("TLOAM_CLOSED_MAP_POSES_STORED", "TLOAM_CLOSED_MAP_POSES_CORRECTED", "TLOAM_CLOSED_MAP_POSES_CALLER",
                             "TLOAM_ABI_VERSION") == [0, 1, 2, 8]   # the pose sources; additive: the ABI stays 8


def test_closed_map_defaults():
    cfg = reg.default_closed_map_config()
    assert (cfg.voxel, tuple(cfg.origin), cfg.cloud_mask, cfg.reserved0, cfg.reserve_voxels) == (1.0, (0.0, 0.0, 0.0), 0xF0, 0, 0)
    over = reg.default_closed_map_config(voxel=0.25, origin=(1.0, -2.0, 0.5), cloud_mask=0x0F, reserve_voxels=64)
    assert (over.voxel, tuple(over.origin), over.cloud_mask, over.reserve_voxels) == (0.25, (1.0, -2.0, 0.5), 0x0F, 64)
    with pytest.raises(KeyError):
        reg.default_closed_map_config(enabled=1)
    with pytest.raises(KeyError):
        reg.default_closed_map_config(mask=0xFF)


def test_closed_map_symbols_are_exported():
    abi_kit.assert_exported(CLOSED_MAP_SYMBOLS)
    for name in ("closed_map_configure", "closed_map_build", "closed_map_info", "closed_map_read", "closed_map_read_box",
                 "closed_map_poses"):
        assert callable(getattr(reg.HipRegistration, name))


def test_a_keyframe_that_leaves_the_grid_drops_out_of_the_order_too():
    """the contract's order: ids follow the smallest global index over the keyframes that add -- which is what feeding the
    restatement the adding keyframes alone, ascending, gives"""
    rng = np.random.default_rng(0)
    clouds = [rng.uniform(-20, 20, (500, 3)) for _ in range(4)]
    clouds[1][17] = [float(1 << 21), 0.0, 0.0]   # keyframe 1 leaves the grid
    clouds[2][5] = [np.nan, 0.0, 0.0]            # a non-finite point is left out; its keyframe adds
    V = VN.VoxelMapNP(0.5)
    added = [V.add_frame(c) for c in clouds]
    assert added == [True, False, True, True] and V.overflow_frames == 1
    W = VN.VoxelMapNP(0.5)
    for k in (0, 2, 3):
        W.add_frame(clouds[k])
    assert V.keys.tobytes() == W.keys.tobytes() and V.N.tobytes() == W.N.tobytes() and V.Q.tobytes() == W.Q.tobytes()
    assert int(V.N.sum()) == 3 * 500 - 1
