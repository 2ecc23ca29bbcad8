"""The ctypes mirrors of tloam_odom_config / tloam_odom_stats against the C header, and the odometry frame's defaults
against the shipped yaml files (no GPU needed)."""
import ctypes as C

import abi_kit
from tloam_amd import registration as reg


def test_odom_struct_layout_matches_the_c_header():
    """(every field of every mirror against the header: tests/test_abi_header.py)"""
    for name, S in (("tloam_odom_config", reg.OdomConfig), ("tloam_odom_stats", reg.OdomStats)):
        assert abi_kit.sizes(name) == [C.sizeof(S)] and abi_kit.offsets(name) == [getattr(S, f).offset for f, _ in S._fields_]


def test_odom_defaults_are_the_shipped_yaml():
    cfg = reg.default_odom_config()
    assert cfg.edge_down_sample == 0.1                                                   # lidar_odometry.yaml:8
    sub = dict(ground_down_sample=0.3, ground_down_sample_submap=0.45, edge_down_sample_submap=0.3, sphere_frame_size=3,
               planar_frame_size=3, edge_crop_box_length=100.0, ground_crop_box_length=100.0)   # lidar_odometry.yaml:6-17
    feat = dict(radius=0.2, K=20, min_neigh=10, planar_num=500, sphere_num=300, cvr_scan=0.25, cvr_submap=0.15,
                planar_scan_thres=0.75, planar_submap_thres=0.65, planar_vertic_thres=0.25)      # feature.yaml
    seg = dict(sensor_model=64, sensor_height=1.73, vertical_res=0.4, init_angle=-24.9, sensor_min_range=1.0,
               sensor_max_range=120.0, near_dis=3.0, quadrant=4, num_sec=3, dis=0.3, max_iter=3, ground_seed_num=20,
               ring_min_num=131, start_r=0.35, delta_r=0.0004, delta_p=1.2, delta_a=1.2, min_seg=80)   # segmentation.yaml
    for block, want in (("submap", sub), ("feature", feat), ("seg", seg)):
        for k, v in want.items():
            assert getattr(getattr(cfg, block), k) == v, (block, k)
    over = reg.default_odom_config(edge_down_sample=0.2, feature__radius=0.5)
    assert over.edge_down_sample == 0.2 and over.feature.radius == 0.5 and over.feature.K == 20
