"""map_io.write_raycast_pcd: the file's header and records, the hit points in the map's frame, and the
rename path."""
import os

import numpy as np
import pytest

from tloam_amd import map_io


def test_the_hit_points_are_written_whole_and_read_back(tmp_path):
    rng = np.random.default_rng(5)
    ends = rng.uniform(-30.0, 30.0, (130, 3))
    status = rng.integers(0, 4, 130).astype(np.uint8)
    L = np.linalg.norm(ends, axis=1)
    ranges = np.where(status >= 2, rng.uniform(0.0, 1.0, 130) * L, -1.0)
    c, s = np.cos(0.7), np.sin(0.7)
    pose = np.array([[c, -s, 0.0, 4.0], [s, c, 0.0, -2.5], [0.0, 0.0, 1.0, 1.25], [0.0, 0.0, 0.0, 1.0]])
    path = str(tmp_path / "hits.pcd")
    open(path, "wb").write(b"an older file")
    hit = status >= 2
    assert map_io.write_raycast_pcd(path, pose, ends, status, ranges) == int(hit.sum())
    assert os.listdir(tmp_path) == ["hits.pcd"]                      # the temporary name is gone
    raw = open(path, "rb").read()
    head, _, body = raw.partition(b"DATA binary\n")
    lines = head.decode("ascii").splitlines()
    assert "FIELDS x y z status" in lines and "SIZE 8 8 8 1" in lines and "TYPE F F F U" in lines
    assert f"POINTS {int(hit.sum())}" in lines and f"WIDTH {int(hit.sum())}" in lines
    rec = np.frombuffer(body, dtype=[("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("status", "u1")])
    assert len(rec) == hit.sum() and rec["status"].tobytes() == status[hit].tobytes()
    X = np.stack([rec["x"], rec["y"], rec["z"]], axis=1)
    # back in the sensor frame each point lies on its segment, `range` from the sensor
    back = (X - pose[:3, 3]) @ pose[:3, :3]
    assert np.allclose(np.linalg.norm(back, axis=1), ranges[hit], rtol=0, atol=1e-9)
    assert np.allclose(back, ends[hit] * (ranges[hit] / L[hit])[:, None], rtol=0, atol=1e-9)
    with pytest.raises(ValueError):
        map_io.write_raycast_pcd(path, pose, ends, status[:10], ranges)
    assert open(path, "rb").read() == raw                            # a refused write leaves the file
    none = np.zeros(4, np.uint8)
    assert map_io.write_raycast_pcd(str(tmp_path / "none.pcd"), pose, ends[:4], none, np.full(4, -1.0)) == 0
