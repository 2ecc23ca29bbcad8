"""map_io.write_labelled_scan_pcd: the file's header and records, and the rename path."""
import os

import numpy as np
import pytest

from tloam_amd import map_io


def test_a_labelled_scan_is_written_whole_and_read_back(tmp_path):
    rng = np.random.default_rng(3)
    pts = rng.uniform(-50.0, 50.0, (257, 3))
    pts[5] = [np.nan, np.inf, -0.0]
    labels = rng.integers(0, 4, 257).astype(np.uint8)
    path = str(tmp_path / "scan.pcd")
    open(path, "wb").write(b"an older file")
    assert map_io.write_labelled_scan_pcd(path, pts, labels) == 257
    assert os.listdir(tmp_path) == ["scan.pcd"]                      # the temporary name is gone
    raw = open(path, "rb").read()
    head, _, body = raw.partition(b"DATA binary\n")
    lines = head.decode("ascii").splitlines()
    assert "FIELDS x y z label" in lines and "SIZE 8 8 8 1" in lines and "TYPE F F F U" in lines and "POINTS 257" in lines
    rec = np.frombuffer(body, dtype=[("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("label", "u1")])
    assert len(rec) == 257 and rec["label"].tobytes() == labels.tobytes()
    assert np.stack([rec["x"], rec["y"], rec["z"]], axis=1).tobytes() == pts.tobytes()
    with pytest.raises(ValueError):
        map_io.write_labelled_scan_pcd(path, pts, labels[:10])
    assert open(path, "rb").read() == raw                            # a refused write leaves the file
    assert map_io.write_labelled_scan_pcd(str(tmp_path / "none.pcd"), np.zeros((0, 3)), np.zeros(0, np.uint8)) == 0
