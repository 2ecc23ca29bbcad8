"""Golden files of the segmentation node: tests/golden/seg_<seed>.npz, written by the numpy restatement
(tests/segmentation_np.py) for ray-cast HDL-64E scans (tloam_amd/synth_hdl64.py), so that the GPU tests do not rerun it.
The scan itself is not stored: it is regenerated from the seed and checked against the stored digest.

    python tests/golden/make_seg_golden.py"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

from tloam_amd import synth_hdl64 as G  # noqa: E402
import segmentation_np as S  # noqa: E402

SEEDS = (0, 1, 2)


def golden_scan(seed):
    W = G.make_street(seed)
    return G.scan(W, G.trajectory(1)[0], seed=seed, nan_inf=6)[0]


def digest(xyz):
    return hashlib.sha256(np.ascontiguousarray(xyz, np.float64).tobytes()).hexdigest()


def main():
    for seed in SEEDS:
        xyz = golden_scan(seed)
        o = S.segment(xyz, first_frame=True, literal="fast")
        assert o["status"] == 0 and not o["margins"], (seed, o["status"], o["margins"][:5])
        np.savez_compressed(os.path.join(HERE, f"seg_{seed}.npz"), digest=digest(xyz), ring=o["ring"].astype(np.int8),
                            ground=o["ground"].astype(np.int32), object=o["object"].astype(np.int32),
                            segmented=o["segmented"].astype(np.int32), label=o["label"].astype(np.int32),
                            edge=o["edge"].astype(np.int32), general=o["general"].astype(np.int32), boxes=o["boxes"],
                            literal_differs=bool(o["literal_differs"]))
        print(seed, len(xyz), {k: len(o[k]) for k in ("ground", "object", "segmented", "edge", "general", "boxes")},
              "literal differs:", o["literal_differs"])


if __name__ == "__main__":
    main()
