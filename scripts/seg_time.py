"""The segmentation node (tloam_segment) on one 120 k-return ray-cast HDL-64E scan (tests/golden seed 0), host call to
host return (upload + 14 kernel launches + the index lists back), steady state.  Run it under
rocprofv3 --kernel-trace --stats for the kernels' own times.

    python scripts/seg_time.py [iterations]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
from tloam_amd import registration as reg  # noqa: E402
import make_seg_golden as MG  # noqa: E402

KERNELS = 14   # tl_seg.hip launch_segment; besides: 1 upload, 3 memsets, the control block and up to 8 lists back

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
xyz = MG.golden_scan(0)
H = reg.HipRegistration()
for _ in range(5):
    o = H.segment(xyz)
ts = []
for _ in range(iters):
    t0 = time.perf_counter()
    o = H.segment(xyz)
    ts.append((time.perf_counter() - t0) * 1e3)
ts = np.array(ts)
print("seg_points %d kernels_per_call %d" % (len(xyz), KERNELS))
print("seg_ms median %.4f mean %.4f min %.4f max %.4f (%d calls)" % (np.median(ts), ts.mean(), ts.min(), ts.max(), iters))
print("sizes", {k: len(o[k]) for k in ("ground", "object", "segmented", "edge", "general", "boxes")})
