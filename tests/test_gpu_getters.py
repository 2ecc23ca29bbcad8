"""-m gpu: tloam_get_correspondences has one read path -- a column of the set read once and gathered through an index map -- for
both forms a frame leaves its factors in: the compact set (the first seg_n rows as they stand) and the direct set (a row per
source point, the rows that hold a factor sorted by source index).  Every combination of output pointers a caller may pass gives
the bytes of the full call, on the smallest frames that reach either form."""
import ctypes as C

import numpy as np
import pytest

from tloam_amd import synth

pytestmark = pytest.mark.gpu

BIG = 1 << 30
E_INVALID = -1
COLUMNS = ("idx", "a", "b", "d", "w", "cost")
FILL = 12345.0   # what an output the call must leave alone holds before and after it


def _frames(hip_module):
    lifted = hip_module.default_config(planar_maxnum=BIG, ground_maxnum=BIG, edge_maxnum=BIG, sphere_maxnum=BIG)
    return {
        "compact": (synth.make_scene(seed=70), hip_module.default_config(), 0),
        # 148 000 slots, above the thread-per-query limit of 131 072: with no cap that binds the frame keeps a direct set
        "direct": (synth.make_scene(seed=82, n_src=(70_000, 40_000, 30_000, 8_000), n_tgt=(40_000, 30_000, 20_000, 5_000)), lifted, 1),
    }


def _buffers(cap):
    return dict(idx=np.full(cap, -7, np.int32), a=np.full((cap, 3), FILL), b=np.full((cap, 3), FILL), d=np.full(cap, FILL),
                w=np.full(cap, FILL), cost=np.full(cap, FILL))


def _call(H, kind, cap, bufs, only=None):
    """tloam_get_correspondences with the output pointers of `only` (None: all six), the others NULL -> (rc, n)"""
    def ptr(name):
        if only is not None and name not in only:
            return None
        t = C.c_int32 if name == "idx" else C.c_double
        return bufs[name].ctypes.data_as(C.POINTER(t))
    n = C.c_size_t(0)
    rc = H.L.tloam_get_correspondences(H.h, int(kind), cap, C.byref(n), *[ptr(name) for name in COLUMNS])
    return rc, n.value


@pytest.mark.parametrize("form", ["compact", "direct"])
def test_every_pointer_combination_reads_the_bytes_of_the_full_call(hip_module, form):
    sc, cfg, direct = _frames(hip_module)[form]
    H = hip_module.HipRegistration(cfg)
    H.set_frames(sc.source, sc.target)
    rc, T, st = H.scan_match(sc.T_pred)
    assert rc == 0 and H.info()["direct_set"] == direct, (rc, H.info())
    full = {}
    for kind in range(4):
        cap = len(sc.source.cloud(kind)) + 8
        written = {"idx", "a", "w", "cost"} | ({"b"} if kind == hip_module.KIND_EDGE else set()) | \
                  ({"d"} if kind in (hip_module.KIND_PLANAR, hip_module.KIND_GROUND) else set())
        ref = _buffers(cap)
        rc, n = _call(H, kind, cap, ref)
        assert rc == 0 and n == st["n_corr"][kind] and 0 < n <= cap, (kind, rc, n, st["n_corr"])
        assert np.all(np.diff(ref["idx"][:n]) > 0) and ref["idx"][0] >= 0      # source-index order
        untouched = _buffers(cap)
        for name in COLUMNS:                                                   # nothing behind the n rows, nothing in b / d
            lo = n if name in written else 0                                   # of a kind that has none
            assert ref[name][lo:].tobytes() == untouched[name][lo:].tobytes(), (kind, name)
        full[kind] = ref
        # no output pointer at all: the count alone
        rc, n0 = _call(H, kind, cap, _buffers(cap), only=())
        assert rc == 0 and n0 == n, (kind, rc, n0)
        # one output pointer: that column of the full call byte for byte, if the kind has it; the others as they were passed
        for name in COLUMNS:
            one = _buffers(cap)
            rc, n1 = _call(H, kind, cap, one, only=(name,))
            assert rc == 0 and n1 == n, (kind, name, rc, n1)
            for other in COLUMNS:
                want = ref if other == name else untouched
                assert one[other].tobytes() == want[other].tobytes(), (kind, name, other)
        # a capacity one short: refused, with the count
        rc, n2 = _call(H, kind, n - 1, _buffers(cap))
        assert rc == E_INVALID and n2 == n, (kind, rc, n2)
    # tloam_get_costs: the cost column of the kind the residual type maps to
    for rt, kind in ((hip_module.RES_PLANE, hip_module.KIND_PLANAR), (hip_module.RES_LINE, hip_module.KIND_EDGE),
                     (hip_module.RES_POINT, hip_module.KIND_SPHERE)):
        cap = len(sc.source.cloud(kind)) + 8
        cost = np.full(cap, FILL)
        n = C.c_size_t(0)
        rc = H.L.tloam_get_costs(H.h, int(rt), cap, C.byref(n), cost.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == 0 and n.value == st["n_corr"][kind], (rt, rc, n.value)
        assert cost.tobytes() == full[kind]["cost"].tobytes(), rt
    H.close()
