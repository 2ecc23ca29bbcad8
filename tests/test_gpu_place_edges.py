"""-m gpu: place recognition on the named hand-made inputs of tests/place_scenes.py -- the branches of tl_place.hip (DESIGN.md
section 16) that no generator scan reaches: the clamps of the binning on atan2's special values, the second turn of
k_place_bin's grid-stride loop, wave runs of every length with the maximum first, in the middle and last, signed zeros and
denormals, the rank pass beyond 256 and 512 keyframes, exact ties of ring keys, shifts and pairs, empty columns and empty
descriptors, the strict threshold, exclude_recent's first searches, grids other than 20 x 60.

Everything is compared with the numpy restatement (tests/place_np.py) bit for bit: tloam_place_describe's descriptor and keys
as bytes, tloam_place_add_scan's database by test_gpu_place.same_database.  tests/test_place_scenes.py shows on the CPU that
each scene reaches its branch and that no return but the ones axis_clamps declares sits near a bin boundary."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import place_scenes as SC  # noqa: E402
from test_gpu_place import bits, same_database  # noqa: E402

pytestmark = pytest.mark.gpu

WARM_UP = "heights_offset"     # a small scan of the default grid, described first on a context that is to be "used before"


def same_descriptor(got, name, what):
    want = SC.described(name)
    for g, w, part in zip(got, want, ("descriptor", "ring key", "sector key")):
        assert bits(g) == bits(w), f"{name} {what}: {part}"


def place_cfg(reg, sc, **over):
    return reg.default_place_config(**{**sc.grid, **over})


# ---- descriptor scenes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.SMALL_DESC_NAMES)
def test_descriptor_scene(hip_module, name):
    reg = hip_module
    sc = SC.desc_scene(name)
    H = reg.HipRegistration()
    same_descriptor(H.place_describe(sc.xyz, place_cfg(reg, sc)), name, "explicit cfg, fresh context")
    H.close()
    # the context's configuration, on a context used before: bins[] must be zero again after every describe
    H = reg.HipRegistration()
    same_descriptor(H.place_describe(SC.desc_scene(WARM_UP).xyz), WARM_UP, "default configuration")
    H.place_configure(place_cfg(reg, sc, enabled=1))
    for turn in range(3):
        same_descriptor(H.place_describe(sc.xyz), name, f"the context's cfg, describe {turn}")
    same_descriptor(H.place_describe(sc.xyz, place_cfg(reg, sc)), name, "explicit cfg on the used context")
    assert H.place_info()["n_keyframes"] == 0
    H.close()


def test_two_turns(hip_module):
    """more than 1024 x 256 returns: twice in a row on a fresh context, and once after a small scan on another"""
    reg = hip_module
    sc = SC.desc_scene("two_turns")
    assert len(sc.xyz) > SC.TURN
    H = reg.HipRegistration()
    cfg = place_cfg(reg, sc)
    same_descriptor(H.place_describe(sc.xyz, cfg), "two_turns", "first")
    same_descriptor(H.place_describe(sc.xyz, cfg), "two_turns", "second in a row")
    H.close()
    H = reg.HipRegistration()
    same_descriptor(H.place_describe(SC.desc_scene("runs").xyz), "runs", "small scan first")
    same_descriptor(H.place_describe(sc.xyz), "two_turns", "after a small scan")
    same_descriptor(H.place_describe(SC.desc_scene("runs").xyz), "runs", "small scan after the large one")
    H.close()


def test_scenes_of_one_grid_follow_each_other(hip_module):
    """every default-grid scene through one context, there and back: no scene leaves anything in bins[] for the next"""
    reg = hip_module
    names = [n for n in SC.SMALL_DESC_NAMES if SC.desc_scene(n).grid == SC.grid_of()]
    assert len(names) >= 2
    H = reg.HipRegistration()
    for name in names + names[::-1]:
        same_descriptor(H.place_describe(SC.desc_scene(name).xyz), name, "in a row")
    H.close()


# ---- database scenes -----------------------------------------------------------------------------------------------------
def feed(H, sc):
    ids = [H.place_add_scan(s, np.eye(4), SC.FIRST_FRAME + f) for f, s in enumerate(sc.scans)]
    assert ids == list(range(len(sc.scans)))


def read_back(H):
    kf = H.place_read_keyframes()
    loops = [tuple(sorted((k, bits(v) if isinstance(v, float) else v) for k, v in L.items())) for L in H.place_loops()]
    return {k: v.tobytes() for k, v in kf.items()}, loops


@pytest.mark.parametrize("name", SC.DB_NAMES)
def test_database_scene(hip_module, name):
    reg = hip_module
    sc = SC.db_scene(name)
    db = SC.restated(name)
    over = {**sc.cfg, **sc.device}
    A = reg.HipRegistration()
    A.place_configure(enabled=1, **over)
    feed(A, sc)
    same_database(A, db)
    first = read_back(A)
    A.place_configure(enabled=1, **over)        # the same context again, from an emptied database
    assert A.place_info()["n_keyframes"] == 0 and A.place_info()["n_loops"] == 0
    feed(A, sc)
    same_database(A, db)
    assert read_back(A) == first, f"{name}: second run"
    A.close()
    B = reg.HipRegistration()                   # a second context
    B.place_configure(enabled=1, **over)
    feed(B, sc)
    same_database(B, db)
    assert read_back(B) == first, f"{name}: second context"
    B.close()
