"""Exact free cells for the frontier tests: axis-aligned runs painted into the free-space grid by rays,
one tloam_closed_map_free_add_scan per origin.

With end_margin = 0 and a max_range beyond every ray, an axis-aligned ray from the centre of cell `a` to the centre of the cell
one past `b` marks exactly the cells a .. b: the start cell and the first n - 1 cells stepped into are marked, the end cell
never is (tests/closed_map_free_np.py states the walk).  The painted bits are checked against FreeNP before anything uses them."""
import numpy as np

PAINT = dict(max_range=5000.0, end_margin=0.0)      # the free configuration the painting needs


def run_cells(a, b):
    """the cells a .. b of an axis-aligned run, inclusive, in order"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    d = b - a
    assert (d != 0).sum() <= 1, (a, b)
    n = int(np.abs(d).max())
    e = np.sign(d)
    return a + np.arange(n + 1)[:, None] * e


def free_set(G):
    """the cells whose bit is set in the restated grid G, as a set of tuples"""
    word, bit = np.nonzero(G.bits())
    bz, rest = np.divmod(word, int(G.nb[0]) * int(G.nb[1]))
    by, bx = np.divmod(rest, int(G.nb[0]))
    cells = 4 * (np.stack([bx, by, bz], axis=1) + G.blo) + np.stack([bit & 3, (bit >> 2) & 3, bit >> 4], axis=1)
    return {tuple(c) for c in cells.tolist()}


def paint(G, runs, H=None, compare=None):
    """marks the runs [(a, b), ...] (cells, inclusive, axis-aligned; a == b: the one cell) in the restated grid G -- and on the
    device H through compare(H, G, scan, pose) (tests/test_gpu_closed_map_free.py's scan_and_compare) when given --, one scan
    per origin; asserts that exactly the runs' cells were added to what the grid held -> the set of cells painted"""
    before = free_set(G)
    by_origin, want = {}, set()
    for a, b in runs:
        a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
        cells = run_cells(a, b)
        e = np.sign(b - a) if (a != b).any() else np.array([1, 0, 0])
        by_origin.setdefault(tuple(a.tolist()), []).append(b + e)          # the ray ends in the cell one past b
        want |= {tuple(c) for c in cells.tolist()}
    for a, ends in by_origin.items():
        pose = np.eye(4)
        pose[:3, 3] = G.o + (np.array(a, np.float64) + 0.5) * G.v
        scan = np.ascontiguousarray((np.array(ends, np.float64) - np.array(a, np.float64)) * G.v)
        if H is None:
            G.add_scan(scan, pose)
        else:
            compare(H, G, scan, pose)
    inside = {c for c in want if G.locate([c])[0][0]}
    assert free_set(G) == before | inside, (sorted(free_set(G) ^ (before | inside))[:8])
    return want


def block_runs(lo, hi):
    """the solid block of cells [lo, hi] as runs along x, one per (y, z)"""
    return [((lo[0], y, z), (hi[0], y, z)) for z in range(lo[2], hi[2] + 1) for y in range(lo[1], hi[1] + 1)]


def serpentine_runs(x0=0, y0=0, z0=0):
    """one tile of 32 x 8 x 4 cells at (x0, y0, z0): in the layers z = 0 and z = 2 the rows y = 0, 2, 4, 6 joined at alternating
    ends, the two layers joined through the cell (0, 6, 1) -- tests/test_gpu_closed_map_route.py's maze, painted.  Every cell of
    it is a frontier cell (the rows between are unknown) and the chain is 26-connected only along itself but for the row ends,
    where a diagonal step cuts a corner: its end-to-end path still exceeds 200 cells"""
    runs = []
    for z in (0, 2):
        for y in (0, 2, 4, 6):
            runs.append(((x0, y0 + y, z0 + z), (x0 + 31, y0 + y, z0 + z)))
        for y in (1, 3, 5):
            x = x0 + (31 if y % 4 == 1 else 0)
            runs.append(((x, y0 + y, z0 + z), (x, y0 + y, z0 + z)))
    runs.append(((x0, y0 + 6, z0 + 1), (x0, y0 + 6, z0 + 1)))
    return runs
