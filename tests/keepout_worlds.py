"""What the keep-out tests share (include/ppgpu.h, "chart clearance": the effective grid of a limit2): the definition on numpy, the
extra grids of tests/test_gpu_keepout_grid.py, and the planning world of tests/test_gpu_keepout_plan.py with the margin, the
relaxed start and the sizes that tests/test_keepout_abi.py shows, on the oracle alone, to be what the GPU tests need.

A plain module: no fixtures, no device."""
import numpy as np

import clearance_replay as clr
import grid_worlds as gw

LIMITS = (0, 1, 2, 4, 5, 9, 10, 65025)


def effective(grid, limit2, gap2=None):
    """The effective grid at limit2: blocked iff gap2 < limit2, or blocked in the grid as set."""
    grid = np.asarray(grid)
    g2 = clr.gap2_numpy(grid) if gap2 is None else gap2
    return ((g2.astype(np.int64) < int(limit2)) | (grid != 0)).astype(np.uint8)


def strip300():
    """3 x 300: wider than the kernel's tile of 256 columns, 300 % 32 = 12, a few blocked cells on both sides of column 256."""
    g = np.zeros((3, 300), dtype=np.uint8)
    g[1, 7] = g[0, 130] = g[2, 255] = g[1, 256] = g[1, 290] = 1
    return g


def block64():
    """9 x 64: exactly one wave's two words per row, no padding bit."""
    g = np.zeros((9, 64), dtype=np.uint8)
    g[4, 0] = g[4, 31] = g[4, 32] = g[2, 63] = g[7, 40] = 1
    return g


EXTRA_GRIDS = {"strip300": strip300, "block64": block64}

# ------------------------------------------------------------------------------------------------------------ the planning world
# grid_worlds.wide_plan (37 x 83 @ 1.0 m, single blocked cells, two ribbons north of the start) with a margin of 3 m: limit2 = 9
PLAN_MARGIN = 3.0
PLAN_LIMIT2 = 9
# a start three cells east of the pillar at (14, 55): two cells between, gap2 = 4, inside the band of limit2 9
RELAXED_RC = (14, 58)
RELAXED_GAP2 = 4


def plan_world():
    """(workload, initial samples, clock polls, gap2 of its grid)"""
    w, init, calls = gw.wide_plan()
    return w, init, calls, clr.gap2_numpy(w.grid)


def relaxed_start(w):
    r, c = RELAXED_RC
    return np.array([(c + 0.37) * w.res, (r + 0.61) * w.res, 0.0, 2.5, float(w.start5[4])])
