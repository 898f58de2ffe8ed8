"""-m gpu: the device's component labels (ppgpu_get_grid_labels -> pp_k_reach_tiles / pp_k_reach_merge / pp_k_reach_flatten) against
the definition of tests/reach_replay.py, byte for byte, with the totals ppgpu_set_reach_seed reports; and when they are built."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import clearance_replay as clr
import grid_worlds as gw
import reach_replay as rr
from path_planner_amd.types import REACH_NONE, REACH_SEED_BLOCKED

T = rr.T


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _context(grid=None, res=1.0):
    from path_planner_amd import api
    from path_planner_amd.types import make_config
    ctx = api.Context(0)
    ctx.set_config(make_config())
    if grid is not None:
        ctx.set_grid(grid, res)
    return ctx


def _zeros(rows, cols):
    return np.zeros((rows, cols), dtype=np.uint8)


GRIDS = {
    "1x1free": lambda: _zeros(1, 1), "1x1blocked": lambda: np.ones((1, 1), dtype=np.uint8),
    "open300": lambda: _zeros(300, 300), "all_blocked": lambda: np.ones((40, 40), dtype=np.uint8),
    "checkerboard": lambda: rr.checkerboard(33, 65),
    "diagonal": lambda: rr.diagonal_channel(2 * T + 6), "antidiagonal": lambda: rr.diagonal_channel(2 * T + 6, anti=True),
    "rings": rr.nested_rings, "comb": rr.comb, "isolated": rr.isolated, "serpentine": rr.serpentine, "spiral": rr.spiral,
    "perc300": lambda: rr.percolation(300, 300, 0.59, 1), "perc257x513": lambda: rr.percolation(257, 513, 0.55, 2),
    "perc1030x1027": lambda: rr.percolation(1030, 1027, 0.59, 3),
    "walls": gw.walls_grid,
}
GRIDS.update({"tiny" + s: (lambda s=s: gw.tiny(s).grid) for s in gw.TINY})
GRIDS.update({"words%d" % c: (lambda c=c: gw.words(c).grid) for c in gw.WORDS_COLS})
# T - 1, T, T + 1 and 2T + 1 in each dimension, at the density where ramified components cross the tile borders
SIZES = (T - 1, T, T + 1, 2 * T + 1)
GRIDS.update({"tile%dx%d" % (r, c): (lambda r=r, c=c: rr.percolation(r, c, 0.59, 100 * r + c)) for r in SIZES for c in SIZES})


@functools.lru_cache(maxsize=None)
def _want(name):
    """(grid, labels, (free, components, largest)) of a named grid, computed once per process, read-only."""
    grid = np.ascontiguousarray(GRIDS[name](), dtype=np.uint8)
    labels = rr.labels_numpy(grid)
    grid.setflags(write=False)
    labels.setflags(write=False)
    return grid, labels, rr.totals(labels)


def _a_free_cell(labels):
    free = np.argwhere(labels != REACH_NONE)
    return None if len(free) == 0 else tuple(free[len(free) // 2])


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_labels_equal_the_definition(torch_cuda, name):
    grid, want, (free, comps, largest) = _want(name)
    ctx = _context(grid, 1.0)
    got = ctx.get_grid_labels(*grid.shape)
    assert got.dtype == np.uint32 and got.tobytes() == want.tobytes(), (name, np.argwhere(got != want)[:5])
    cell = _a_free_cell(want)
    if cell is None:
        info = ctx.set_reach_seed(0.5, 0.5)
        assert (info["free_cells"], info["components"], info["reachable_cells"], info["flags"]) == (0, 0, 0, REACH_SEED_BLOCKED)
        assert info["seed_label"] == REACH_NONE
    else:
        info = ctx.set_reach_seed(cell[1] + 0.5, cell[0] + 0.5)
        assert (info["free_cells"], info["components"], info["flags"]) == (free, comps, 0)
        assert info["seed_label"] == want[cell] and info["reachable_cells"] == (want == want[cell]).sum()
    assert ctx.get_grid_labels(*grid.shape).tobytes() == want.tobytes()            # the cached labels


def test_the_named_grids_are_what_they_claim():
    """The figures of the cases above, on the replay alone: a case cannot degenerate unnoticed."""
    assert _want("open300")[1].max() == 0 and _want("open300")[2] == (90000, 1, 90000)
    assert _want("all_blocked")[2] == (0, 0, 0)
    assert _want("checkerboard")[2] == (1073, 1, 1073)
    assert rr.totals(rr.labels_brute(_want("checkerboard")[0], connectivity=4))[1] == 1073
    n = 2 * T + 6
    assert _want("diagonal")[2] == (n, 1, n) and _want("antidiagonal")[2] == (n, 1, n)
    assert _want("rings")[2][1] == 3
    assert _want("comb")[2][1] == 1 and _want("comb")[0][T - 1, 0] == 1 and _want("comb")[0][T, 0] == 0
    iso = _want("isolated")
    assert iso[2][0] == iso[2][1] and iso[2][2] == 1
    assert _want("serpentine")[2] == (8710, 1, 8710)
    assert _want("spiral")[2][1] == 1 and _want("spiral")[2][0] > 2000
    assert _want("perc300")[2][1:] == (1341, 8211) and _want("perc300")[2][1] >= 1000
    assert _want("perc257x513")[2][1:] == (1009, 56094)
    assert _want("perc1030x1027")[2][1:] == (14573, 233626)
    for r in SIZES:
        for c in SIZES:
            assert _want("tile%dx%d" % (r, c))[2][1] >= 4


def test_a_new_grid_of_the_same_shape_relabels(torch_cuda):
    a, _, _ = _want("perc300")
    b = rr.percolation(300, 300, 0.5, 7)
    ctx = _context(a, 1.0)
    assert ctx.get_grid_labels(300, 300).tobytes() == _want("perc300")[1].tobytes()
    ctx.set_grid(b, 1.0)
    assert ctx.get_grid_labels(300, 300).tobytes() == rr.labels_numpy(b).tobytes()


def test_a_changed_keepout_limit_relabels(torch_cuda):
    """The labels are those of the effective grid: gw.walls at limits 0, 1 and 9 (and back)."""
    grid = gw.walls_grid()
    gap2 = clr.gap2_numpy(grid)
    ctx = _context(grid, 1.0)
    seen = set()
    for limit2 in (0, 1, 9, 0):
        ctx.set_keepout_limit2(limit2)
        eff = ((grid != 0) | (gap2 < limit2)).astype(np.uint8)
        assert np.array_equal(ctx.get_grid_blocked(*grid.shape), eff)
        want = rr.labels_numpy(eff)
        assert ctx.get_grid_labels(*grid.shape).tobytes() == want.tobytes(), limit2
        seen.add(rr.totals(want))
    assert len(seen) == 3                                # three different effective grids


def test_labels_are_built_on_first_use_only(torch_cuda):
    """With timing on, a build is timed: none after set_grid alone, one at the first call that needs the labels, none for a second
    call; a seed that moves inside its component builds nothing, one that moves into another component builds its reach set."""
    from path_planner_amd import api
    grid, want, _ = _want("rings")
    n = grid.shape[0]
    ctx = _context(grid, 1.0)
    ctx.enable_timing(True)
    growths = ctx.growth_stats()[0]
    assert ctx.last_reach_timing() == (-1.0, -1.0, -1.0) and ctx.growth_stats()[0] == growths      # set_grid built nothing
    ctx.get_grid_labels(n, n)
    ms = ctx.last_reach_timing()
    assert ms[0] > 0 and ms[1] == -1.0 and ctx.growth_stats()[0] > growths
    ctx.enable_timing(True)                              # forgets the timed build
    ctx.get_grid_labels(n, n)
    assert ctx.last_reach_timing()[0] == -1.0            # the cached labels served
    outer = ctx.set_reach_seed(1.5, 1.5)
    assert ctx.last_reach_timing()[0] == -1.0 and ctx.last_reach_timing()[1] > 0
    ctx.enable_timing(True)
    moved = ctx.set_reach_seed(n - 1.5, n - 2.5)         # the same outer water
    assert moved["seed_label"] == outer["seed_label"] == 0 and moved["reachable_cells"] == outer["reachable_cells"]
    assert ctx.last_reach_timing() == (-1.0, -1.0, -1.0)
    inner = ctx.set_reach_seed(n / 2, n / 2)             # the innermost basin
    assert inner["seed_label"] == want[n // 2, n // 2] != 0 and inner["reachable_cells"] == (want == inner["seed_label"]).sum()
    assert ctx.last_reach_timing()[0] == -1.0 and ctx.last_reach_timing()[1] > 0
    ctx.set_grid(grid, 1.0)                              # stale again: the next call builds
    ctx.enable_timing(True)
    ctx.get_grid_labels(n, n)
    assert ctx.last_reach_timing()[0] > 0
    ctx.enable_timing(False)
    with pytest.raises(api.PpgpuError):
        ctx.last_reach_timing()
