"""-m gpu: the device's distance-by-water map (ppgpu_set_water_seed, ppgpu_get_grid_water -> pp_k_water_seed / pp_k_water_round /
pp_k_water_totals) against the Dijkstra of tests/water_replay.py, byte for byte, with the totals of the info block; the invariant
against the component labels; when the map is built; what the entry points refuse; and the look-up of points in the map."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import clearance_replay as clr
import grid_worlds as gw
import reach_replay as rr
import water_replay as wr
from path_planner_amd.types import WATER_NONE, WATER_SEED_BLOCKED, WATER_NO_MAP, WATER_TILE

PPGPU_EINVAL, PPGPU_ESTATE = -1, -4
T = WATER_TILE


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


def _largest(grid):
    """A cell of the largest component: the one that names it."""
    lab = rr.labels_numpy(grid).ravel()
    free = lab != rr.REACH_NONE
    big = int(np.bincount(lab[free].astype(np.int64)).argmax())
    return divmod(big, grid.shape[1])


_N = 3 * T + 5
# name: (grid, the seed cells that are particular to it)
GRIDS = {
    "1x1free": (lambda: np.zeros((1, 1), dtype=np.uint8), []), "1x1blocked": (lambda: np.ones((1, 1), dtype=np.uint8), []),
    "1x40": (lambda: np.zeros((1, 40), dtype=np.uint8), [(0, 33)]), "40x1": (lambda: np.zeros((40, 1), dtype=np.uint8), [(33, 0)]),
    "open33x65": (lambda: np.zeros((33, 65), dtype=np.uint8), []),
    "checkerboard": (lambda: rr.checkerboard(33, 65), [(32, 32), (1, 63)]),       # every step is diagonal, through the tile corners
    "diagonal": (lambda: rr.diagonal_channel(37), [(36, 36)]), "antidiagonal": (lambda: rr.diagonal_channel(37, anti=True), [(0, 36), (36, 0)]),
    "spiral": (rr.spiral, [(0, 0)]),                                               # one 2 591-cell corridor: many rounds
    "serpentine": (rr.serpentine, [(0, 0), (129, 130)]), "comb": (rr.comb, [(63, 0)]),
    "rings": (rr.nested_rings, [(1, 1), (10, 10), (_N // 2, _N // 2)]),           # outside, the middle basin, the inner one
    "perc257x513": (lambda: rr.percolation(257, 513, 0.55, 2), ["largest"]),
    "walls": (gw.walls_grid, ["largest"]),
}
COMMON_SEEDS = [(0, 0), "last", (T - 1, T - 1), (T - 1, T), (T, T), "blocked", "outside"]


@functools.lru_cache(maxsize=None)
def _grid(name):
    g = np.ascontiguousarray(GRIDS[name][0](), dtype=np.uint8)
    g.setflags(write=False)
    return g


def _seed_points(name):
    """{label: (x, y)} at res 1: the common seeds that fit the grid and the grid's own."""
    g = _grid(name)
    rows, cols = g.shape
    out = {}
    for s in COMMON_SEEDS + GRIDS[name][1]:
        if s == "last":
            cell = (rows - 1, cols - 1)
        elif s == "largest":
            cell = _largest(g)
        elif s == "blocked":
            b = np.argwhere(g != 0)
            if len(b) == 0:
                continue
            cell = tuple(b[len(b) // 2])
        elif s == "outside":
            out["outside"] = (cols + 0.5, 0.5)
            continue
        else:
            cell = s
        if cell[0] < rows and cell[1] < cols:
            out[str(s) if isinstance(s, str) else "%d,%d" % cell] = (cell[1] + 0.5, cell[0] + 0.5)
    return out


@functools.lru_cache(maxsize=None)
def _want(name, x, y):
    g = _grid(name)
    cell, index = wr.seed_index(g, 1.0, x, y)
    wd = wr.wd_dijkstra(g, cell)
    wd.setflags(write=False)
    return wd, wr.totals(wd), index


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_map_equals_the_definition(torch_cuda, name):
    g = _grid(name)
    ctx = _context(g, 1.0)
    labels = ctx.get_grid_labels(*g.shape)
    wet_seeds = 0
    for key, (x, y) in _seed_points(name).items():
        want, (wet, top, far), index = _want(name, x, y)
        info = ctx.set_water_seed(x, y)
        got = ctx.get_grid_water(*g.shape)
        print(name, key, "rounds", info["rounds"], "wet", info["wet_cells"], "max", info["max_wd"])
        assert got.dtype == np.uint32 and got.tobytes() == want.tobytes(), (name, key, np.argwhere(got != want)[:5])
        assert (info["wet_cells"], info["max_wd"], info["farthest_cell"], info["seed_cell"]) == (wet, top, far, index), (name, key)
        assert info["flags"] == (WATER_SEED_BLOCKED if index == WATER_NONE else 0), (name, key)
        # the invariant: a cell has a distance iff it carries the label of the seed's cell
        if index == WATER_NONE:
            assert wet == 0 and (got == WATER_NONE).all() and info["rounds"] == 0
        else:
            assert np.array_equal(got != WATER_NONE, labels == labels.ravel()[index]), (name, key)
            assert got.ravel()[index] == 0 and (got == 0).sum() == 1 and info["rounds"] >= 1
            wet_seeds += 1
    assert wet_seeds or name == "1x1blocked"


def test_the_named_grids_are_what_they_claim():
    """The figures of the cases above, on the replay alone: a case cannot degenerate unnoticed."""
    wd, (wet, top, far), _ = _want("checkerboard", 0.5, 0.5)
    assert wet == 1073 and wd[32, 32] == 17 * 32 and wd[0, 64] == 17 * 64 and top == 17 * 64      # diagonal steps only
    wd, (wet, top, far), _ = _want("spiral", 0.5, 0.5)
    assert wet == 2591 and 12 * 2400 < top < 12 * 2590 and wd.ravel()[far] == top    # a corridor; a diagonal step cuts each of its corners
    assert _want("diagonal", 36.5, 36.5)[1][:2] == (37, 17 * 36) and _want("antidiagonal", 36.5, 0.5)[1][:2] == (37, 17 * 36)
    assert _want("serpentine", 0.5, 0.5)[1][0] == 8710 and _want("comb", 0.5, 63.5)[1][0] == rr.totals(rr.labels_numpy(_grid("comb")))[0]
    sizes = [_want("rings", c + 0.5, c + 0.5)[1][0] for c in (1, 10, _N // 2)]
    assert len(set(sizes)) == 3 and sum(sizes) == int((_grid("rings") == 0).sum())
    r, c = _largest(_grid("perc257x513"))
    assert _want("perc257x513", c + 0.5, r + 0.5)[1][0] == 56094
    wd = _want("open33x65", 0.5, 0.5)[0]
    rr_, cc = np.indices(wd.shape)
    assert np.array_equal(wd, 12 * np.maximum(rr_, cc) + 5 * np.minimum(rr_, cc))


def test_map_is_built_when_the_cell_the_grid_or_the_limit_changes(torch_cuda):
    grid = gw.walls_grid()
    rows, cols = grid.shape
    gap2 = clr.gap2_numpy(grid)
    eff9 = ((gap2 < 9) | (grid != 0)).astype(np.uint8)
    lab9 = rr.labels_numpy(eff9)
    r0, c0 = _largest(eff9)
    pairs = np.argwhere((lab9[:, :-1] == lab9[r0, c0]) & (lab9[:, 1:] == lab9[r0, c0]))
    r, c = (int(v) for v in pairs[len(pairs) // 2])                      # (r, c) and (r, c + 1) are free at every limit used below
    x, y = c + 0.25, r + 0.75
    ctx = _context(grid, 1.0)
    first = ctx.set_water_seed(x, y)
    assert first["builds"] == 1 and first["rounds"] >= 1
    again = ctx.set_water_seed(c + 0.9, r + 0.1)                          # the same cell: the cached map
    assert again["builds"] == 1 and again.tobytes() == first.tobytes()
    ctx.enable_timing(True)
    ctx.set_water_seed(x, y)
    assert ctx.last_water_timing() == (-1.0, -1.0)                        # nothing was launched
    moved = ctx.set_water_seed(x + 1.0, y)                                # another cell
    assert moved["builds"] == 2 and moved["seed_cell"] == first["seed_cell"] + 1 and ctx.last_water_timing()[0] > 0
    ctx.set_grid(grid, 1.0)                                               # stale: the next call builds
    assert ctx.set_water_seed(x + 1.0, y)["builds"] == 3
    ctx.set_keepout_limit2(9)
    got = ctx.get_grid_water(rows, cols)                                  # (the getter builds it too)
    info = ctx.set_water_seed(x + 1.0, y)
    assert info["builds"] == 4
    assert np.array_equal(ctx.get_grid_blocked(rows, cols), eff9)
    want = wr.wd_dijkstra(eff9, (r, c + 1))
    assert got.tobytes() == want.tobytes() and (info["wet_cells"], info["max_wd"], info["farthest_cell"]) == wr.totals(want)
    assert info["wet_cells"] < first["wet_cells"]
    ctx.set_keepout_limit2(0)
    back = ctx.set_water_seed(x, y)
    assert back["builds"] == 5 and (back["wet_cells"], back["max_wd"], back["farthest_cell"]) == (first["wet_cells"], first["max_wd"], first["farthest_cell"])
    # a blocked seed, twice: the second finds the map that is all NONE
    b = np.argwhere(grid != 0)[0]
    assert ctx.set_water_seed(b[1] + 0.5, b[0] + 0.5)["builds"] == 6 and ctx.set_water_seed(-1.0, 2.0)["builds"] == 6
    ctx.enable_timing(False)
    from path_planner_amd import api
    with pytest.raises(api.PpgpuError):
        ctx.last_water_timing()


def test_map_does_not_depend_on_the_batch_of_rounds(torch_cuda, monkeypatch):
    """PPGPU_WATER_BATCH (read when a handle is made): rounds issued between two reads of the active counts."""
    g = _grid("spiral")
    want, totals, index = _want("spiral", 0.5, 0.5)
    for batch in ("1", "3", "64"):
        monkeypatch.setenv("PPGPU_WATER_BATCH", batch)
        ctx = _context(g, 1.0)
        info = ctx.set_water_seed(0.5, 0.5)
        assert ctx.get_grid_water(*g.shape).tobytes() == want.tobytes(), batch
        assert (info["wet_cells"], info["max_wd"], info["farthest_cell"]) == totals and info["rounds"] >= 10, batch


def test_refusals(torch_cuda):
    from path_planner_amd import api
    L = api.LIB
    err = lambda: L.ppgpu_last_error().decode()
    grid = gw.walls_grid()
    n = grid.size
    out = np.zeros(n, dtype=np.uint32)
    xy, m, w = np.array([[1.5, 1.5]]), np.zeros(1), np.zeros(1, dtype=np.uint32)
    ctx = _context()
    # no grid: the getter refuses, the seed answers NO_MAP
    assert L.ppgpu_get_grid_water(ctx._h, out.ctypes.data, n) == PPGPU_EINVAL and "no grid" in err()
    ctx.set_grid(grid, 1.0)
    # no seed yet
    assert L.ppgpu_get_grid_water(ctx._h, out.ctypes.data, n) == PPGPU_ESTATE and "ppgpu_set_water_seed" in err()
    assert L.ppgpu_water_distance_at(ctx._h, 1, xy.ctypes.data, m.ctypes.data, w.ctypes.data) == PPGPU_ESTATE and "ppgpu_set_water_seed" in err()
    # a NaN; a refused seed is no seed; the reach seed is another seed
    assert L.ppgpu_set_water_seed(ctx._h, float("nan"), 1.0, None) == PPGPU_EINVAL and "not a number" in err()
    assert L.ppgpu_set_water_seed(ctx._h, 1.0, float("nan"), None) == PPGPU_EINVAL
    ctx.set_reach_seed(1.5, 1.5)
    assert L.ppgpu_get_grid_water(ctx._h, out.ctypes.data, n) == PPGPU_ESTATE
    assert L.ppgpu_set_water_seed(ctx._h, 1.5, 1.5, None) == 0                                   # (out may be NULL)
    # capacity below rows * cols, null outputs
    assert L.ppgpu_get_grid_water(ctx._h, out.ctypes.data, n - 1) == PPGPU_EINVAL and "capacity" in err()
    assert L.ppgpu_get_grid_water(ctx._h, None, n) == PPGPU_EINVAL
    assert L.ppgpu_get_grid_water(ctx._h, out.ctypes.data, n) == 0
    assert L.ppgpu_water_distance_at(ctx._h, 1, None, m.ctypes.data, w.ctypes.data) == PPGPU_EINVAL
    assert L.ppgpu_water_distance_at(ctx._h, -1, xy.ctypes.data, m.ctypes.data, w.ctypes.data) == PPGPU_EINVAL
    assert L.ppgpu_water_distance_at(ctx._h, 0, None, None, None) == 0
    # the base Map
    ctx.set_grid(None, 0.0)
    info = ctx.set_water_seed(1.0, 1.0)
    assert info["flags"] == WATER_NO_MAP and info["wet_cells"] == 0 and info["seed_cell"] == WATER_NONE
    metres, wd = ctx.water_distance_at(xy)
    assert np.isposinf(metres[0]) and wd[0] == WATER_NONE
    with pytest.raises(api.PpgpuError):
        ctx.get_grid_water(3, 3)


@pytest.mark.parametrize("res", [1.0, 0.25])
def test_water_distance_at_reads_the_map(torch_cuda, res):
    grid = rr.nested_rings()
    n = grid.shape[0]
    ctx = _context(grid, res)
    ctx.set_water_seed(1.5 * res, 1.5 * res)
    wd = ctx.get_grid_water(n, n)
    rng = np.random.default_rng(5)
    pts = rng.uniform(-2.0 * res, (n + 2.0) * res, size=(400, 2))
    special = np.array([[0.0, 0.0], [3.0 * res, 7.0 * res], [n * res, 1.0], [1.0, n * res], [-1e-9, 1.0], [(n - 1e-9) * res, 0.5 * res],
                        [7.5 * res, 6.0 * res], [6.0 * res, 6.0 * res], [(n // 2) * res, (n // 2) * res]])     # cell boundaries, the far edges, a wall, a basin
    pts = np.concatenate([special, pts])
    metres, got = ctx.water_distance_at(pts)
    want = np.full(len(pts), WATER_NONE, dtype=np.uint32)
    for i, (x, y) in enumerate(pts):
        cell = rr.seed_cell((n, n), res, float(x), float(y))
        if cell is not None:
            want[i] = wd[cell]
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:5]
    assert np.array_equal(metres, wr.metres(res, want))
    assert got[0] == 17 and got[1] == wd[7, 3] != WATER_NONE and got[2] == got[3] == got[4] == WATER_NONE and got[5] != WATER_NONE
    assert got[6] == WATER_NONE and grid[6, 7] == 1 and got[8] == WATER_NONE and np.isposinf(metres[8]) and (got != WATER_NONE).sum() > 50
