"""-m gpu: the device's distance map (ppgpu_get_grid_distance -> pp_k_dist_cols / pp_k_dist_rows) against the definition of
tests/clearance_replay.py, byte for byte, and its lookup at points (ppgpu_grid_clearance_at): gap2 exactly, the metres to 1 ulp."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import clearance_replay as clr
import grid_worlds as gw

WORLDS = ["wide", "tall", "third", "walls", "open"] + ["words%d" % c for c in gw.WORDS_COLS] + ["tiny" + s for s in gw.TINY]
PPGPU_EINVAL = -1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _context(grid, res):
    from path_planner_amd import api
    from path_planner_amd.types import make_config
    ctx = api.Context(0)
    ctx.set_config(make_config())
    if grid is not None:
        ctx.set_grid(grid, res)
    return ctx


def _named(name):
    if name == "far":
        return np.zeros((clr.FAR_N, clr.FAR_N), dtype=np.uint8), clr.FAR_RES
    if name == "all_blocked":
        return np.ones((40, 40), dtype=np.uint8), 1.0
    if name == "1x1":
        return np.zeros((1, 1), dtype=np.uint8), 2.0
    w = gw.WORLDS[name]()
    return w.grid, w.res


@pytest.mark.parametrize("name", WORLDS + ["all_blocked", "1x1", "far"])
def test_distance_map_equals_the_definition(torch_cuda, name):
    grid, res = _named(name)
    want = clr.gap2_numpy(grid)
    ctx = _context(grid, res)
    got = ctx.get_grid_distance(*grid.shape)
    assert got.dtype == np.uint16 and got.tobytes() == want.tobytes(), (name, np.argwhere(got != want)[:5])
    assert ctx.get_grid_distance(*grid.shape).tobytes() == want.tobytes()          # the cached map
    if name == "far":
        assert got.max() == clr.DIST_CAP2 and got[350, 350] == clr.DIST_CAP2 and got[254, 350] == 254 * 254
    if name == "all_blocked":
        assert not got.any()


def test_a_new_grid_rebuilds_the_map(torch_cuda):
    from path_planner_amd import api
    a, b = gw.wide(), gw.tiny("5x7")
    ctx = _context(a.grid, a.res)
    assert ctx.get_grid_distance(a.rows, a.cols).tobytes() == clr.gap2_numpy(a.grid).tobytes()
    ctx.set_grid(b.grid, b.res)
    assert ctx.get_grid_distance(b.rows, b.cols).tobytes() == clr.gap2_numpy(b.grid).tobytes()
    other = b.grid.copy()
    other[0, 3] = 1                                  # the same shape, other cells
    ctx.set_grid(other, b.res)
    assert ctx.get_grid_distance(b.rows, b.cols).tobytes() == clr.gap2_numpy(other).tobytes()
    out = np.zeros(b.rows * b.cols, dtype=np.uint16)
    assert api.LIB.ppgpu_get_grid_distance(ctx._h, out.ctypes.data, out.size - 1) == PPGPU_EINVAL       # capacity below rows * cols
    assert api.LIB.ppgpu_get_grid_distance(ctx._h, None, out.size) == PPGPU_EINVAL
    ctx.set_grid(None, 0.0)                          # the base Map: no grid, no map
    assert api.LIB.ppgpu_get_grid_distance(ctx._h, out.ctypes.data, out.size) == PPGPU_EINVAL
    assert b"no grid" in api.LIB.ppgpu_last_error()


def test_the_map_is_built_on_first_use_only(torch_cuda):
    """With timing on, a build is timed: none after set_grid alone, one at the first call that needs the map, none again until the
    next set_grid."""
    from path_planner_amd import api
    w = gw.wide()
    ctx = _context(w.grid, w.res)
    ctx.enable_timing(True)
    with pytest.raises(api.PpgpuError):
        ctx.last_grid_distance_timing()              # set_grid built nothing
    growths = ctx.growth_stats()[0]
    ctx.grid_clearance_at(np.array([[1.5, 1.5]]))
    assert ctx.last_grid_distance_timing() > 0 and ctx.growth_stats()[0] > growths
    ctx.enable_timing(True)                          # forgets the timed build
    ctx.get_grid_distance(w.rows, w.cols)
    with pytest.raises(api.PpgpuError):
        ctx.last_grid_distance_timing()              # the cached map served
    ctx.set_grid(w.grid, w.res)
    ctx.get_grid_distance(w.rows, w.cols)
    assert ctx.last_grid_distance_timing() > 0


def _points(grid, res, rng):
    """Cell centres, points on cell boundaries (k * res, which the quotient may put in cell k or k - 1), points outside each of the
    four sides, points on blocked cells."""
    rows, cols = grid.shape
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    pts = [np.stack([(c.ravel() + 0.5) * res, (r.ravel() + 0.5) * res], axis=1)]
    k = np.arange(0, max(rows, cols) + 1)
    kx, ky = k[k <= cols], k[k <= rows]
    pts.append(np.stack([kx * res, rng.uniform(0, rows * res, len(kx))], axis=1))                 # on column boundaries
    pts.append(np.stack([rng.uniform(0, cols * res, len(ky)), ky * res], axis=1))                 # on row boundaries
    kk = k[k <= min(rows, cols)]
    pts.append(np.stack([kk * res, kk * res], axis=1))                                            # on corners
    w, h = cols * res, rows * res
    pts.append(np.array([[-0.01 * res, 0.5 * h], [-3.0, 0.5 * h], [w + 0.01 * res, 0.5 * h], [w, 0.5 * h], [w + 7.0, 0.5 * h],
                         [0.5 * w, -0.01 * res], [0.5 * w, -2.0], [0.5 * w, h + 0.01 * res], [0.5 * w, h], [0.5 * w, h + 9.0], [-1.0, -1.0], [w + 1, h + 1]]))
    br, bc = np.nonzero(grid)
    if len(br):
        pts.append(np.stack([(bc + rng.uniform(0.05, 0.95, len(bc))) * res, (br + rng.uniform(0.05, 0.95, len(br))) * res], axis=1))
    return np.concatenate(pts)


@pytest.mark.parametrize("key", ["third", "0.3", "0.07"])
def test_clearance_at_points(torch_cuda, key):
    w = gw.boundary(key)
    gap2 = clr.gap2_numpy(w.grid)
    ctx = _context(w.grid, w.res)
    rng = np.random.default_rng(5)
    p = _points(w.grid, w.res, rng)
    clearance, g2 = ctx.grid_clearance_at(p)
    want = clr.step_gap2(gap2, w.res, p[:, 0], p[:, 1])
    assert np.array_equal(g2.astype(np.int64), want), np.nonzero(g2 != want)[0][:5]
    metres = w.res * np.sqrt(want.astype(np.float64))
    assert np.all(np.abs(clearance - metres) <= np.spacing(metres))
    outside = (p[:, 0] < 0) | (p[:, 1] < 0) | (p[:, 0] / w.res >= w.cols) | (p[:, 1] / w.res >= w.rows)
    assert outside.sum() >= 10 and not g2[outside].any() and not clearance[outside].any()
    br, bc = np.nonzero(w.grid)
    assert not g2[-len(br):].any()                   # the points on blocked cells
    assert (g2 > 0).sum() > 1000
    # either output alone, and none
    from path_planner_amd import api
    only = np.full(len(p), 7, dtype=np.uint32)
    assert api.LIB.ppgpu_grid_clearance_at(ctx._h, len(p), p.ctypes.data, None, only.ctypes.data) == 0 and np.array_equal(only, g2)
    only_m = np.full(len(p), -7.0)
    assert api.LIB.ppgpu_grid_clearance_at(ctx._h, len(p), p.ctypes.data, only_m.ctypes.data, None) == 0 and np.array_equal(only_m, clearance)
    assert api.LIB.ppgpu_grid_clearance_at(ctx._h, len(p), p.ctypes.data, None, None) == 0
    assert api.LIB.ppgpu_grid_clearance_at(ctx._h, 0, None, None, None) == 0
    assert api.LIB.ppgpu_grid_clearance_at(ctx._h, 3, None, only_m.ctypes.data, None) == PPGPU_EINVAL


def test_clearance_at_crosses_the_cap_and_a_ragged_width(torch_cuda):
    """The far grid's centre answers the cap; `wide` (83 columns: padding bits in every row) answers its own map at every cell."""
    grid, res = _named("far")
    ctx = _context(grid, res)
    c = clr.FAR_N * res / 2
    clearance, g2 = ctx.grid_clearance_at(np.array([[c, c], [c, 254.5 * res], [0.5 * res, c]]))
    assert list(g2) == [clr.DIST_CAP2, 254 * 254, 0] and list(clearance) == [res * 255.0, res * 254.0, 0.0]
    w = gw.wide()
    ctx.set_grid(w.grid, w.res)
    r, cc = np.meshgrid(np.arange(w.rows), np.arange(w.cols), indexing="ij")
    p = np.stack([(cc.ravel() + 0.25) * w.res, (r.ravel() + 0.75) * w.res], axis=1)
    _, g2 = ctx.grid_clearance_at(p)
    assert np.array_equal(g2.reshape(w.rows, w.cols), clr.gap2_numpy(w.grid))


def test_clearance_at_without_a_grid(torch_cuda):
    ctx = _context(None, 0.0)
    clearance, g2 = ctx.grid_clearance_at(np.array([[1.0, 2.0], [-5.0, 1e9]]))
    assert np.all(clearance == clr.DBL_MAX) and np.all(g2 == clr.DIST_CAP2)
    ctx.set_grid(gw.tiny("5x7").grid, 4.0)
    ctx.set_grid(None, 0.0)
    clearance, g2 = ctx.grid_clearance_at(np.array([[1.0, 2.0]]))
    assert clearance[0] == clr.DBL_MAX and g2[0] == clr.DIST_CAP2
