"""-m gpu: the effective grid of a keep-out limit on the device (ppgpu_set_keepout_limit2 -> pp_k_keepout_bits over the distance
map, then pp_k_grid_row_clear / pp_k_grid_clear over the result), byte for byte against the definition on numpy
(tests/keepout_worlds.py): the effective bits, the chessboard clearance map over them, and the distance map, which stays that of
the grid as set.  Every named grid of tests/test_clearance_abi.py, one wider than the kernel's tile of 256 columns and one of
exactly 64 columns, at every limit of keepout_worlds.LIMITS, in either order of the two calls, and along a walk of limits."""
import ctypes as C

import numpy as np
import pytest

import clearance_replay as clr
import grid_worlds as gw
import keepout_worlds as kw
from test_clearance_abi import GRIDS

pytestmark = pytest.mark.gpu
PPGPU_EINVAL = -1
ALL_GRIDS = dict(GRIDS, **kw.EXTRA_GRIDS)
_REF = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _ref(name):
    """(grid, gap2, {limit2: (effective grid, its chessboard clearance map)}) of a named grid, computed once per process."""
    if name not in _REF:
        g = np.ascontiguousarray(ALL_GRIDS[name](), dtype=np.uint8)
        g2 = clr.gap2_numpy(g)
        by = {}
        for k in kw.LIMITS:
            e = kw.effective(g, k, g2)
            by[k] = (e, gw.clearance_numpy(e))
            e.setflags(write=False); by[k][1].setflags(write=False)
        g.setflags(write=False); g2.setflags(write=False)
        _REF[name] = (g, g2, by)
    return _REF[name]


def _context():
    from path_planner_amd import api
    from path_planner_amd.types import make_config
    ctx = api.Context(0)
    ctx.set_config(make_config())
    return ctx


def _check(ctx, name, k, what):
    g, g2, by = _ref(name)
    rows, cols = g.shape
    assert ctx.get_keepout_limit2() == k, (name, k, what)
    got = ctx.get_grid_blocked(rows, cols)
    assert np.array_equal(got, by[k][0]), (name, k, what, np.argwhere(got != by[k][0])[:5].tolist())
    got = ctx.get_grid_clearance(rows, cols)
    assert np.array_equal(got, by[k][1]), (name, k, what, np.argwhere(got != by[k][1])[:5].tolist())
    got = ctx.get_grid_distance(rows, cols)
    assert np.array_equal(got, g2), (name, k, what, np.argwhere(got != g2)[:5].tolist())


@pytest.mark.parametrize("name", sorted(ALL_GRIDS))
def test_effective_grid_equals_the_definition_at_every_limit(torch_cuda, name):
    g, g2, by = _ref(name)
    ctx = _context()
    ctx.set_grid(g, 0.5)
    _check(ctx, name, 0, "never set")                                  # at 0 the bytes are the grid's own
    assert np.array_equal(by[0][0], (g != 0).astype(np.uint8))
    for k in kw.LIMITS[1:] + (0,):                                     # grid, then limit
        ctx.set_keepout_limit2(k)
        _check(ctx, name, k, "grid then limit")
    for k in kw.LIMITS:                                                # limit, then grid: a fresh handle each, and the same handle again
        fresh = _context()
        fresh.set_keepout_limit2(k)
        assert fresh.get_keepout_limit2() == k
        fresh.set_grid(g, 0.5)
        _check(fresh, name, k, "limit then grid")
        ctx.set_keepout_limit2(k)
        ctx.set_grid(g, 0.5)
        _check(ctx, name, k, "limit then grid, handle reused")
        fresh.close()
    ctx.close()


@pytest.mark.parametrize("name", ["wide", "strip300", "block64", "tiny1x40", "tiny40x1"])
def test_walk_of_limits_and_a_change_of_grid(torch_cuda, name):
    g, g2, by = _ref(name)
    ctx = _context()
    ctx.set_grid(g, 1.0)
    for k in (4, 9, 0, 4):
        ctx.set_keepout_limit2(k)
        _check(ctx, name, k, "walk")
    # the limit survives another grid of another shape, and the first grid again
    other = "block64" if name != "block64" else "strip300"
    ctx.set_grid(_ref(other)[0], 1.0)
    _check(ctx, other, 4, "other grid under the kept limit")
    ctx.set_grid(g, 1.0)
    _check(ctx, name, 4, "first grid again")
    ctx.set_keepout_limit2(4)                                          # the same value again: nothing to do, nothing changed
    _check(ctx, name, 4, "same value")
    ctx.close()


def test_arguments(torch_cuda):
    from path_planner_amd import api
    g, g2, by = _ref("wide")
    rows, cols = g.shape
    ctx = _context()
    ctx.set_grid(g, 1.0)
    ctx.set_keepout_limit2(5)
    assert api.LIB.ppgpu_set_keepout_limit2(ctx._h, 65026) == PPGPU_EINVAL and b"limit2" in api.LIB.ppgpu_last_error()
    _check(ctx, "wide", 5, "after a refused limit")                   # the state is unchanged
    assert api.LIB.ppgpu_set_keepout_limit2(None, 1) == PPGPU_EINVAL and api.LIB.ppgpu_get_keepout_limit2(ctx._h, None) == PPGPU_EINVAL
    ctx.set_keepout_limit2(65025)
    _check(ctx, "wide", 65025, "the cap itself is a limit")
    # get_grid_blocked behaves like get_grid_clearance
    out = np.full(rows * cols + 8, 0xA5, dtype=np.uint8)
    assert api.LIB.ppgpu_get_grid_blocked(ctx._h, out.ctypes.data, rows * cols - 1) == PPGPU_EINVAL
    assert api.LIB.ppgpu_last_error().decode() == "grid blocked: capacity below rows * cols"
    assert api.LIB.ppgpu_get_grid_blocked(ctx._h, None, out.size) == PPGPU_EINVAL and np.all(out == 0xA5)
    assert api.LIB.ppgpu_get_grid_blocked(ctx._h, out.ctypes.data, rows * cols) == 0
    assert np.array_equal(out[:rows * cols].reshape(rows, cols), by[65025][0]) and np.all(out[rows * cols:] == 0xA5)
    # the base Map: the call succeeds, the value is kept and has no effect, and the next grid gets it
    ctx.set_grid(None, 0.0)
    ctx.set_keepout_limit2(9)
    assert ctx.get_keepout_limit2() == 9
    assert api.LIB.ppgpu_get_grid_blocked(ctx._h, out.ctypes.data, out.size) == PPGPU_EINVAL
    assert api.LIB.ppgpu_last_error().decode() == "grid blocked: no grid is set"
    assert api.LIB.ppgpu_set_keepout_limit2(ctx._h, 65026) == PPGPU_EINVAL and ctx.get_keepout_limit2() == 9
    ctx.set_grid(g, 1.0)
    _check(ctx, "wide", 9, "a grid after the base Map")
    ctx.close()


def test_timing_of_a_change(torch_cuda):
    from path_planner_amd import api
    g, g2, by = _ref("walls")
    ctx = _context()
    ctx.enable_timing(True)
    ctx.set_grid(g, 0.25)
    ms = C.c_double(-1.0)
    assert api.LIB.ppgpu_last_keepout_timing(ctx._h, C.byref(ms)) != 0       # no change of the effective grid was timed yet
    ctx.set_keepout_limit2(9)
    on = ctx.last_keepout_timing()
    _check(ctx, "walls", 9, "timed")
    ctx.set_keepout_limit2(0)
    back = ctx.last_keepout_timing()
    _check(ctx, "walls", 0, "timed, back to 0")
    assert 0 < on < 1000 and 0 < back < 1000
    print("keep-out change on a %d x %d grid: %.4f ms on, %.4f ms back to 0" % (g.shape[0], g.shape[1], on, back))
    ctx.close()
