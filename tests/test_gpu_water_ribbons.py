"""-m gpu: the ribbon records of the distance by water (ppgpu_ribbon_water_host -> pp_k_water_ribbons) field for field against
tests/water_replay.py, on the grid and the ribbons of tests/test_gpu_reach_ribbons.py; the report agrees with the reach report on which
samples can be approached at all; and what the entry point refuses."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import reach_replay as rr
import water_replay as wr
from test_gpu_reach_ribbons import RIBBONS, RES, WIDTH_CELLS, _ribbon_grid
from path_planner_amd.types import (DIST_CAP2, WATER_NONE, WATER_MAX_LIM2, WATER_SEED_BLOCKED, WATER_NO_MAP, RIBBON_WATER_DTYPE, RW_ANY_DRY, RW_WHOLE_DRY,
                                    RW_DEGENERATE, RW_NO_SEED, RW_NO_MAP)

PPGPU_EINVAL, PPGPU_ESTATE = -1, -4
# in cells, beside the imported ones: one that the diagonal through the outer seed mirrors onto itself (open water is symmetric about
# it, so the two ends tie for the largest distance and mirrored samples in the middle for the smallest), and one along the seed's row
EXTRA = np.array([[12.5, 4.5, 4.5, 12.5], [2.5, 2.5, 9.5, 2.5]], dtype=np.float64)
SEEDS = {"outer": (2.5, 2.5), "basin": (35.5, 24.5)}


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


def _compare(got, want, what):
    assert got.dtype == RIBBON_WATER_DTYPE
    for f in RIBBON_WATER_DTYPE.names:
        assert np.array_equal(got[f], want[f]), (what, f, np.nonzero(got[f] != want[f])[0][:5], got[f][:8], want[f][:8])


@pytest.mark.parametrize("key", sorted(RES))
def test_ribbon_records_equal_the_definition(torch_cuda, key):
    res = RES[key]
    grid = _ribbon_grid()
    ribbons = np.concatenate([RIBBONS, EXTRA]) * res
    width = WIDTH_CELLS * res
    labels = rr.labels_numpy(grid)
    ctx = _context(grid, res)
    for what, (cx, cy) in SEEDS.items():
        sx, sy = cx * res, cy * res
        info = ctx.set_water_seed(sx, sy)
        cell, index = wr.seed_index(grid, res, sx, sy)
        assert info["seed_cell"] == index != WATER_NONE
        wd = wr.wd_dijkstra(grid, cell)
        want = wr.ribbon_records(wd, res, ribbons, width)
        got = ctx.ribbon_water(ribbons, width)
        _compare(got, want, (key, what))
        # wet is "not OUT" of the reach report seeded at the same pose
        ctx.set_reach_seed(sx, sy)
        reach = ctx.ribbon_reach(ribbons, width)
        assert np.array_equal(got["wet_samples"], reach["samples"] - reach["out_samples"]) and np.array_equal(got["samples"], reach["samples"])
        assert np.array_equal(got["lim2"], reach["lim2"]) and (got["lim2"] == 4).all()
        if what == "outer":
            # the cases are what they claim to be
            assert want["samples"][0] > 64 and want["flags"][0] == 0 and want["wet_samples"][0] == want["samples"][0]
            for i in (1, 2):       # through the basin: wet, dry, wet again
                assert want["flags"][i] == RW_ANY_DRY and 0 < want["wet_samples"][i] < want["samples"][i]
                assert want["start_ad"][i] != WATER_NONE and want["end_ad"][i] != WATER_NONE
            assert want["flags"][7] == RW_ANY_DRY and want["start_ad"][7] != WATER_NONE and want["end_ad"][7] == WATER_NONE
            for i in (8, 9):       # wholly outside the grid: its samples are clamped onto the border's cells, which are wet
                assert want["flags"][i] == 0 and want["wet_samples"][i] == want["samples"][i]
            assert want["flags"][10] == RW_ANY_DRY | RW_WHOLE_DRY and want["nearest_sample"][10] == want["farthest_sample"][10] == -1
            assert want["min_ad"][10] == want["max_ad"][10] == WATER_NONE and np.isposinf(want["nearest_metres"][10])
            assert want["flags"][11] == RW_DEGENERATE and want["samples"][11] == 1 and want["pitch"][11] == 0 and want["nearest_sample"][11] == 0
            assert want["flags"][12] == RW_DEGENERATE | RW_ANY_DRY | RW_WHOLE_DRY
            assert want["samples"][15] > 4096 and want["flags"][15] == RW_ANY_DRY
            # both tie rules: the lowest index wins
            tie, row = len(RIBBONS), len(RIBBONS) + 1
            _, _, _, r, c, _, _ = wr.sample_cells(grid.shape, res, ribbons[tie])
            ad = wr.approach_map(wd, 4)[r, c]
            assert (ad == ad.max()).sum() >= 2 and ad[0] == ad[-1] == ad.max() and want["farthest_sample"][tie] == 0
            assert (ad == ad.min()).sum() >= 2 and want["nearest_sample"][tie] == np.nonzero(ad == ad.min())[0][0] > 0
            assert want["min_ad"][row] == 0 and want["nearest_sample"][row] == 0 and want["nearest_metres"][row] == 0.0
            assert want["farthest_sample"][row] > want["samples"][row] // 2 and want["max_ad"][row] == want["end_ad"][row]
        else:
            assert want["flags"][0] == RW_ANY_DRY | RW_WHOLE_DRY and want["flags"][10] == 0 and want["min_ad"][12] == 0


def test_ribbon_records_with_a_blocked_seed_and_without_a_map(torch_cuda):
    grid = _ribbon_grid()
    ribbons = np.array([[1.0, 1.0, 20.0, 9.0], [35.5, 24.5, 35.5, 10.0], [7.0, 7.0, 7.0, 7.0]])
    ctx = _context(grid, 1.0)
    info = ctx.set_water_seed(25.5, 15.5)                    # on the ring wall
    assert info["flags"] == WATER_SEED_BLOCKED and info["wet_cells"] == 0 and info["seed_cell"] == WATER_NONE and grid[15, 25] == 1
    want = wr.ribbon_records(None, 1.0, ribbons, 2.0, seed_flags=WATER_SEED_BLOCKED)
    _compare(ctx.ribbon_water(ribbons, 2.0), want, "blocked seed")
    assert list(want["flags"]) == [RW_NO_SEED, RW_NO_SEED, RW_NO_SEED | RW_DEGENERATE] and not want["wet_samples"].any()
    assert (want["min_ad"] == WATER_NONE).all() and (want["nearest_sample"] == -1).all() and np.isposinf(want["nearest_metres"]).all()
    # the base Map: nothing is charted
    ctx.set_grid(None, 0.0)
    info = ctx.set_water_seed(1.0, 1.0)
    assert info["flags"] == WATER_NO_MAP and info["wet_cells"] == 0
    want = wr.ribbon_records(None, 0.0, ribbons, 2.0, no_map=True)
    _compare(ctx.ribbon_water(ribbons, 2.0), want, "no map")
    assert list(want["flags"]) == [RW_NO_MAP, RW_NO_MAP, RW_NO_MAP | RW_DEGENERATE] and list(want["samples"]) == [2, 2, 1]


def test_the_widest_window_and_the_one_beyond_it(torch_cuda):
    """lim2 = PPGPU_WATER_MAX_LIM2 exactly (ribbon_width + resolution / 4 = 32 cells): cells up to 32 away in a row or column count;
    one more is refused."""
    from path_planner_amd import api
    grid = _ribbon_grid()
    ribbons = np.array([[35.5, 24.5, 36.5, 24.5], [69.5, 47.5, 60.0, 40.0], [35.0, 24.0, 35.0, 24.0]])      # in the basin, near a corner, a point in the basin
    ctx = _context(grid, 1.0)
    ctx.set_water_seed(2.5, 2.5)
    wd = wr.wd_dijkstra(grid, (2, 2))
    width = 31.75
    assert rr.ribbon_lim2(1.0, width) == WATER_MAX_LIM2
    want = wr.ribbon_records(wd, 1.0, ribbons, width)
    by_hand = wr.ribbon_record(wd, 1.0, ribbons[1], width)          # (cell by cell, without the shifted minimum)
    assert by_hand.tobytes() == want[1].tobytes()
    got = ctx.ribbon_water(ribbons, width)
    _compare(got, want, "lim2 1024")
    assert (got["lim2"] == WATER_MAX_LIM2).all() and got["flags"][1] == 0 and got["wet_samples"][0] > 0
    # the basin's cell (24, 35) is 9 rows from the wall's outer side: wet through the window, from water 10 or more cells away
    assert got["min_ad"][2] == wr.approach(wd, 24, 35, 1024) != WATER_NONE and wd[24, 35] == WATER_NONE
    rec = np.zeros(3, dtype=RIBBON_WATER_DTYPE)
    L = api.LIB
    assert L.ppgpu_ribbon_water_host(ctx._h, 3, ribbons.ctypes.data, 31.76, rec.ctypes.data) == PPGPU_EINVAL
    assert "PPGPU_WATER_MAX_LIM2" in L.ppgpu_last_error().decode()
    assert rr.ribbon_lim2(1.0, 31.76) == WATER_MAX_LIM2 + 1 <= DIST_CAP2


def test_refusals(torch_cuda):
    from path_planner_amd import api
    L = api.LIB
    err = lambda: L.ppgpu_last_error().decode()
    ctx = _context(_ribbon_grid(), 0.5)
    rib, rec = np.array([[1.0, 1.0, 5.0, 5.0]]), np.zeros(1, dtype=RIBBON_WATER_DTYPE)
    assert L.ppgpu_ribbon_water_host(ctx._h, 1, rib.ctypes.data, 1.0, rec.ctypes.data) == PPGPU_ESTATE and "ppgpu_set_water_seed" in err()
    ctx.set_reach_seed(1.0, 1.0)                             # the reach seed is another seed
    assert L.ppgpu_ribbon_water_host(ctx._h, 1, rib.ctypes.data, 1.0, rec.ctypes.data) == PPGPU_ESTATE
    ctx.set_water_seed(1.0, 1.0)
    for j in range(4):
        bad = rib.copy()
        bad[0, j] = float("nan")
        assert L.ppgpu_ribbon_water_host(ctx._h, 1, bad.ctypes.data, 1.0, rec.ctypes.data) == PPGPU_EINVAL and "not a number" in err()
    assert L.ppgpu_ribbon_water_host(ctx._h, 1, rib.ctypes.data, float("nan"), rec.ctypes.data) == PPGPU_EINVAL and "not a number" in err()
    assert L.ppgpu_ribbon_water_host(ctx._h, 1, None, 1.0, rec.ctypes.data) == PPGPU_EINVAL
    assert L.ppgpu_ribbon_water_host(ctx._h, -1, rib.ctypes.data, 1.0, rec.ctypes.data) == PPGPU_EINVAL
    assert L.ppgpu_ribbon_water_host(ctx._h, 0, None, 1.0, None) == 0
    # more than 2^22 samples: n + 1 = 2^22 is the last that is taken
    pitch = 0.25
    ok = np.array([[0.0, 3.0, (2 ** 22 - 1) * pitch, 3.0]])
    assert L.ppgpu_ribbon_water_host(ctx._h, 1, ok.ctypes.data, 1.0, rec.ctypes.data) == 0 and rec["samples"][0] == 2 ** 22
    over = np.array([[0.0, 3.0, 2 ** 22 * pitch, 3.0]])
    assert L.ppgpu_ribbon_water_host(ctx._h, 1, over.ctypes.data, 1.0, rec.ctypes.data) == PPGPU_EINVAL and "2^22" in err()
    # ribbon_width + res / 4 above 255 cells is the keep-out rule's own refusal
    assert L.ppgpu_ribbon_water_host(ctx._h, 1, rib.ctypes.data, 254.76 * 0.5, rec.ctypes.data) == PPGPU_EINVAL and "255 cells" in err()
    assert L.ppgpu_ribbon_water_host(ctx._h, 1, rib.ctypes.data, 1.0, rec.ctypes.data) == 0 and rec["flags"][0] == 0
