"""The distance-by-water entry points exist at every layer that needs no GPU — declared in include/ppgpu.h with the layout of their
numpy mirrors, exported by libppgpu.so, bound in path_planner_amd.api — and the definitions the GPU tests compare the device against
(tests/water_replay.py) pin themselves: the Dijkstra on the closed form of open water, on a numpy Bellman-Ford fixed point (and on
scipy where it is installed), on the component labels, the ribbon record on a cell-by-cell walk and on the reach report, and the
detour world of tests/test_gpu_plan_water.py on the oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import reach_replay as rr
import water_replay as wr
from test_contact_trace_abi import _header, _struct_layout
from test_reach_abi import SMALL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ppgpu_set_water_seed", "ppgpu_get_grid_water", "ppgpu_water_distance_at", "ppgpu_ribbon_water_host", "ppgpu_last_water_timing"]
METHODS = ["set_water_seed", "get_grid_water", "water_distance_at", "ribbon_water", "last_water_timing"]
C_TYPES = {"uint64_t": ("<u8", 8)}


def test_header_layout_equals_the_numpy_mirrors(monkeypatch):
    import test_contact_trace_abi as base
    from path_planner_amd import types as T
    monkeypatch.setattr(base, "C_TYPES", dict(base.C_TYPES, **C_TYPES))
    txt = _header()
    for name in SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(\s*ppgpu_ctx\s*\*" % name, txt, flags=re.M), name
    for struct, D, size in (("ppgpu_water_info", T.WATER_INFO_DTYPE, 32), ("ppgpu_ribbon_water_record", T.RIBBON_WATER_DTYPE, 64)):
        fields, got = _struct_layout(txt, struct)
        assert got == D.itemsize == size and size % 16 == 0
        assert [(n, D.fields[n][0].str, D.fields[n][1]) for n in D.names] == fields
    defines = dict(re.findall(r"#define\s+(PPGPU_(?:WATER|RW)_\w+)\s+(\w+)", txt))
    assert int(defines["PPGPU_WATER_NONE"].rstrip("u"), 16) == T.WATER_NONE == 0xFFFFFFFF
    assert (int(defines["PPGPU_WATER_STEP"]), int(defines["PPGPU_WATER_DIAG"]), int(defines["PPGPU_WATER_TILE"])) == (T.WATER_STEP, T.WATER_DIAG, T.WATER_TILE) == (12, 17, 32)
    assert int(defines["PPGPU_WATER_MAX_LIM2"].rstrip("u")) == T.WATER_MAX_LIM2 == 1024
    assert T.WATER_DIAG ** 2 > 2 * T.WATER_STEP ** 2                     # 17 / 12 > sqrt(2): the certified upper bound
    for name in ("SEED_BLOCKED", "NO_MAP"):
        assert int(defines["PPGPU_WATER_" + name].rstrip("u"), 16) == getattr(T, "WATER_" + name), name
    for name in ("ANY_DRY", "WHOLE_DRY", "DEGENERATE", "NO_SEED", "NO_MAP"):
        assert int(defines["PPGPU_RW_" + name].rstrip("u"), 16) == getattr(T, "RW_" + name), name
    full = open(os.path.join(ROOT, "include", "ppgpu.h")).read()
    section = full[full.index("distance by water"):]
    for cite in ("GridWorldMap.cpp:84-93", "NOT a lower bound", "17 * rows * cols", "gap2(A, B) < lim2"):
        assert cite in section, cite
    kernels = open(os.path.join(ROOT, "path_planner_amd", "csrc", "pp_k_water.h")).read()
    assert "PP_WATER_TILE PPGPU_WATER_TILE" in kernels
    assert '#include "pp_k_water.h"' in open(os.path.join(ROOT, "path_planner_amd", "csrc", "pp_kernels.h")).read()


def test_library_exports_and_binding_has_them():
    from path_planner_amd import api
    lib = C.CDLL(api.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS
        assert getattr(api.LIB, name).restype is C.c_int
    for method in METHODS:
        assert callable(getattr(api.Context, method)), method


def test_host_planner_declares_the_switch():
    inc = os.path.join(ROOT, "path_planner_amd", "host", "include", "path_planner_amd")
    assert "void setPlanWater(bool on)" in open(os.path.join(inc, "World.h")).read()
    assert "void setPlanWater(bool on)" in open(os.path.join(inc, "Executive.h")).read()
    planner = open(os.path.join(inc, "Planner.h")).read()
    assert "WaterReport Water;" in planner and "Planner::Stats::WaterReport water;" in planner
    cli = open(os.path.join(ROOT, "path_planner_amd", "host", "tools", "plan_cli.cpp")).read()
    for key in ("plan_water", "plan_water_file", "water_cells", "water_max_metres", "water_seed_blocked", "water_rounds", "ribbons_dry",
                "nearest_ribbon_by_water", "nearest_ribbon_water_metres", "nearest_ribbon_straight_metres"):
        assert key in cli, key


# ------------------------------------------------------------------------------------------------------------ the replay's map
def test_open_water_is_the_octile_closed_form():
    g = np.zeros((9, 13), dtype=np.uint8)
    r, c = np.indices(g.shape)
    for seed in ((0, 0), (4, 6), (8, 12), (3, 11)):
        dr, dc = np.abs(r - seed[0]), np.abs(c - seed[1])
        want = 12 * np.maximum(dr, dc) + 5 * np.minimum(dr, dc)
        got = wr.wd_dijkstra(g, seed)
        assert got.dtype == np.uint32 and np.array_equal(got, want)
        assert wr.totals(got) == (g.size, int(want.max()), int(np.argmax(want.ravel() == want.max())))


def _seeds(g):
    """The first, the middle and the last free cell, a blocked cell, no cell."""
    free, blocked = np.argwhere(g == 0), np.argwhere(g != 0)
    out = [tuple(free[k]) for k in sorted({0, len(free) // 2, len(free) - 1})] if len(free) else []
    return out + ([tuple(blocked[0])] if len(blocked) else []) + [None]


@pytest.mark.parametrize("name", sorted(SMALL))
def test_dijkstra_equals_the_bellman_ford_fixed_point_and_the_labels(name):
    g = SMALL[name]()
    labels = rr.labels_numpy(g)
    for seed in _seeds(g):
        got = wr.wd_dijkstra(g, seed)
        assert np.array_equal(got, wr.wd_bellman_ford(g, seed)), (name, seed)
        if seed is None or g[seed]:
            assert (got == wr.NONE).all() and wr.totals(got) == (0, 0, wr.NONE)
        else:
            # a cell has a distance iff it carries the label of the seed's cell
            assert np.array_equal(got != wr.NONE, labels == labels[seed]), (name, seed)
            assert got[seed] == 0 and (got == 0).sum() == 1
            wet, top, far = wr.totals(got)
            assert wet == (labels == labels[seed]).sum() and got.ravel()[far] == top == got[got != wr.NONE].max() and not (got.ravel()[:far] == top).any()


@pytest.mark.parametrize("name", ["perc59", "rings", "spiral", "checkerboard", "comb"])
def test_dijkstra_equals_scipy(name):
    sp = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    g = SMALL[name]()
    rows, cols = g.shape
    idx = np.arange(g.size).reshape(g.shape)
    src, dst, cost = [], [], []
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr or dc:
                a = idx[max(0, -dr):rows - max(0, dr), max(0, -dc):cols - max(0, dc)]
                b = idx[max(0, dr):rows - max(0, -dr), max(0, dc):cols - max(0, -dc)]
                ok = (g.ravel()[a] == 0) & (g.ravel()[b] == 0)
                src.append(a[ok]); dst.append(b[ok]); cost.append(np.full(int(ok.sum()), 17 if dr and dc else 12))
    graph = sp.csr_matrix((np.concatenate(cost), (np.concatenate(src), np.concatenate(dst))), shape=(g.size, g.size))
    for seed in _seeds(g)[:2]:
        d = csgraph.dijkstra(graph, indices=int(idx[seed]))
        want = np.where(np.isinf(d), float(wr.NONE), d).astype(np.uint32).reshape(g.shape)
        want[g != 0] = wr.NONE
        assert np.array_equal(wr.wd_dijkstra(g, seed), want), (name, seed)


# ------------------------------------------------------------------------------------------------------------ ribbon records
def test_approach_map_equals_the_cell_by_cell_window():
    g = SMALL["rings"]()
    wd = wr.wd_dijkstra(g, (1, 1))
    rng = np.random.default_rng(3)
    for lim2 in (0, 1, 2, 4, 5, 9, 10, 1024):
        ad = wr.approach_map(wd, lim2)
        for r, c in rng.integers(0, 39, size=(12, 2)):
            assert ad[r, c] == wr.approach(wd, int(r), int(c), lim2), (lim2, r, c)
        if lim2 == 0:
            assert (ad == wr.NONE).all()                     # no cell has gap2 < 0: the sample's own cell does not count either
        if lim2 == 1:
            assert ad[0, 0] == 0 and ad[1, 1] == 0 and ad[2, 2] == 0 and ad[3, 3] == 17      # gap2 0: the cell and its eight neighbours


@pytest.mark.parametrize("limit2", [0, 1, 9])
def test_wet_samples_are_the_samples_the_reach_report_does_not_call_out(limit2):
    for world in (rr.plan_world, wr.detour_world):
        w, init, calls, gap2 = world()
        wd, (wet, top, far, index), recs, keys = wr.plan_water(w, gap2, limit2)
        labels, label, _, reach = rr.plan_reach(w, gap2, limit2)
        assert np.array_equal(recs["wet_samples"], reach["samples"] - reach["out_samples"]) and np.array_equal(recs["samples"], reach["samples"])
        assert np.array_equal(recs["length"], reach["length"]) and np.array_equal(recs["pitch"], reach["pitch"]) and np.array_equal(recs["lim2"], reach["lim2"])
        assert wet == (labels == label).sum() and index == int(w.start5[1]) * 83 + int(w.start5[0])
        if limit2 == 9 and world is rr.plan_world:
            # ribbon 0 lies wholly inside the keep-out band: its own cells have no distance, the window finds water beside them
            _, _, _, r, c, _, _ = wr.sample_cells(wd.shape, w.res, w.ribbons4[0])
            assert (wd[r, c] == wr.NONE).all() and recs["wet_samples"][0] == recs["samples"][0] == 51 and recs["flags"][0] == 0
            assert list(recs["wet_samples"]) == [51, 0, 12] and keys["ribbons_dry"] == 1


def test_detour_world_on_numpy_and_on_the_oracle():
    """The wall of row 27 is open at columns 78-82 only: ribbon 1, behind it, is 62.6 m away by water and 18.8 m in a straight line (11 m
    by water in the planning world), and the reference's planner still finds a goal."""
    import oracle as orc
    w, init, calls, gap2 = wr.detour_world()
    assert w.grid[rr.PLAN_WALL_ROW].sum() == 83 - 5 and not w.grid[rr.PLAN_WALL_ROW, 78:83].any() and w.grid[rr.PLAN_WALL_ROW, 40:45].all()
    _, _, recs, keys = wr.plan_water(w, gap2, 0)
    pw, _, _, pgap2 = rr.plan_world()
    _, _, precs, _ = wr.plan_water(pw, pgap2, 0)
    assert (recs["min_ad"][1], precs["min_ad"][1]) == (751, 132) and recs["nearest_metres"][1] == 751.0 / 12.0 and recs["nearest_sample"][1] == 50
    assert recs["min_ad"][0] == precs["min_ad"][0] == 48                  # the ribbon on the start's side is as far as it was
    assert keys == {"water_cells": 2981, "water_max_metres": 122.5, "water_seed_blocked": False, "ribbons_dry": 0, "nearest_ribbon_by_water": 2,
                    "nearest_ribbon_water_metres": 0.0, "nearest_ribbon_straight_metres": keys["nearest_ribbon_straight_metres"]}
    assert 1.7 < keys["nearest_ribbon_straight_metres"] < 1.8
    orc.O.ppo_set_ribbon_width(w.cfg.ribbon_width)
    rc, st, plan, _, _ = orc.World(w.cfg, w.grid, w.res, w.obst).plan(w.ribbons4, w.start5, calls * 1e-3, 1000.0, 1e-3, initial_samples=init)
    assert rc == 0 and st.first_goal_iteration >= 0 and len(plan) >= 1
