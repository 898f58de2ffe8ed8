"""The route-by-water entry points exist at every layer that needs no GPU — declared in include/ppgpu.h with the layout of their numpy
mirror, exported by libppgpu.so, bound in path_planner_amd.api, switched in the host planner and plan_cli — and the definitions the GPU
tests compare the device against (tests/route_replay.py) pin themselves: the step map on the water map, the walk on the step map, the
record on the walk, the vertex list on the walk, open water on its closed form, the approach cell on water_replay.approach, and the
detour world on the strait its route must pass."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import reach_replay as rr
import route_replay as ro
import water_replay as wr
from test_contact_trace_abi import _header, _struct_layout
from test_reach_abi import SMALL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ppgpu_get_grid_water_dirs", "ppgpu_water_routes_host", "ppgpu_last_water_route_timing"]
METHODS = ["get_grid_water_dirs", "water_routes", "last_water_route_timing"]
ROUTE_KEYS = ("water_route_metres", "water_route_turns", "water_route_vertices", "water_route_truncated", "water_route_narrowest_metres", "water_route_first_dir")


def test_header_layout_equals_the_numpy_mirror():
    from path_planner_amd import types as T
    txt = _header()
    for name in SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(\s*ppgpu_ctx\s*\*" % name, txt, flags=re.M), name
    fields, got = _struct_layout(txt, "ppgpu_water_route_record")
    D = T.WATER_ROUTE_DTYPE
    assert got == D.itemsize == 64
    assert [(n, D.fields[n][0].str, D.fields[n][1]) for n in D.names] == fields
    defines = dict(re.findall(r"#define\s+(PPGPU_(?:ROUTE|WR)_\w+)\s+(\w+)", txt))
    assert int(defines["PPGPU_ROUTE_NONE"].rstrip("u"), 16) == T.ROUTE_NONE == 0xFF and int(defines["PPGPU_ROUTE_SEED"].rstrip("u")) == T.ROUTE_SEED == 8
    want = {"DRY": 0x01, "OUTSIDE": 0x02, "AT_SEED": 0x04, "TRUNCATED": 0x08, "NO_SEED": 0x40, "NO_MAP": 0x80}
    for name, value in want.items():
        assert int(defines["PPGPU_WR_" + name].rstrip("u"), 16) == getattr(T, "WR_" + name) == value, name
    assert (T.WR_NO_SEED, T.WR_NO_MAP) == (T.RW_NO_SEED, T.RW_NO_MAP)
    full = open(os.path.join(ROOT, "include", "ppgpu.h")).read()
    section = full[full.index("route by water"):]
    for cite in ("LOWEST code", "the lowest row-major index wins", "the one nearest the seed along the route", "code | flags << 8", "FROM THE SEED",
                 "N(-1,0), S(+1,0), W(0,-1), E(0,+1), NW(-1,-1), NE(-1,+1), SW(+1,-1), SE(+1,+1)", "GridWorldMap.cpp:84-93", "left as they were"):
        assert cite in section, cite
    kernels = open(os.path.join(ROOT, "path_planner_amd", "csrc", "pp_kernels.h")).read()
    assert kernels.index('#include "pp_k_water.h"') < kernels.index('#include "pp_k_route.h"')


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
    assert "void setPlanWaterRoute(bool on)" in open(os.path.join(inc, "World.h")).read()
    assert "void setPlanWaterRoute(bool on)" in open(os.path.join(inc, "Executive.h")).read()
    planner = open(os.path.join(inc, "Planner.h")).read()
    assert "std::vector<RouteReport> Routes;" in planner and "int NearestRoute" in planner and "waterRoutes(" in planner
    cli = open(os.path.join(ROOT, "path_planner_amd", "host", "tools", "plan_cli.cpp")).read()
    for key in ("plan_water_route", "plan_water_route_file") + ROUTE_KEYS:
        assert key in cli, key
    assert "plan_water_route" in open(os.path.join(ROOT, "path_planner_amd", "host", "tools", "mission_sim.cpp")).read()


# ------------------------------------------------------------------------------------------------------------ the replay pins itself
def test_codes_are_water_replays_steps():
    assert ro.OFFSETS == ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1)) and ro.COSTS == (12, 12, 12, 12, 17, 17, 17, 17)
    for k, (dr, dc) in enumerate(ro.OFFSETS):
        assert ro.OFFSETS[ro.OPPOSITE[k]] == (-dr, -dc) and ro.OPPOSITE[ro.OPPOSITE[k]] == k


def _seeds(g):
    """Three free cells: the first, the middle and the last."""
    free = np.argwhere(g == 0)
    return [tuple(int(v) for v in free[k]) for k in sorted({0, len(free) // 2, len(free) - 1})] if len(free) else []


@functools.lru_cache(maxsize=None)
def _world(name, seed):
    import clearance_replay as clr
    g = SMALL[name]()
    wd = wr.wd_dijkstra(g, seed)
    return g, wd, ro.step_map(wd), clr.gap2_numpy(g)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_step_map_walk_record_and_vertices(name):
    g = SMALL[name]()
    rows, cols = g.shape
    res = 0.5
    for seed in _seeds(g):
        _, wd, dirs, gap2 = _world(name, seed)
        assert np.array_equal(dirs, ro.step_map_numpy(wd)), (name, seed)
        assert np.array_equal(dirs == ro.ROUTE_NONE, wd == wr.NONE) and (dirs == ro.ROUTE_SEED).sum() == 1 and dirs[seed] == ro.ROUTE_SEED
        # every wet non-seed cell has a dir, and the neighbour it names is wet and cheaper by exactly the step's cost
        for r, c in np.argwhere((wd != wr.NONE) & (wd != 0)):
            k = int(dirs[r, c])
            assert k < 8
            nb = (r + ro.OFFSETS[k][0], c + ro.OFFSETS[k][1])
            assert 0 <= nb[0] < rows and 0 <= nb[1] < cols and wd[nb] != wr.NONE and int(wd[nb]) + ro.COSTS[k] == int(wd[r, c]), (name, seed, r, c)
        pts = [((c + 0.5) * res, (r + 0.5) * res) for r in range(rows) for c in range(cols)]
        recs, verts = ro.routes(wd, gap2, res, pts, 0, 4, dirs=dirs)
        for (r, c), rec, vs in zip(np.ndindex(rows, cols), recs, verts):
            flags = ro.flags_of(rec)
            if wd[r, c] == wr.NONE:
                assert flags == ro.WR_DRY and rec["vertices"] == 0 and vs == [] and rec["point_cell"] == r * cols + c and rec["from_cell"] == wr.NONE
                assert np.isposinf(rec["metres"]) and np.isposinf(rec["narrowest_metres"]) and ro.code_of(rec) == 0xFF and rec["min_gap2"] == wr.NONE
                continue
            s, d = int(rec["straight_steps"]), int(rec["diagonal_steps"])
            assert 12 * s + 17 * d == rec["wd"] == wd[r, c]
            assert rec["metres"] <= res * float(rec["wd"]) / 12.0
            assert rec["vertices"] == len(vs) == (1 if (r, c) == seed else rec["turns"] + 2) and rec["vertices_written"] == min(len(vs), 4)
            assert bool(flags & ro.WR_TRUNCATED) == (len(vs) > 4) and bool(flags & ro.WR_AT_SEED) == ((r, c) == seed)
            assert vs[0] == seed[0] * cols + seed[1] and vs[-1] == r * cols + c
            # the vertex list expanded back into cells is the walk (consecutive vertices lie on one of the eight directions)
            cells, codes = ro.walk(dirs, (r, c))
            assert ro.expand(vs, cols) == cells[::-1], (name, seed, r, c)
            assert ro.code_of(rec) == (ro.OPPOSITE[codes[-1]] if codes else ro.ROUTE_SEED)
            gaps = [int(gap2[cell]) for cell in cells]
            assert rec["min_gap2"] == min(gaps) and rec["narrowest_metres"] == res * math.sqrt(min(gaps))
            where = divmod(int(rec["min_gap2_cell"]), cols)
            i = cells.index(where)
            assert gaps[i] == min(gaps) and all(v > min(gaps) for v in gaps[i + 1:])           # nearest the seed on a tie


def test_open_water_has_at_most_one_turn():
    g = np.zeros((9, 13), dtype=np.uint8)
    for seed in ((0, 0), (4, 6), (8, 12), (3, 11)):
        wd = wr.wd_dijkstra(g, seed)
        dirs = ro.step_map(wd)
        recs, verts = ro.routes(wd, np.zeros(g.shape, dtype=np.uint16), 1.0, [(c + 0.5, r + 0.5) for r in range(9) for c in range(13)], 0, 256, dirs=dirs)
        for (r, c), rec in zip(np.ndindex(9, 13), recs):
            dr, dc = abs(r - seed[0]), abs(c - seed[1])
            assert rec["turns"] <= 1 and rec["diagonal_steps"] == min(dr, dc) and rec["straight_steps"] == abs(dr - dc), (seed, r, c)


@pytest.mark.parametrize("name", ["rings", "perc59", "spiral", "comb"])
def test_approach_cell_attains_water_replays_approach(name):
    g = SMALL[name]()
    rows, cols = g.shape
    seed = _seeds(g)[0]
    _, wd, dirs, gap2 = _world(name, seed)
    rng = np.random.default_rng(11)
    for lim2 in (1, 2, 5, 10, 1024):
        for r, c in rng.integers(0, (rows, cols), size=(10, 2)):
            b = ro.approach_cell(wd, int(r), int(c), lim2)
            assert int(wd[b]) == wr.approach(wd, int(r), int(c), lim2), (name, lim2, r, c)
            rec, _ = ro.route(wd, dirs, gap2, 1.0, c + 0.5, r + 0.5, lim2, 8)
            assert int(rec["wd"]) == int(wd[b]) and (rec["from_cell"] == b[0] * cols + b[1] or wd[b] == wr.NONE)
            # the lowest row-major index among the cells of the window that attain it
            if wd[b] != wr.NONE:
                first = min(rr_ * cols + cc for rr_ in range(rows) for cc in range(cols)
                            if max(abs(rr_ - r) - 1, 0) ** 2 + max(abs(cc - c) - 1, 0) ** 2 < lim2 and wd[rr_, cc] == wd[b])
                assert rec["from_cell"] == first


def test_outside_and_states():
    g = SMALL["rings"]()
    _, wd, dirs, gap2 = _world("rings", _seeds(g)[0])
    rec, vs = ro.route(wd, dirs, gap2, 1.0, -0.5, 3.0, 5, 8)
    assert ro.flags_of(rec) == ro.WR_DRY | ro.WR_OUTSIDE and rec["point_cell"] == wr.NONE and vs == [] and rec["lim2"] == 5
    for kwargs, flag in (({"seed_flags": wr.WATER_SEED_BLOCKED}, ro.WR_NO_SEED), ({"no_map": True}, ro.WR_NO_MAP)):
        rec, vs = ro.route(wd, dirs, gap2, 1.0, 3.5, 3.5, 0, 8, **kwargs)
        assert ro.flags_of(rec) == flag and ro.code_of(rec) == 0xFF and rec["vertices"] == 0 and np.isposinf(rec["metres"]) and rec["from_cell"] == wr.NONE


def test_the_issues_figures():
    """The long walks: steps and turns of the route to the farthest cell from the first free cell."""
    for grid, steps, turns in ((rr.spiral(), 2520, 139), (rr.serpentine(), 4322, 129), (rr.spiral(31), 480, 59)):
        seed = tuple(int(v) for v in np.argwhere(grid == 0)[0])
        wd = wr.wd_dijkstra(grid, seed)
        far = divmod(wr.totals(wd)[2], grid.shape[1])
        rec, vs = ro.route(wd, ro.step_map_numpy(wd), np.zeros(grid.shape, dtype=np.uint16), 1.0, far[1] + 0.5, far[0] + 0.5, 0, 256)
        assert (int(rec["straight_steps"]) + int(rec["diagonal_steps"]), int(rec["turns"])) == (steps, turns)
        assert 12 * int(rec["straight_steps"]) + 17 * int(rec["diagonal_steps"]) == int(rec["wd"]) and len(vs) == turns + 2


def test_detour_world_route_passes_the_strait():
    w, init, calls, gap2 = wr.detour_world()
    recs, verts, keys, lines = ro.plan_routes(w, gap2, 0)
    cols = w.grid.shape[1]
    assert recs["wd"][1] == 751 and recs["metres"][1] <= 751.0 / 12.0
    cells = ro.expand(verts[1], cols)
    crossing = [c for r, c in cells if r == rr.PLAN_WALL_ROW]
    assert crossing and all(wr.DETOUR_STRAIT[0] <= c < wr.DETOUR_STRAIT[1] for c in crossing)
    assert recs["min_gap2"][1] == 0                       # the strait's cells touch the wall
    # the nearest ribbon by water is the one the start lies on: its route is the seed's cell alone
    assert keys == {"water_route_metres": 0.0, "water_route_turns": 0, "water_route_vertices": 1, "water_route_truncated": False,
                    "water_route_narrowest_metres": keys["water_route_narrowest_metres"], "water_route_first_dir": 8}
    assert len(lines) == sum(len(v) for v in verts) and lines[0][:2] == (0, 0)
    # at limit2 9 the strait is closed: ribbon 1 is dry, and every route stays in the inflated grid
    recs9, verts9, _, _ = ro.plan_routes(w, gap2, 9)
    assert ro.flags_of(recs9[1]) == ro.WR_DRY and verts9[1] == []
    assert all(r["min_gap2"] >= 9 for r in recs9 if not ro.flags_of(r) & ro.WR_DRY)
