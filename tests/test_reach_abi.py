"""The reachable-water entry points exist at every layer that needs no GPU — declared in include/ppgpu.h with the layout of their
numpy mirrors, exported by libppgpu.so, bound in path_planner_amd.api — and the definitions the GPU tests compare the device against
(tests/reach_replay.py) pin themselves: the run union-find on the flood fill (and on scipy where it is installed), the padded
distance transform on the cell-by-cell reach gap, the ribbon record on a brute-force walk, and the planning world of
tests/test_gpu_plan_reach.py on numpy and on the oracle."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import clearance_replay as clr
import grid_worlds as gw
import reach_replay as rr
from test_contact_trace_abi import _header, _struct_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ppgpu_get_grid_labels", "ppgpu_set_reach_seed", "ppgpu_get_grid_reach_gap", "ppgpu_ribbon_reach_host", "ppgpu_last_reach_timing"]
METHODS = ["get_grid_labels", "set_reach_seed", "get_grid_reach_gap", "ribbon_reach", "last_reach_timing"]
C_TYPES = {"uint64_t": ("<u8", 8)}


def test_header_layout_equals_the_numpy_mirrors(monkeypatch):
    import test_contact_trace_abi as base
    from path_planner_amd import types as T
    monkeypatch.setattr(base, "C_TYPES", dict(base.C_TYPES, **C_TYPES))
    txt = _header()
    for name in SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(\s*ppgpu_ctx\s*\*" % name, txt, flags=re.M), name
    # (the info block is the typedef the ABI states: two 64-bit counts and four 32-bit words, 32 bytes)
    for struct, D, size in (("ppgpu_reach_info", T.REACH_INFO_DTYPE, 32), ("ppgpu_ribbon_reach_record", T.RIBBON_REACH_DTYPE, 64)):
        fields, got = _struct_layout(txt, struct)
        assert got == D.itemsize == size and size % 16 == 0
        assert [(n, D.fields[n][0].str, D.fields[n][1]) for n in D.names] == fields
    defines = dict(re.findall(r"#define\s+(PPGPU_(?:REACH|RB)_\w+)\s+(\w+)", txt))
    assert int(defines["PPGPU_REACH_NONE"].rstrip("u"), 16) == T.REACH_NONE == 0xFFFFFFFF
    assert int(defines["PPGPU_REACH_TILE"]) == T.REACH_TILE == rr.T
    for name in ("SEED_BLOCKED", "NO_MAP"):
        assert int(defines["PPGPU_REACH_" + name].rstrip("u"), 16) == getattr(T, "REACH_" + name), name
    for name in ("ANY_OUT", "WHOLE_OUT", "START_OUT", "END_OUT", "DEGENERATE", "CAPPED", "NO_SEED", "NO_MAP"):
        assert int(defines["PPGPU_RB_" + name].rstrip("u"), 16) == getattr(T, "RB_" + name), name
    full = open(os.path.join(ROOT, "include", "ppgpu.h")).read()
    section = full[full.index("reachable water"):]
    for cite in ("Edge.cpp:114,173", "Edge.cpp:144-147", "Ribbon.cpp:39-43", "GridWorldMap.cpp:84-93", "proves nothing"):
        assert cite in section, cite
    kernels = open(os.path.join(ROOT, "path_planner_amd", "csrc", "pp_k_reach.h")).read()
    assert "PP_REACH_TILE PPGPU_REACH_TILE" in kernels


def test_library_exports_and_binding_has_them():
    from path_planner_amd import api
    lib = C.CDLL(api.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS
        assert getattr(api.LIB, name).restype is C.c_int
    for method in METHODS:
        assert callable(getattr(api.Context, method)), method


# ------------------------------------------------------------------------------------------------------------ the replay's labels
SMALL = {
    "tiny5x7": lambda: gw.tiny("5x7").grid, "tiny1x40": lambda: gw.tiny("1x40").grid, "tiny40x1": lambda: gw.tiny("40x1").grid,
    "1x1free": lambda: np.zeros((1, 1), dtype=np.uint8), "1x1blocked": lambda: np.ones((1, 1), dtype=np.uint8),
    "open": lambda: np.zeros((9, 13), dtype=np.uint8), "all_blocked": lambda: np.ones((6, 11), dtype=np.uint8),
    "checkerboard": lambda: rr.checkerboard(33, 40), "diagonal": lambda: rr.diagonal_channel(37), "antidiagonal": lambda: rr.diagonal_channel(37, anti=True),
    "rings": lambda: rr.nested_rings(39)[:39, :39], "comb": lambda: rr.comb(40, 37), "isolated": lambda: rr.isolated(21, 24),
    "serpentine": lambda: rr.serpentine(38, 29), "spiral": lambda: rr.spiral(31),
    "perc59": lambda: rr.percolation(40, 40, 0.59, 1), "perc55": lambda: rr.percolation(33, 40, 0.55, 2), "perc30": lambda: rr.percolation(40, 29, 0.3, 3),
}
LARGE = {
    "checkerboard": lambda: rr.checkerboard(33, 65), "rings": rr.nested_rings, "comb": rr.comb, "serpentine": rr.serpentine, "spiral": rr.spiral,
    "perc300": lambda: rr.percolation(300, 300, 0.59, 1), "perc257x513": lambda: rr.percolation(257, 513, 0.55, 2), "walls": gw.walls_grid,
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_run_union_find_equals_the_flood_fill(name):
    g = SMALL[name]()
    assert g.shape[0] <= 40 and g.shape[1] <= 40
    got, want = rr.labels_numpy(g), rr.labels_brute(g)
    assert got.dtype == np.uint32 and np.array_equal(got, want), np.argwhere(got != want)[:5]
    free = g == 0
    assert np.array_equal(got != rr.REACH_NONE, free)
    # canonical: a label is the index of a cell that carries it, and no cell of the component comes before it
    idx = np.arange(g.size, dtype=np.uint32).reshape(g.shape)
    assert (got[free] <= idx[free]).all()
    for lab in np.unique(got[free]):
        assert got.ravel()[lab] == lab


def test_the_directed_grids_are_what_they_claim():
    tot = lambda g, k=8: rr.totals(rr.labels_brute(g, connectivity=k))
    assert tot(rr.checkerboard(33, 65)) == (1073, 1, 1073) and tot(rr.checkerboard(33, 65), 4)[1] == 1073
    assert tot(rr.diagonal_channel(37)) == (37, 1, 37) and tot(rr.diagonal_channel(37), 4)[1] == 37
    assert rr.totals(rr.labels_numpy(rr.nested_rings()))[1] == 3
    comb = rr.comb()
    assert rr.totals(rr.labels_numpy(comb))[1] == 1 and rr.totals(rr.labels_numpy(comb[:-1]))[1] > 20       # the teeth join along the last row only
    iso = rr.totals(rr.labels_numpy(rr.isolated()))
    assert iso[0] == iso[1] > 1000 and iso[2] == 1
    assert rr.totals(rr.labels_numpy(rr.serpentine())) == (8710, 1, 8710)
    assert rr.totals(rr.labels_numpy(rr.spiral()))[1] == 1 and tot(rr.spiral(31), 4)[1] == 1
    assert rr.totals(rr.labels_numpy(rr.percolation(300, 300, 0.59, 1)))[1:] == (1341, 8211)
    assert rr.totals(rr.labels_numpy(rr.percolation(257, 513, 0.55, 2)))[1:] == (1009, 56094)


@pytest.mark.parametrize("name", sorted(LARGE))
def test_run_union_find_equals_scipy(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    g = LARGE[name]()
    lab, n = ndimage.label(g == 0, structure=np.ones((3, 3), dtype=int))
    got = rr.labels_numpy(g)
    assert rr.totals(got)[1] == n
    # scipy numbers the components in row-major order of their first cells: the canonical label of component k is that cell's index
    first = np.full(n + 1, rr.REACH_NONE, dtype=np.uint32)
    flat = lab.ravel()
    seen = np.unique(flat, return_index=True)
    first[seen[0]] = seen[1]
    first[0] = rr.REACH_NONE
    assert np.array_equal(got, first[lab])


# ------------------------------------------------------------------------------------------------------------ the reach gap
@pytest.mark.parametrize("name", ["perc59", "rings", "tiny5x7", "serpentine", "all_blocked"])
def test_padded_transform_equals_the_reach_gap_cell_by_cell(name):
    g = SMALL[name]()
    labels = rr.labels_numpy(g)
    seen = 0
    for lab in list(np.unique(labels[labels != rr.REACH_NONE]))[:3] + [rr.REACH_NONE]:
        reach = rr.reach_set(labels, int(lab))
        got = rr.rgap2_numpy(reach)
        assert got.dtype == np.uint16 and np.array_equal(got, rr.rgap2_brute(reach)), (name, lab)
        if lab == rr.REACH_NONE:
            assert (got == clr.DIST_CAP2).all()          # no source at all: the cap everywhere (the outside is none either)
        else:
            near = np.zeros(g.shape, dtype=bool)         # gap 0: the set and the cells beside it
            pad = np.pad(reach, 1)
            for dr in (0, 1, 2):
                for dc in (0, 1, 2):
                    near |= pad[dr:dr + g.shape[0], dc:dc + g.shape[1]]
            assert np.array_equal(got == 0, near)
            seen += 1
    assert seen or name == "all_blocked"


def test_seed_cell_is_the_map_lookup():
    assert rr.seed_cell((5, 7), 0.5, 3.49, 2.49) == (4, 6) and rr.seed_cell((5, 7), 0.5, 3.5, 1.0) is None
    assert rr.seed_cell((5, 7), 0.5, -1e-9, 1.0) is None and rr.seed_cell((5, 7), 0.5, 1.0, 2.5) is None and rr.seed_cell((5, 7), 0.5, 0.0, 0.0) == (0, 0)


# ------------------------------------------------------------------------------------------------------------ ribbon records
def _record_by_hand(rgap2, res, ribbon, width):
    """The header's words, sample by sample in plain Python floats."""
    sx, sy, ex, ey = ribbon
    dx, dy = ex - sx, ey - sy
    length = math.sqrt(dx * dx + dy * dy)
    n = max(1, math.ceil(length / (0.5 * res)))
    lim2 = clr.limit2(res, width + 0.25 * res)
    rows, cols = rgap2.shape
    out = []
    for k in range(1 if length == 0 else n + 1):
        x, y = sx + dx * (k / n), sy + dy * (k / n)
        x, y = min(max(x, 0.0), cols * res), min(max(y, 0.0), rows * res)
        out.append(int(rgap2[min(int(y / res), rows - 1), min(int(x / res), cols - 1)]) >= lim2)
    return length, n, out


@pytest.mark.parametrize("res", [1.0, 1.0 / 3.0, 0.07])
def test_ribbon_record_follows_the_definition(res):
    import test_gpu_reach_ribbons as tr
    grid = tr._ribbon_grid()
    labels = rr.labels_numpy(grid)
    rgap2 = rr.rgap2_numpy(rr.reach_set(labels, 0))
    width = tr.WIDTH_CELLS * res
    for ribbon in tr.RIBBONS * res:
        rec = rr.ribbon_record(rgap2, res, ribbon, width)
        length, n, out = _record_by_hand(rgap2, res, [float(v) for v in ribbon], width)
        assert rec["length"] == length and rec["samples"] == len(out) and rec["out_samples"] == sum(out) and rec["lim2"] == 4
        assert rec["pitch"] == (0.0 if length == 0 else length / n) and rec["pitch"] <= 0.5 * res
        assert rec["first_out"] == (out.index(True) if any(out) else -1) and rec["last_out"] == (len(out) - 1 - out[::-1].index(True) if any(out) else -1)
        assert bool(rec["flags"] & rr.RB_ANY_OUT) == any(out) and bool(rec["flags"] & rr.RB_WHOLE_OUT) == all(out)
        assert bool(rec["flags"] & rr.RB_START_OUT) == out[0] and bool(rec["flags"] & rr.RB_END_OUT) == out[-1]
        assert rec["out_length"] == min(rec["pitch"] * sum(out), length) and rec["reserved"] == 0


# ------------------------------------------------------------------------------------------------------------ the planning world
def test_planning_world_on_numpy():
    w, init, calls, gap2 = rr.plan_world()
    assert w.grid.shape == (37, 83) and w.res == 1.0 and w.cfg.ribbon_width == 1.5 and rr.ribbon_lim2(w.res, w.cfg.ribbon_width) == 4
    assert w.cfg.collision_checking_increment <= w.res                       # Certified
    assert w.grid[rr.PLAN_WALL_ROW].sum() == 83 - 5 and not w.grid[rr.PLAN_WALL_ROW, 40:45].any()
    for margin, limit2 in rr.PLAN_MARGINS.items():
        assert clr.limit2(w.res, margin) == limit2
        labels, label, (free, comps), recs = rr.plan_reach(w, gap2, limit2)
        if limit2 < 9:
            assert comps == 1 and not recs["out_samples"].any() and not recs["flags"].any()
            continue
        assert (free, comps, int((labels == label).sum()), label) == (1480, 4, 1297, 259)
        assert [(int(r["samples"]), int(r["out_samples"])) for r in recs] == [(51, 0), (51, 51), (29, 17)]
        assert recs["min_rgap2"][1] == recs["max_rgap2"][1] == 49
        assert (recs["first_out"][2], recs["last_out"][2]) == (12, 28)
        assert recs["flags"][2] == rr.RB_ANY_OUT | rr.RB_END_OUT and recs["flags"][0] == 0
        # ribbon 0 lies inside the band (its own cells are blocked at this margin) and is still coverable from row 23
        eff = (gap2 < 9) | (w.grid != 0)
        assert eff[24, 30:56].any() and recs["max_rgap2"][0] < 4


def test_planning_world_on_the_oracle():
    """With the strait closed (the grid inflated at limit2 9) the reference's planner finds no goal: ribbon 1 cannot be covered.  On
    the grid as set it does."""
    import oracle as orc
    w, init, calls, gap2 = rr.plan_world()
    orc.O.ppo_set_ribbon_width(w.cfg.ribbon_width)
    plans = {}
    for limit2 in (0, 9):
        grid = ((gap2 < limit2) | (w.grid != 0)).astype(np.uint8)
        rc, st, plan, _, _ = orc.World(w.cfg, grid, w.res, w.obst).plan(w.ribbons4, w.start5, calls * 1e-3, 1000.0, 1e-3, initial_samples=init)
        assert rc == 0
        plans[limit2] = (st, plan)
    assert plans[0][0].first_goal_iteration >= 0 and len(plans[0][1]) >= 1
    assert plans[9][0].first_goal_iteration < 0 and len(plans[9][1]) == 0
