"""The chart-clearance entry points exist at every layer that needs no GPU — declared in include/ppgpu.h with the layout of their numpy
mirror, exported by libppgpu.so, bound in path_planner_amd.api — and the definitions the GPU tests compare the device against
(tests/clearance_replay.py) pin themselves: the separable passes on the cell-by-cell definition, the definition on the plain
Euclidean transform of the dilated hazard set and on random point pairs, the margin's integer limit, the merge rules, the far world
on the oracle."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import clearance_replay as clr
import grid_worlds as gw
from test_contact_trace_abi import _header, _struct_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ppgpu_get_grid_distance", "ppgpu_grid_clearance_at", "ppgpu_last_grid_distance_timing", "ppgpu_trace_clearance_list",
           "ppgpu_trace_clearance_host", "ppgpu_trace_clearance_wrapper_edges_host", "ppgpu_last_clearance_trace_timing"]
METHODS = ["get_grid_distance", "grid_clearance_at", "last_grid_distance_timing", "trace_clearance", "trace_clearance_wrapper_edges",
           "trace_clearance_list", "last_clearance_trace_timing"]


def test_header_layout_equals_the_numpy_mirror():
    from path_planner_amd import types as T
    txt = _header()
    for name in SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(\s*ppgpu_ctx\s*\*" % name, txt, flags=re.M), name
    fields, size = _struct_layout(txt, "ppgpu_clearance_record")
    D = T.CLEARANCE_DTYPE
    assert size == D.itemsize == 64 and size % 16 == 0
    assert [(n, D.fields[n][0].str, D.fields[n][1]) for n in D.names] == fields
    defines = dict(re.findall(r"#define\s+(PPGPU_(?:CL|DIST)_\w+)\s+(\w+)", txt))
    assert int(defines["PPGPU_DIST_CAP"]) == T.DIST_CAP == 255 and int(defines["PPGPU_DIST_CAP2"]) == T.DIST_CAP2 == 255 * 255
    for name in ("EMPTY", "BLOCKED", "CAPPED", "NO_MAP"):
        assert int(defines["PPGPU_CL_" + name].rstrip("u"), 16) == getattr(T, "CL_" + name), name
    full = open(os.path.join(ROOT, "include", "ppgpu.h")).read()
    for cite in ("GridWorldMap.cpp:84-93", "Edge.cpp:144"):
        assert cite in full[full.index("chart clearance"):], cite


def test_library_exports_and_binding_has_them():
    from path_planner_amd import api
    lib = C.CDLL(api.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS
        assert getattr(api.LIB, name).restype is C.c_int
    for method in METHODS:
        assert callable(getattr(api.Context, method)), method


# ------------------------------------------------------------------------------------------------------------ the map's definition
def _random_grid(rows, cols, seed):
    return (np.random.default_rng(seed).uniform(size=(rows, cols)) < 0.05).astype(np.uint8)


def _corner():
    g = np.zeros((9, 13), dtype=np.uint8)
    g[0, 0] = 1
    return g


GRIDS = {
    "tiny5x7": lambda: gw.tiny("5x7").grid, "tiny1x40": lambda: gw.tiny("1x40").grid, "tiny40x1": lambda: gw.tiny("40x1").grid,
    "1x1free": lambda: np.zeros((1, 1), dtype=np.uint8), "1x1blocked": lambda: np.ones((1, 1), dtype=np.uint8),
    "1xN": lambda: _random_grid(1, 29, 3), "Nx1": lambda: _random_grid(29, 1, 4),
    "all_blocked": lambda: np.ones((6, 11), dtype=np.uint8), "corner": _corner,
    "walls": gw.walls_grid, "wide": lambda: gw.wide().grid,
    "random33x70": lambda: _random_grid(33, 70, 1), "random64x31": lambda: _random_grid(64, 31, 2),
}
_MAPS = {}


def _maps(name):
    """(grid, gap2_brute, gap2_numpy) of a named grid, computed once per process."""
    if name not in _MAPS:
        g = GRIDS[name]()
        _MAPS[name] = (g, clr.gap2_brute(g), clr.gap2_numpy(g))
        for a in _MAPS[name]:
            a.setflags(write=False)
    return _MAPS[name]


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_separable_passes_equal_the_definition(name):
    g, brute, sep = _maps(name)
    assert sep.dtype == np.uint16 and sep.shape == g.shape
    assert np.array_equal(sep, brute), np.argwhere(sep != brute)[:5]
    # 0 on a blocked cell and on its eight neighbours, and on the border cells (the outside is a hazard)
    b = np.pad(g != 0, 1, constant_values=True)
    near = np.zeros(g.shape, dtype=bool)
    for dr in (0, 1, 2):
        for dc in (0, 1, 2):
            near |= b[dr:dr + g.shape[0], dc:dc + g.shape[1]]
    assert np.array_equal(brute == 0, near)


def test_empty_grid_is_the_distance_to_the_nearest_side():
    rows, cols = 23, 40
    r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    want = np.minimum(np.minimum(r, rows - 1 - r), np.minimum(c, cols - 1 - c)) ** 2
    assert np.array_equal(clr.gap2_numpy(np.zeros((rows, cols), dtype=np.uint8)), want)
    far = clr.gap2_numpy(np.zeros((clr.FAR_N, clr.FAR_N), dtype=np.uint8))
    assert far.max() == clr.DIST_CAP2 and far[clr.FAR_N // 2, clr.FAR_N // 2] == clr.DIST_CAP2 and far[254, 350] == 254 * 254


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_definition_is_the_euclidean_transform_of_the_dilated_hazards(name):
    """gap2 = the plain squared Euclidean distance (between cell centres) to the hazard set dilated by one cell.  One ring of outside
    cells stands for the whole outside: any outside cell farther out has one of the ring nearer to every cell of the grid."""
    g, brute, _ = _maps(name)
    rows, cols = g.shape
    hz = np.pad(g != 0, 2, constant_values=True)                     # the grid, one ring of outside, one ring for the dilation to fall in
    dil = np.zeros_like(hz)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            dil |= np.roll(np.roll(hz, dr, axis=0), dc, axis=1)
    dr_, dc_ = np.nonzero(dil)
    dr_, dc_ = dr_ - 2, dc_ - 2                                      # in the grid's own coordinates
    for r in range(rows):
        d2 = (dr_[None, :] - r) ** 2 + (dc_[None, :] - np.arange(cols)[:, None]) ** 2
        assert np.array_equal(np.minimum(d2.min(axis=1), clr.DIST_CAP2), brute[r].astype(np.int64)), (name, r)


@pytest.mark.parametrize("name,res", [("wide", 1.0), ("tiny5x7", 4.0), ("random33x70", 1.0 / 3.0), ("random64x31", 0.07)])
def test_clearance_is_a_certified_lower_bound(name, res):
    """20 000 random pairs (a point of a free cell, a point of a hazard cell, blocked or outside): never nearer than
    res * sqrt(gap2) of the free point's cell.  And for every free cell some hazard cell comes within res * (sqrt(gap2) + sqrt 2)."""
    g, brute, _ = _maps(name)
    rows, cols = g.shape
    rng = np.random.default_rng(17)
    fr, fc = np.nonzero(g == 0)
    hz = np.pad(g != 0, 3, constant_values=True)                     # hazard cells: the blocked ones and three rings of the outside
    hr, hc = np.nonzero(hz)
    hr, hc = hr - 3, hc - 3
    n = 20000
    i, j = rng.integers(0, len(fr), n), rng.integers(0, len(hr), n)
    px, py = (fc[i] + rng.uniform(0, 1, n)) * res, (fr[i] + rng.uniform(0, 1, n)) * res
    qx, qy = (hc[j] + rng.uniform(0, 1, n)) * res, (hr[j] + rng.uniform(0, 1, n)) * res
    bound = res * np.sqrt(brute[fr[i], fc[i]].astype(np.float64))
    dist = np.hypot(px - qx, py - qy)
    assert np.all(dist >= bound * (1 - 1e-12)), float((dist - bound).min())
    # ... and it is tight to a cell's diagonal: from the centre and the four corners of every free cell, the nearest point of some
    # hazard cell is no farther than sqrt(gap2) + sqrt 2 cells (in cells; these grids stay below the cap)
    assert brute.max() < clr.DIST_CAP2
    for ox, oy in ((0.5, 0.5), (0, 0), (0, 1), (1, 0), (1, 1)):
        for k in range(0, len(fr), 2048):
            r, c = fr[k:k + 2048], fc[k:k + 2048]
            px, py = (c + ox)[:, None], (r + oy)[:, None]
            dx = np.maximum(np.maximum(hc[None, :] - px, px - (hc[None, :] + 1)), 0)
            dy = np.maximum(np.maximum(hr[None, :] - py, py - (hr[None, :] + 1)), 0)
            true = np.sqrt((dx * dx + dy * dy).min(axis=1))
            bound = np.sqrt(brute[r, c].astype(np.float64))
            assert np.all(true >= bound - 1e-12) and np.all(true <= bound + math.sqrt(2.0) + 1e-12), (ox, oy, k)


# ------------------------------------------------------------------------------------------------------------ margin and merge
@pytest.mark.parametrize("res", [1.0, 0.25, 1.0 / 3.0, 0.3, 0.07, 0.05])
def test_limit2_is_the_smallest_k_that_reaches_the_margin(res):
    assert clr.limit2(res, 0.0) == 0 and clr.limit2(res, -1.0) == 0
    assert clr.limit2(res, 1e-300) == 1                               # any positive margin: the cells that touch a hazard are below
    for k in (1, 2, 3, 4, 5, 8, 9, 10, 17, 100, 101, 4096, 65024, 65025):
        m = res * math.sqrt(float(k))
        assert clr.limit2(res, m) <= k                                # a margin of exactly res * sqrt(k): gap2 == k is not below
        up = float(np.nextafter(m, np.inf))
        if k < clr.DIST_CAP2:
            assert clr.limit2(res, up) > k                            # one ulp above: it is
        lim = clr.limit2(res, m)
        assert res * math.sqrt(float(lim)) >= m and (lim == 0 or res * math.sqrt(float(lim - 1)) < m)
    assert clr.limit2(res, clr.DIST_CAP * res) <= clr.DIST_CAP2
    with pytest.raises(ValueError):
        clr.limit2(res, clr.DIST_CAP * res * (1 + 1e-9))


def _rec(clearance, step, below=0, first_below=-1, first_time=-1.0, flags=0, gap2=0, time=0.0):
    r = clr.empty_record()
    r["clearance"], r["step"], r["below_steps"], r["first_below_step"], r["first_below_time"] = clearance, step, below, first_below, first_time
    r["flags"], r["gap2"], r["time"], r["x"], r["y"] = flags, gap2, time, 10.0 + step, 20.0 + step
    return r


def test_merge_follows_its_rules():
    from path_planner_amd.types import CL_EMPTY, CL_BLOCKED, CL_CAPPED
    e = clr.empty_record()
    assert e["flags"] == CL_EMPTY and e["clearance"] == -1 and e["time"] == -1 and e["step"] == -1 and e["first_below_step"] == -1
    assert e["first_below_time"] == -1 and e["below_steps"] == 0 and e["gap2"] == 0 and e["x"] == 0 and e["y"] == 0
    m, seg = clr.merge([])
    assert m.tobytes() == e.tobytes() and seg == -1
    m, seg = clr.merge([e, e])
    assert m.tobytes() == e.tobytes() and seg == -1
    a = _rec(3.0, 5, below=2, first_below=4, first_time=107.0, gap2=9, time=105.0, flags=CL_CAPPED)
    b = _rec(2.0, 7, below=3, first_below=1, first_time=101.0, gap2=4, time=111.0)
    c = _rec(2.0, 1, gap2=4, time=120.0, flags=CL_BLOCKED)
    m, seg = clr.merge([a, e, b, c])
    assert seg == 2 and m["clearance"] == 2.0 and m["step"] == 7 and m["time"] == 111.0 and m["gap2"] == 4        # the earlier of equal minima
    assert (m["x"], m["y"]) == (17.0, 27.0)
    assert m["below_steps"] == 5 and m["first_below_time"] == 101.0 and m["first_below_step"] == 1
    assert m["flags"] == CL_CAPPED | CL_BLOCKED                       # ORed; EMPTY only when every segment is empty
    m, seg = clr.merge([e, a])
    assert seg == 1 and m["flags"] == CL_CAPPED and m["clearance"] == 3.0 and m["first_below_time"] == 107.0


# ------------------------------------------------------------------------------------------------------------ replay and the far world
def test_replay_takes_the_earliest_of_equal_minima_and_counts_below():
    from path_planner_amd.types import STEP_DTYPE, CL_BLOCKED, CL_CAPPED, CL_NO_MAP, CL_EMPTY, S_BLOCKED
    g = np.zeros((20, 20), dtype=np.uint8)
    g[10, 15] = 1
    res = 0.5
    s = np.zeros(8, dtype=STEP_DTYPE)
    s["y"] = 10.5 * res
    s["x"] = (np.array([8, 9, 10, 11, 12, 13, 14, 15]) + 0.5) * res       # eastwards along row 10 onto the blocked cell
    s["time"] = 100.0 + np.arange(8)
    s["flags"][-1] = S_BLOCKED
    r = clr.replay(g, res, s, 1.0)                                    # limit2 = 4: gap2 < 4 is below
    assert clr.limit2(res, 1.0) == 4
    assert r["gap2"] == 0 and r["step"] == 6 and r["time"] == 106.0 and r["clearance"] == 0.0      # column 14 touches the hazard first
    assert r["below_steps"] == 3 and r["first_below_step"] == 5 and r["first_below_time"] == 105.0   # columns 13 (one cell between: gap2 1) .. 15
    assert r["flags"] == CL_BLOCKED
    r = clr.replay(g, res, s[:3], 0.0)
    assert r["gap2"] == 16 and r["step"] == 2 and r["below_steps"] == 0 and r["first_below_step"] == -1 and r["flags"] == 0
    assert r["clearance"] == res * 4.0
    r = clr.replay(None, 0.0, s[:7], 5.0)                             # (the base Map blocks nothing: the steps before the blocked one)
    assert r["flags"] == CL_NO_MAP | CL_CAPPED and r["clearance"] == clr.DBL_MAX and r["gap2"] == clr.DIST_CAP2 and r["step"] == 0
    assert clr.replay(g, res, s[:0], 1.0).tobytes() == clr.empty_record().tobytes()
    out = s.copy()
    out["x"][3] = -0.25                                               # a pose outside the grid: gap2 0
    r = clr.replay(g, res, out[:5], 0.0)
    assert r["gap2"] == 0 and r["step"] == 3 and CL_EMPTY & r["flags"] == 0


def test_far_world_is_what_it_claims_to_be():
    from path_planner_amd.types import F_THROWS
    w = clr.far_world()
    rec, _ = w.oracle_cost()
    assert not np.any(rec["flags"] & F_THROWS)
    counts = (rec["info"] >> 16).astype(int)
    assert list(counts) == list(clr.FAR_CENTRAL) + [clr.FAR_OUTWARD]
    gap2 = clr.gap2_numpy(w.grid)
    for e in w.central:
        p = clr.oracle_poses(w, rec, e)
        assert np.all(clr.step_gap2(gap2, w.res, p[:, 0], p[:, 1]) >= clr.DIST_CAP2), e
    p = clr.oracle_poses(w, rec, w.outward)
    g2 = clr.step_gap2(gap2, w.res, p[:, 0], p[:, 1])
    assert g2[0] == clr.DIST_CAP2 and g2.min() < clr.DIST_CAP2 and g2.min() > 0
