"""The definitions the device's route-by-water reports are compared against (include/ppgpu.h, "route by water"): the step map of a water
map (ppgpu_get_grid_water_dirs -> pp_k_water_dirs), the approach cell of a query point, the walk from it to the seed, and the record
and vertex list of a route (ppgpu_water_routes_host -> pp_k_water_routes), with plan_cli's keys.

A plain module, numpy only: no fixtures, no device.  Nothing here is clever: a loop over the cells and codes, a window scan, a walk
cell by cell.  It builds on water_replay.wd_dijkstra.  Everything is integer arithmetic except the two metres fields."""
import math

import numpy as np

import clearance_replay as clr
import reach_replay as rr
import water_replay as wr
from path_planner_amd.types import (WATER_NONE, WATER_STEP, WATER_DIAG, WATER_MAX_LIM2, WATER_ROUTE_DTYPE, ROUTE_NONE, ROUTE_SEED, WR_DRY, WR_OUTSIDE,
                                    WR_AT_SEED, WR_TRUNCATED, WR_NO_SEED, WR_NO_MAP)

NONE = WATER_NONE
# codes 0 .. 7: N, S, W, E, NW, NE, SW, SE, the order of `steps` in water_replay.wd_dijkstra
OFFSETS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))
COSTS = (WATER_STEP,) * 4 + (WATER_DIAG,) * 4
OPPOSITE = (1, 0, 3, 2, 7, 6, 5, 4)
VERTEX_STRIDE = 256               # what the host planner asks for


# ------------------------------------------------------------------------------------------------------------ the step map
def step_map(wd):
    """dir per cell: ROUTE_NONE where wd is NONE, ROUTE_SEED where it is 0 (the seed's cell), otherwise the lowest code whose neighbour
    lies in the grid, has a distance and is nearer by exactly the step's cost."""
    rows, cols = wd.shape
    out = np.full((rows, cols), ROUTE_NONE, dtype=np.uint8)
    for r in range(rows):
        for c in range(cols):
            v = int(wd[r, c])
            if v == NONE:
                continue
            if v == 0:
                out[r, c] = ROUTE_SEED
                continue
            for k, ((dr, dc), cost) in enumerate(zip(OFFSETS, COSTS)):
                nr, nc = r + dr, c + dc
                if 0 <= nr < rows and 0 <= nc < cols and int(wd[nr, nc]) != NONE and int(wd[nr, nc]) + cost == v:
                    out[r, c] = k
                    break
            else:
                raise AssertionError("wd is not a fixed point at (%d, %d)" % (r, c))
    return out


def step_map_numpy(wd):
    """The same bytes by whole-grid shifts (for the grids a Python loop over the cells is too slow for)."""
    rows, cols = wd.shape
    pad = np.full((rows + 2, cols + 2), np.int64(NONE), dtype=np.int64)
    pad[1:-1, 1:-1] = wd
    v = pad[1:-1, 1:-1]
    out = np.full((rows, cols), ROUTE_NONE, dtype=np.uint8)
    for k in range(7, -1, -1):                        # downwards: the lowest code is written last
        dr, dc = OFFSETS[k]
        nb = pad[1 + dr:1 + dr + rows, 1 + dc:1 + dc + cols]
        out[(v != NONE) & (nb != NONE) & (nb + COSTS[k] == v)] = k
    out[v == 0] = ROUTE_SEED
    assert not ((v != NONE) & (out == ROUTE_NONE)).any()
    return out


# ------------------------------------------------------------------------------------------------------------ the approach cell
def approach_cell(wd, r, c, lim2):
    """B for A = (r, c): A itself with lim2 0; otherwise the cell with gap2(A, B) < lim2 of the smallest wd, the lowest row-major index
    on a tie (the window is scanned in row-major order and only a smaller wd replaces the best).  -> (row, col), whatever its wd."""
    assert lim2 <= WATER_MAX_LIM2
    if lim2 == 0:
        return r, c
    rows, cols = wd.shape
    best, where = None, None
    reach = 34
    for rr_ in range(max(r - reach, 0), min(r + reach, rows - 1) + 1):
        for cc in range(max(c - reach, 0), min(c + reach, cols - 1) + 1):
            if max(abs(rr_ - r) - 1, 0) ** 2 + max(abs(cc - c) - 1, 0) ** 2 < lim2 and (best is None or int(wd[rr_, cc]) < best):
                best, where = int(wd[rr_, cc]), (rr_, cc)
    return where


# ------------------------------------------------------------------------------------------------------------ the walk
def walk(dirs, cell):
    """(cells, codes): the cells from `cell` to the seed's cell, both included, and the code of every step."""
    cells, codes = [cell], []
    r, c = cell
    for _ in range(dirs.size + 1):
        k = int(dirs[r, c])
        if k == ROUTE_SEED:
            return cells, codes
        assert k < 8, (r, c, k)
        r, c = r + OFFSETS[k][0], c + OFFSETS[k][1]
        assert 0 <= r < dirs.shape[0] and 0 <= c < dirs.shape[1]
        cells.append((r, c))
        codes.append(k)
    raise AssertionError("the walk does not end")


def expand(vertices, cols):
    """The cells of the polyline through `vertices` (row-major indices, seed first), every cell once: consecutive vertices must lie on
    one of the eight directions."""
    pts = [divmod(int(v), cols) for v in vertices]
    out = [pts[0]]
    for (r0, c0), (r1, c1) in zip(pts, pts[1:]):
        dr, dc = r1 - r0, c1 - c0
        n = max(abs(dr), abs(dc))
        assert n > 0 and (dr == 0 or dc == 0 or abs(dr) == abs(dc)), ((r0, c0), (r1, c1))
        out += [(r0 + (dr // n) * i, c0 + (dc // n) * i) for i in range(1, n + 1)]
    return out


# ------------------------------------------------------------------------------------------------------------ records
def _blank(lim2, flags):
    rec = np.zeros((), dtype=WATER_ROUTE_DTYPE)
    rec["point_cell"] = rec["from_cell"] = rec["wd"] = rec["min_gap2"] = rec["min_gap2_cell"] = NONE
    rec["lim2"] = lim2
    rec["first_dir"] = ROUTE_NONE | (flags << 8)
    rec["metres"] = rec["narrowest_metres"] = np.inf
    return rec


def route(wd, dirs, gap2, res, x, y, lim2, stride, seed_flags=0, no_map=False):
    """(record, vertices): one ppgpu_water_route_record and ALL vertices of the route, seed first (the device writes the first
    min(vertices, stride) of them).  gap2: the distance map of the occupancy grid as set."""
    if no_map or (seed_flags & wr.WATER_SEED_BLOCKED):
        return _blank(lim2, WR_NO_MAP if no_map else WR_NO_SEED), []
    rows, cols = wd.shape
    a = rr.seed_cell((rows, cols), res, float(x), float(y))
    if a is None:
        return _blank(lim2, WR_DRY | WR_OUTSIDE), []
    b = approach_cell(wd, a[0], a[1], lim2)
    if int(wd[b]) == NONE:
        rec = _blank(lim2, WR_DRY)
        rec["point_cell"] = a[0] * cols + a[1]
        return rec, []
    cells, codes = walk(dirs, b)
    turns = [i for i in range(1, len(cells) - 1) if codes[i - 1] != codes[i]]           # cell i: arrived by codes[i - 1], left by codes[i]
    vertices = [r * cols + c for r, c in [cells[-1]] + [cells[i] for i in reversed(turns)] + [cells[0]]] if codes else [b[0] * cols + b[1]]
    straight, diagonal = sum(1 for k in codes if k < 4), sum(1 for k in codes if k >= 4)
    flags = (0 if codes else WR_AT_SEED) | (WR_TRUNCATED if len(vertices) > stride else 0)
    gaps = [int(gap2[cell]) for cell in cells]
    low = min(gaps)
    narrow = max(i for i, g in enumerate(gaps) if g == low)                             # the one nearest the seed: the last of the walk
    rec = np.zeros((), dtype=WATER_ROUTE_DTYPE)
    rec["point_cell"], rec["from_cell"], rec["wd"], rec["lim2"] = a[0] * cols + a[1], b[0] * cols + b[1], int(wd[b]), lim2
    rec["straight_steps"], rec["diagonal_steps"], rec["turns"], rec["vertices"] = straight, diagonal, len(turns), len(vertices)
    rec["vertices_written"] = min(len(vertices), stride)
    rec["first_dir"] = (OPPOSITE[codes[-1]] if codes else ROUTE_SEED) | (flags << 8)
    rec["min_gap2"], rec["min_gap2_cell"] = low, cells[narrow][0] * cols + cells[narrow][1]
    rec["metres"] = res * (float(straight) + float(diagonal) * math.sqrt(2.0))
    rec["narrowest_metres"] = res * math.sqrt(float(low))
    return rec, vertices


def routes(wd, gap2, res, points, lim2, stride, seed_flags=0, no_map=False, dirs=None):
    """(records, [all vertices of route i]) of n points {x, y}."""
    if dirs is None and not no_map:
        dirs = step_map_numpy(wd)
    got = [route(wd, dirs, gap2, res, x, y, lim2, stride, seed_flags, no_map) for x, y in np.asarray(points, dtype=np.float64).reshape(-1, 2)]
    return np.array([g[0] for g in got], dtype=WATER_ROUTE_DTYPE), [g[1] for g in got]


def flags_of(rec):
    return int(rec["first_dir"]) >> 8


def code_of(rec):
    return int(rec["first_dir"]) & 0xFF


# ------------------------------------------------------------------------------------------------------------ the planning worlds
def ribbon_points(shape, res, ribbons4, recs):
    """Query i of the host planner: ribbon i's nearest_sample (sample 0 without a wet one), clamped to the grid as the ribbon walk
    clamps it, as the centre of the cell that walk puts it in."""
    pts = []
    for q, rec in zip(np.asarray(ribbons4, dtype=np.float64).reshape(-1, 4), recs):
        _, _, _, r, c, _, _ = wr.sample_cells(shape, res, q)
        k = max(int(rec["nearest_sample"]), 0)
        pts.append(((int(c[k]) + 0.5) * res, (int(r[k]) + 0.5) * res))
    return np.array(pts, dtype=np.float64).reshape(-1, 2)


def plan_routes(w, gap2, limit2):
    """(records, vertices per ribbon, keys, file lines) of a planning world at a keep-out limit, seeded at its start: what
    Planner::Stats::WaterReport::Routes holds and plan_cli prints.  gap2: clearance_replay.gap2_numpy of the world's grid as set."""
    wd, (_, _, _, index), recs, _ = wr.plan_water(w, gap2, limit2)
    flags = wr.WATER_SEED_BLOCKED if index == NONE else 0
    lim2 = rr.ribbon_lim2(w.res, w.cfg.ribbon_width)
    pts = ribbon_points(wd.shape, w.res, w.ribbons4, recs)
    rrecs, verts = routes(wd, gap2, w.res, pts, lim2, VERTEX_STRIDE, seed_flags=flags)
    nearest = wr.nearest_keys(recs, w.res, np.asarray(w.ribbons4, dtype=np.float64).reshape(-1, 4), float(w.start5[0]), float(w.start5[1]))["nearest_ribbon_by_water"]
    keys = {"water_route_metres": -1.0, "water_route_turns": -1, "water_route_vertices": -1, "water_route_truncated": False,
            "water_route_narrowest_metres": -1.0, "water_route_first_dir": -1}
    if nearest >= 0:
        r = rrecs[nearest]
        keys = {"water_route_metres": float(r["metres"]), "water_route_turns": int(r["turns"]), "water_route_vertices": int(r["vertices"]),
                "water_route_truncated": bool(flags_of(r) & WR_TRUNCATED), "water_route_narrowest_metres": float(r["narrowest_metres"]),
                "water_route_first_dir": code_of(r)}
    cols = wd.shape[1]
    lines = [(i, j, (v % cols + 0.5) * w.res, (v // cols + 0.5) * w.res) for i, vs in enumerate(verts) for j, v in enumerate(vs[:VERTEX_STRIDE])]
    return rrecs, verts, keys, lines
