"""The definitions the device's distance-by-water reports are compared against (include/ppgpu.h, "distance by water"): the map of a
seed (ppgpu_get_grid_water -> pp_k_water_round), its totals (ppgpu_set_water_seed -> pp_k_water_totals), the approach distance of a
cell and the record of a ribbon's sample points (ppgpu_ribbon_water_host -> pp_k_water_ribbons), and the detour world of the host
planner's test.

A plain module, numpy and heapq only: no fixtures, no device.  Everything is integer arithmetic except where a ribbon's samples are
placed, which is reach_replay's (the header's order of operations in float64)."""
import heapq
import math

import numpy as np

import clearance_replay as clr
import reach_replay as rr
from path_planner_amd.types import (WATER_NONE, WATER_STEP, WATER_DIAG, WATER_MAX_LIM2, WATER_SEED_BLOCKED, RIBBON_WATER_DTYPE, RW_ANY_DRY, RW_WHOLE_DRY,
                                    RW_DEGENERATE, RW_NO_SEED, RW_NO_MAP)

NONE = WATER_NONE


# ------------------------------------------------------------------------------------------------------------ the map
def wd_dijkstra(grid, seed_cell):
    """wd(cell): the cost of the cheapest 8-connected path through free cells from seed_cell = (r, c) or None, 12 per row or column
    step, 17 per diagonal step whatever the two cells beside it hold; NONE on blocked cells, on other components, and everywhere for
    a seed that is None or blocked.  Dijkstra with a heap over a grid padded by one blocked cell all round."""
    g = np.asarray(grid) != 0
    rows, cols = g.shape
    out = np.full((rows, cols), NONE, dtype=np.uint32)
    if seed_cell is None or g[seed_cell]:
        return out
    w = cols + 2
    blocked = np.ones((rows + 2, w), dtype=bool)
    blocked[1:-1, 1:-1] = g
    blocked = blocked.ravel().tolist()
    inf = 1 << 62
    dist = [inf] * len(blocked)
    steps = ((-w, WATER_STEP), (w, WATER_STEP), (-1, WATER_STEP), (1, WATER_STEP), (-w - 1, WATER_DIAG), (-w + 1, WATER_DIAG), (w - 1, WATER_DIAG), (w + 1, WATER_DIAG))
    s = (seed_cell[0] + 1) * w + seed_cell[1] + 1
    dist[s] = 0
    heap = [(0, s)]
    pop, push = heapq.heappop, heapq.heappush
    while heap:
        d, i = pop(heap)
        if d > dist[i]:
            continue
        for off, cost in steps:
            j = i + off
            if not blocked[j]:
                nd = d + cost
                if nd < dist[j]:
                    dist[j] = nd
                    push(heap, (nd, j))
    d = np.array(dist, dtype=np.int64).reshape(rows + 2, w)[1:-1, 1:-1]
    wet = d != inf
    assert not wet.any() or d[wet].max() < NONE
    out[wet] = d[wet]
    return out


def wd_bellman_ford(grid, seed_cell):
    """The same map as the fixed point of whole-grid numpy sweeps (each cell takes the minimum over its eight neighbours): slow on
    corridors, independent of the heap."""
    g = np.asarray(grid) != 0
    rows, cols = g.shape
    inf = np.int64(1) << 62
    d = np.full((rows + 2, cols + 2), inf, dtype=np.int64)
    if seed_cell is not None and not g[seed_cell]:
        d[seed_cell[0] + 1, seed_cell[1] + 1] = 0
        free = ~g
        for _ in range(rows * cols + 1):
            best = d[1:-1, 1:-1].copy()
            for dr in (0, 1, 2):
                for dc in (0, 1, 2):
                    if dr != 1 or dc != 1:
                        np.minimum(best, d[dr:dr + rows, dc:dc + cols] + (WATER_DIAG if (dr != 1 and dc != 1) else WATER_STEP), out=best)
            best[~free] = inf
            if np.array_equal(best, d[1:-1, 1:-1]):
                break
            d[1:-1, 1:-1] = best
        else:
            raise AssertionError("no fixed point")
    inner = d[1:-1, 1:-1]
    out = np.full((rows, cols), NONE, dtype=np.uint32)
    wet = inner < inf
    out[wet] = inner[wet]
    return out


def totals(wd):
    """(wet cells, the largest distance, the lowest row-major index that attains it): (0, 0, NONE) when nothing is wet."""
    flat = np.asarray(wd).ravel()
    wet = flat != NONE
    if not wet.any():
        return 0, 0, NONE
    top = int(flat[wet].max())
    return int(wet.sum()), top, int(np.nonzero(wet & (flat == top))[0][0])


def seed_index(grid, res, x, y):
    """(cell or None, the row-major index the info block reports): NONE for a seed outside the grid or on a blocked cell."""
    cell = rr.seed_cell(np.asarray(grid).shape, res, x, y)
    if cell is None or np.asarray(grid)[cell]:
        return None, NONE
    return cell, cell[0] * np.asarray(grid).shape[1] + cell[1]


def metres(res, wd):
    """resolution * wd / 12 in the header's order; +inf for NONE."""
    wd = np.asarray(wd)
    return np.where(wd == NONE, np.inf, res * wd.astype(np.float64) / float(WATER_STEP))


# ------------------------------------------------------------------------------------------------------------ ribbons
def approach(wd, r, c, lim2):
    """ad(A) for A = (r, c): the minimum of wd(B) over the cells B of the grid with gap2(A, B) < lim2, cell by cell."""
    rows, cols = wd.shape
    best = NONE
    assert lim2 <= WATER_MAX_LIM2
    reach = 34                                              # max(|dr| - 1, 0)^2 < 1024 keeps |dr| below 33
    for rr_ in range(max(r - reach, 0), min(r + reach, rows - 1) + 1):
        for cc in range(max(c - reach, 0), min(c + reach, cols - 1) + 1):
            if max(abs(rr_ - r) - 1, 0) ** 2 + max(abs(cc - c) - 1, 0) ** 2 < lim2:
                best = min(best, int(wd[rr_, cc]))
    return best


def approach_map(wd, lim2):
    """ad of every cell at once: the minimum over the shifts (dr, dc) with gap2 < lim2."""
    rows, cols = wd.shape
    reach = 0
    while reach * reach < lim2:
        reach += 1
    pad = np.full((rows + 2 * reach, cols + 2 * reach), NONE, dtype=np.uint32)
    pad[reach:reach + rows, reach:reach + cols] = wd
    out = np.full((rows, cols), NONE, dtype=np.uint32)
    for dr in range(-reach, reach + 1):
        for dc in range(-reach, reach + 1):
            if max(abs(dr) - 1, 0) ** 2 + max(abs(dc) - 1, 0) ** 2 < lim2:
                np.minimum(out, pad[reach + dr:reach + dr + rows, reach + dc:reach + dc + cols], out=out)
    return out


def sample_cells(shape, res, ribbon):
    """(len, n, count, r[k], c[k], x[k], y[k]) of a ribbon's samples: reach_replay's placement, the clamp and the cell rule."""
    rows, cols = shape
    length, n, count, x, y = rr.ribbon_samples(ribbon, res)
    xc, yc = np.clip(x, 0.0, cols * res), np.clip(y, 0.0, rows * res)
    c = np.minimum((xc / res).astype(np.int64), cols - 1)
    r = np.minimum((yc / res).astype(np.int64), rows - 1)
    return length, n, count, r, c, x, y


def ribbon_record(wd, res, ribbon, ribbon_width, seed_flags=0, no_map=False, ad_map=None):
    """One ppgpu_ribbon_water_record.  `wd` is the map of the current seed; with a blocked seed (seed_flags) or the base Map nothing
    is judged.  ad_map: approach_map(wd, lim2) when the caller has it (many ribbons on one map)."""
    rec = np.zeros((), dtype=RIBBON_WATER_DTYPE)
    res_used = 1.0 if no_map else res
    length, n, count, _, _ = rr.ribbon_samples(ribbon, res_used)
    if no_map:
        n, count = 1, (1 if length == 0.0 else 2)
    rec["length"], rec["pitch"], rec["samples"] = length, (0.0 if length == 0.0 else length / n), count
    rec["nearest_sample"] = rec["farthest_sample"] = -1
    rec["min_ad"] = rec["max_ad"] = rec["start_ad"] = rec["end_ad"] = NONE
    rec["nearest_metres"] = np.inf
    lim2 = 0 if no_map else rr.ribbon_lim2(res, ribbon_width)
    assert lim2 <= WATER_MAX_LIM2
    rec["lim2"] = lim2
    flags = RW_DEGENERATE if length == 0.0 else 0
    if no_map or (seed_flags & WATER_SEED_BLOCKED):
        rec["flags"] = flags | (RW_NO_MAP if no_map else RW_NO_SEED)
        return rec
    _, _, _, r, c, _, _ = sample_cells(wd.shape, res, ribbon)
    if ad_map is not None:
        ad = ad_map[r, c].astype(np.int64)
    else:
        ad = np.array([approach(wd, int(a), int(b), lim2) for a, b in zip(r, c)], dtype=np.int64)
    wet = ad != NONE
    rec["wet_samples"] = int(wet.sum())
    rec["start_ad"], rec["end_ad"] = ad[0], ad[-1]
    if wet.any():
        lo, hi = int(ad[wet].min()), int(ad[wet].max())
        rec["min_ad"], rec["max_ad"] = lo, hi
        rec["nearest_sample"] = int(np.nonzero(wet & (ad == lo))[0][0])          # the lowest index on a tie
        rec["farthest_sample"] = int(np.nonzero(wet & (ad == hi))[0][0])
        rec["nearest_metres"] = res * float(lo) / float(WATER_STEP)
    if not wet.all():
        flags |= RW_ANY_DRY | (0 if wet.any() else RW_WHOLE_DRY)
    rec["flags"] = flags
    return rec


def ribbon_records(wd, res, ribbons, ribbon_width, seed_flags=0, no_map=False):
    ribbons = np.asarray(ribbons, dtype=np.float64).reshape(-1, 4)
    ad_map = None
    if not no_map and not (seed_flags & WATER_SEED_BLOCKED):
        ad_map = approach_map(wd, rr.ribbon_lim2(res, ribbon_width))
    return np.array([ribbon_record(wd, res, q, ribbon_width, seed_flags, no_map, ad_map) for q in ribbons], dtype=RIBBON_WATER_DTYPE)


# ------------------------------------------------------------------------------------------------------------ the planning worlds
# reach_replay.plan_world, and the same world with the strait moved to the far end of the wall: ribbon 1, just behind the wall, is a
# few metres from the start in a straight line and several times that by water.
DETOUR_STRAIT = (78, 83)


def detour_world():
    """(workload, initial samples, clock polls, gap2 of its grid): plan_world's with the wall of row 27 open at columns 78-82 only."""
    from path_planner_amd import workloads
    w, init, calls, _ = rr.plan_world()
    g = w.grid.copy()
    g[rr.PLAN_WALL_ROW, :] = 1
    g[rr.PLAN_WALL_ROW, DETOUR_STRAIT[0]:DETOUR_STRAIT[1]] = 0
    w2 = workloads.Workload("water_detour", g, w.res, None, rr.PLAN_RIBBONS, list(w.start5), 128, 7, w.cfg)
    return w2, init, calls, clr.gap2_numpy(g)


def plan_water(w, gap2, limit2):
    """(wd, (wet, max_wd, farthest, seed index), records, keys) of a planning world at a keep-out limit, seeded at its start; keys are
    plan_cli's: ribbons_dry, nearest_ribbon_by_water, nearest_ribbon_water_metres, nearest_ribbon_straight_metres, water_max_metres."""
    eff = ((gap2.astype(np.int64) < int(limit2)) | (w.grid != 0)).astype(np.uint8)
    x0, y0 = float(w.start5[0]), float(w.start5[1])
    cell, index = seed_index(eff, w.res, x0, y0)
    wd = wd_dijkstra(eff, cell)
    flags = WATER_SEED_BLOCKED if cell is None else 0
    recs = ribbon_records(wd, w.res, w.ribbons4, w.cfg.ribbon_width, seed_flags=flags)
    wet, top, far = totals(wd)
    keys = {"water_cells": wet, "water_max_metres": w.res * float(top) / float(WATER_STEP), "water_seed_blocked": cell is None,
            "ribbons_dry": int(((recs["flags"] & RW_WHOLE_DRY) != 0).sum()) if cell is not None else 0}
    keys.update(nearest_keys(recs, w.res, np.asarray(w.ribbons4, dtype=np.float64).reshape(-1, 4), x0, y0))
    return wd, (wet, top, far, index), recs, keys


def nearest_keys(recs, res, ribbons4, x0, y0):
    """The ribbon with the smallest min_ad (the lowest index on a tie; -1, and -1 for both
    distances, without a wet one), its metres by water, and the straight
    line from the start to its nearest_sample point (sx + dx * (k / n), sy + dy * (k / n)): the point on the ribbon, not clamped."""
    best = -1
    for i, r in enumerate(recs):
        if r["wet_samples"] and (best < 0 or r["min_ad"] < recs[best]["min_ad"]):
            best = i
    if best < 0:
        return {"nearest_ribbon_by_water": -1, "nearest_ribbon_water_metres": -1.0, "nearest_ribbon_straight_metres": -1.0}
    _, _, _, x, y = rr.ribbon_samples(ribbons4[best], res)
    k = int(recs[best]["nearest_sample"])
    ddx, ddy = float(x[k]) - x0, float(y[k]) - y0
    return {"nearest_ribbon_by_water": best, "nearest_ribbon_water_metres": float(recs[best]["nearest_metres"]),
            "nearest_ribbon_straight_metres": math.sqrt(ddx * ddx + ddy * ddy)}
