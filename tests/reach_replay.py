"""The definitions the device's reachable-water reports are compared against (include/ppgpu.h, "reachable water"): canonical
8-connected component labels (ppgpu_get_grid_labels -> pp_k_reach_tiles / _merge / _flatten), the reach-gap map of a seed
(ppgpu_get_grid_reach_gap -> pp_k_reach_bits, pp_k_dist_cols / pp_k_dist_rows without the outside as a source) and the record of a
ribbon's sample points (ppgpu_ribbon_reach_host -> pp_k_reach_ribbons), and the directed grids of the label tests.

A plain module, numpy only: no fixtures, no device.  Everything is integer arithmetic except where a ribbon's samples are placed,
which follows the header's order of operations in float64."""
import math

import numpy as np

import clearance_replay as clr
from path_planner_amd.types import (DIST_CAP2, REACH_NONE, REACH_TILE, REACH_SEED_BLOCKED, RIBBON_REACH_DTYPE, RB_ANY_OUT, RB_WHOLE_OUT,
                                    RB_START_OUT, RB_END_OUT, RB_DEGENERATE, RB_CAPPED, RB_NO_SEED, RB_NO_MAP)

T = REACH_TILE
PAD = 256                 # source-free cells around the reach set: farther than the map's cap, so the padded border decides nothing


# ------------------------------------------------------------------------------------------------------------ labels
def labels_numpy(grid):
    """label(r, c) = the smallest row-major index over the 8-connected component of free cell (r, c), REACH_NONE on a blocked cell:
    a union-find over the runs of free cells of each row (two runs of neighbouring rows touch when their column ranges, widened
    by one, overlap), the smaller root winning, so a root's first cell is the component's smallest index."""
    g = np.asarray(grid) != 0
    rows, cols = g.shape
    out = np.full((rows, cols), REACH_NONE, dtype=np.uint32)
    free = np.zeros((rows, cols + 2), dtype=np.int8)
    free[:, 1:-1] = ~g
    edge = np.diff(free, axis=1)
    rr, cs = np.nonzero(edge == 1)                    # a run starts at column cs ...
    _, ce = np.nonzero(edge == -1)                    # ... and ends before column ce (same order: row by row, left to right)
    n = len(rr)
    parent = np.arange(n)

    def find(i):
        root = i
        while parent[root] != root:
            root = parent[root]
        while parent[i] != root:
            parent[i], i = root, parent[i]
        return root

    first = np.searchsorted(rr, np.arange(rows + 1))  # runs of row r: first[r] .. first[r + 1]
    for r in range(1, rows):
        i, iend, j, jend = first[r - 1], first[r], first[r], first[r + 1]
        while i < iend and j < jend:
            if cs[i] <= ce[j] and cs[j] <= ce[i]:     # [cs, ce) ranges that overlap or touch diagonally
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)     # runs are numbered in row-major order of their first cells
            if ce[i] < ce[j]:
                i += 1
            else:
                j += 1
    for k in range(n):
        root = find(k)
        out[rr[k], cs[k]:ce[k]] = rr[root] * cols + cs[root]
    return out


def labels_brute(grid, connectivity=8):
    """The definition by flood fill, cell by cell in row-major order: the first cell of a component names it."""
    g = np.asarray(grid) != 0
    rows, cols = g.shape
    out = np.full((rows, cols), REACH_NONE, dtype=np.uint32)
    steps = [(dr, dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1) if (dr or dc) and (connectivity == 8 or not (dr and dc))]
    for r0 in range(rows):
        for c0 in range(cols):
            if g[r0, c0] or out[r0, c0] != REACH_NONE:
                continue
            out[r0, c0] = r0 * cols + c0
            stack = [(r0, c0)]
            while stack:
                r, c = stack.pop()
                for dr, dc in steps:
                    rr, cc = r + dr, c + dc
                    if 0 <= rr < rows and 0 <= cc < cols and not g[rr, cc] and out[rr, cc] == REACH_NONE:
                        out[rr, cc] = r0 * cols + c0
                        stack.append((rr, cc))
    return out


def totals(labels):
    """(free cells, components, size of the largest component)."""
    lab = np.asarray(labels).ravel()
    free = lab != REACH_NONE
    roots = lab == np.arange(lab.size, dtype=np.uint32)
    largest = int(np.bincount(lab[free].astype(np.int64)).max()) if free.any() else 0
    return int(free.sum()), int(roots.sum()), largest


# ------------------------------------------------------------------------------------------------------------ the reach set
def seed_cell(grid_shape, res, x, y):
    """The cell GridWorldMap::isBlocked puts the pose in, or None outside the grid."""
    rows, cols = grid_shape
    if x < 0 or x / res >= cols or y < 0 or y / res >= rows:
        return None
    return int(y / res), int(x / res)


def seed_label(labels, res, x, y):
    cell = seed_cell(labels.shape, res, x, y)
    return REACH_NONE if cell is None else int(labels[cell])


def reach_set(labels, label):
    return np.zeros(labels.shape, dtype=bool) if label == REACH_NONE else labels == np.uint32(label)


def rgap2_numpy(reach):
    """min(rgap2, DIST_CAP2): clearance_replay.gap2_numpy with the reach set as the hazards, padded by PAD source-free cells on every
    side so that the outside of the grid, a hazard of that function, is farther than the cap from every cell of the grid."""
    rows, cols = reach.shape
    padded = np.zeros((rows + 2 * PAD, cols + 2 * PAD), dtype=np.uint8)
    padded[PAD:PAD + rows, PAD:PAD + cols] = reach
    return np.ascontiguousarray(clr.gap2_numpy(padded)[PAD:PAD + rows, PAD:PAD + cols])


def rgap2_brute(reach):
    rows, cols = reach.shape
    br, bc = np.nonzero(reach)
    out = np.full((rows, cols), DIST_CAP2, dtype=np.int64)
    if len(br):
        for r in range(rows):
            for c in range(cols):
                gr, gc = np.maximum(np.abs(br - r) - 1, 0), np.maximum(np.abs(bc - c) - 1, 0)
                out[r, c] = min(int((gr * gr + gc * gc).min()), DIST_CAP2)
    return out.astype(np.uint16)


# ------------------------------------------------------------------------------------------------------------ ribbons
def ribbon_lim2(res, ribbon_width):
    return clr.limit2(res, ribbon_width + 0.25 * res)


def ribbon_samples(ribbon, res):
    """(len, n, sample count, x[k], y[k]) in the header's order: separate products and sums, k / n first."""
    sx, sy, ex, ey = (float(v) for v in ribbon)
    dx, dy = ex - sx, ey - sy
    length = math.sqrt(dx * dx + dy * dy)
    n = max(1, int(math.ceil(length / (0.5 * res))))
    count = 1 if length == 0.0 else n + 1
    t = np.arange(count, dtype=np.float64) / float(n)
    return length, n, count, sx + dx * t, sy + dy * t


def ribbon_record(rgap2, res, ribbon, ribbon_width, seed_flags=0, no_map=False):
    """One ppgpu_ribbon_reach_record.  `rgap2` is the capped map of the current seed; with a blocked seed (seed_flags) or the base Map
    nothing is judged."""
    rec = np.zeros((), dtype=RIBBON_REACH_DTYPE)
    res_used = 1.0 if no_map else res
    length, n, count, x, y = ribbon_samples(ribbon, res_used)
    if no_map:
        n, count = 1, (1 if length == 0.0 else 2)
    rec["length"], rec["pitch"], rec["samples"] = length, (0.0 if length == 0.0 else length / n), count
    rec["first_out"] = rec["last_out"] = -1
    rec["lim2"] = 0 if no_map else ribbon_lim2(res, ribbon_width)
    flags = RB_DEGENERATE if length == 0.0 else 0
    if no_map or (seed_flags & REACH_SEED_BLOCKED):
        rec["flags"] = flags | (RB_NO_MAP if no_map else RB_NO_SEED)
        return rec
    rows, cols = rgap2.shape
    x, y = np.clip(x, 0.0, cols * res), np.clip(y, 0.0, rows * res)
    c = np.minimum((x / res).astype(np.int64), cols - 1)
    r = np.minimum((y / res).astype(np.int64), rows - 1)
    g2 = rgap2[r, c].astype(np.int64)
    out = g2 >= int(rec["lim2"])
    k = np.nonzero(out)[0]
    rec["out_samples"] = len(k)
    if len(k):
        rec["first_out"], rec["last_out"] = k[0], k[-1]
        flags |= RB_ANY_OUT | (RB_WHOLE_OUT if len(k) == count else 0) | (RB_START_OUT if out[0] else 0) | (RB_END_OUT if out[-1] else 0)
    rec["min_rgap2"], rec["max_rgap2"] = g2.min(), g2.max()
    if g2.max() == DIST_CAP2:
        flags |= RB_CAPPED
    rec["flags"] = flags
    rec["out_length"] = min(float(rec["pitch"]) * len(k), length)
    return rec


def ribbon_records(rgap2, res, ribbons, ribbon_width, seed_flags=0, no_map=False):
    ribbons = np.asarray(ribbons, dtype=np.float64).reshape(-1, 4)
    return np.array([ribbon_record(rgap2, res, q, ribbon_width, seed_flags, no_map) for q in ribbons], dtype=RIBBON_REACH_DTYPE)


# ------------------------------------------------------------------------------------------------------------ directed grids
def percolation(rows, cols, p, seed):
    return (np.random.default_rng(seed).uniform(size=(rows, cols)) < p).astype(np.uint8)


def checkerboard(rows, cols):
    r, c = np.indices((rows, cols))
    return ((r + c) & 1).astype(np.uint8)


def diagonal_channel(n, anti=False):
    """Everything blocked but a one-cell-wide diagonal: it crosses every tile corner on its way."""
    g = np.ones((n, n), dtype=np.uint8)
    k = np.arange(n)
    g[k, (n - 1 - k) if anti else k] = 0
    return g


def nested_rings(n=3 * T + 5):
    """Open water, a ring wall, water, a ring wall, water: a basin inside a basin (three components)."""
    g = np.zeros((n, n), dtype=np.uint8)
    for inset in (6, T + 3):
        g[inset, inset:n - inset] = g[n - 1 - inset, inset:n - inset] = 1
        g[inset:n - inset, inset] = g[inset:n - inset, n - 1 - inset] = 1
    return g


def comb(rows=2 * T, cols=3 * T + 4):
    """Free teeth in every other column that join only along the last row; the teeth end on a tile border."""
    g = np.ones((rows, cols), dtype=np.uint8)
    g[:, ::2] = 0
    g[:T, ::4] = 1                                    # every other tooth starts at the tile border
    g[rows - 1, :] = 0
    return g


def isolated(rows=2 * T + 3, cols=2 * T + 5):
    g = np.ones((rows, cols), dtype=np.uint8)
    g[::2, ::2] = 0
    return g


def serpentine(rows=130, cols=131):
    """Two-row corridors between two-row walls, each wall open for one column at alternate ends: one component."""
    g = np.zeros((rows, cols), dtype=np.uint8)
    for k, r in enumerate(range(2, rows, 4)):
        if k % 2 == 0:
            g[r:r + 2, :cols - 1] = 1
        else:
            g[r:r + 2, 1:] = 1
    return g


def spiral(n=2 * T + 7):
    """A one-cell corridor that winds inwards between one-cell walls: legs of n-1, n-1, n-1, n-3, n-3, n-5, n-5, ... cells."""
    g = np.ones((n, n), dtype=np.uint8)
    g[0, 0] = 0
    legs = [n - 1, n - 1, n - 1] + [v for k in range(n - 3, 0, -2) for v in (k, k)]
    r, c, dr, dc = 0, 0, 0, 1
    for leg in legs:
        for _ in range(leg):
            r, c = r + dr, c + dc
            g[r, c] = 0
        dr, dc = dc, -dr
    return g


# ------------------------------------------------------------------------------------------------------------ the planning world
# grid_worlds.wide_plan's grid (37 x 83 @ 1.0 m) with a wall along row 27 that is open at columns 40-44: at a keep-out margin of 3 m
# (limit2 9) the five-cell strait closes and the water north of the wall is out of reach.  Ribbon width 1.5: lim2 = 4.
PLAN_WALL_ROW, PLAN_STRAIT = 27, (40, 45)
PLAN_RIBBONS = [[30.0, 24.0, 55.0, 24.0], [30.0, 31.5, 55.0, 31.5], [42.5, 20.0, 42.5, 34.0]]
PLAN_MARGINS = {0.0: 0, 1.0: 1, 3.0: 9}     # metres: limit2


def plan_world():
    """(workload, initial samples, clock polls, gap2 of its grid)"""
    import grid_worlds as gw
    from path_planner_amd import workloads
    base, init, calls = gw.wide_plan()
    g = base.grid.copy()
    g[PLAN_WALL_ROW, :] = 1
    g[PLAN_WALL_ROW, PLAN_STRAIT[0]:PLAN_STRAIT[1]] = 0
    w = workloads.Workload("reach_plan", g, base.res, None, PLAN_RIBBONS, list(base.start5), 128, 7, base.cfg)
    return w, init, calls, clr.gap2_numpy(g)


def plan_reach(w, gap2, limit2):
    """(labels, seed label, (free, components), records) of the planning world at a keep-out limit, seeded at its start."""
    eff = ((gap2.astype(np.int64) < int(limit2)) | (w.grid != 0)).astype(np.uint8)
    labels = labels_numpy(eff)
    label = seed_label(labels, w.res, float(w.start5[0]), float(w.start5[1]))
    free, comps, _ = totals(labels)
    flags = REACH_SEED_BLOCKED if label == REACH_NONE else 0
    recs = ribbon_records(rgap2_numpy(reach_set(labels, label)), w.res, w.ribbons4, w.cfg.ribbon_width, seed_flags=flags)
    return labels, label, (free, comps), recs
