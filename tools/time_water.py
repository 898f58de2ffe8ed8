#!/usr/bin/env python3
"""What the distance by water costs on the device (ppgpu_last_water_timing: HIP events from the fill of the map to its totals, the
host's reads of the rounds' active counts between the batches of launches included, and around the ribbon walk), next to the label
build on the same handle, on 2048 x 2048 grids: config 3's and an empty one, each seeded at the centre and in a corner.  Every build
follows a ppgpu_set_grid (the map is stale then); medians over --reps builds after one warm-up build.  Then the walk of 64 ribbons.

    python tools/time_water.py [--reps 10] [--out profiles/water.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N = 2048


def _free_near(grid, r, c):
    """The free cell nearest to (r, c)."""
    free = np.argwhere(grid == 0)
    return tuple(free[np.argmin((free[:, 0] - r) ** 2 + (free[:, 1] - c) ** 2)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from path_planner_amd import api, workloads
    w = workloads.config3(n_samples=16, n_obst=0)
    assert w.grid.shape == (N, N)
    ctx = api.Context(0)
    ctx.set_config(w.cfg)
    ctx.enable_timing(True)
    fmt = lambda v: "%.3f (%.3f .. %.3f)" % (float(np.median(v)), min(v), max(v))
    lines = ["device: " + torch.cuda.get_device_name(0),
             "%d x %d grids at %.2f m; medians of %d builds after a warm-up one, ms (min .. max); batches of %s rounds" %
             (N, N, w.res, a.reps, os.environ.get("PPGPU_WATER_BATCH", "16")),
             "map = fill + pp_k_water_seed + rounds of pp_k_water_round (with the host's reads of the active counts) + pp_k_water_totals;",
             "labels = pp_k_reach_tiles + pp_k_reach_merge + pp_k_reach_flatten on the same handle (ppgpu_last_reach_timing)"]
    rng = np.random.default_rng(11)
    ribbons = rng.uniform(0.0, N * w.res, size=(64, 4))
    for name, grid in (("config 3", w.grid), ("empty", np.zeros((N, N), dtype=np.uint8))):
        for where, (r, c) in (("centre", _free_near(grid, N // 2, N // 2)), ("corner", _free_near(grid, 0, 0))):
            x, y = (c + 0.5) * w.res, (r + 0.5) * w.res
            t = {"map": [], "rounds": [], "labels": [], "ribbons": []}
            for rep in range(a.reps + 1):
                ctx.set_grid(grid, w.res)                    # the map and the labels are stale again
                info = ctx.set_water_seed(x, y)
                recs = ctx.ribbon_water(ribbons, w.cfg.ribbon_width)
                ms = ctx.last_water_timing()
                ctx.get_grid_labels(N, N)
                if rep:
                    t["map"].append(ms[0]); t["ribbons"].append(ms[1]); t["rounds"].append(int(info["rounds"])); t["labels"].append(ctx.last_reach_timing()[0])
            lines.append("  %-9s seed %-6s cell (%4d, %4d)  wet %8d  max %.1f m  rounds %d .. %d" %
                         (name, where, r, c, info["wet_cells"], w.res * info["max_wd"] / 12.0, min(t["rounds"]), max(t["rounds"])))
            lines.append("  %-9s      %-6s map %s  labels %s  walk of 64 ribbons (%d samples, lim2 %d, %d dry) %s" %
                         ("", "", fmt(t["map"]), fmt(t["labels"]), int(recs["samples"].sum()), int(recs["lim2"][0]), int(((recs["flags"] & 2) != 0).sum()),
                          fmt(t["ribbons"])))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
