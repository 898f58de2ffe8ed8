#!/usr/bin/env python3
"""What the route by water costs on the device (ppgpu_last_water_route_timing: HIP events around pp_k_water_dirs and around
pp_k_water_routes), next to the build of the water map on the same handle (ppgpu_last_water_timing), at 2048 x 2048:
  - config 3's world seeded at its start, with the routes to its ribbons (each ribbon's nearest sample, the records' lim2, stride 256);
  - a serpentine grid seeded at its first free cell with the route to its farthest cell, the worst case for the chain of loads.
Every build follows a ppgpu_set_grid (the maps are stale then); medians over --reps calls after one warm-up call.

    python tools/time_route.py [--reps 20] [--out profiles/route.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N = 2048
STRIDE = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import reach_replay as rr
    from path_planner_amd import api, workloads
    from path_planner_amd.types import WR_DRY, WR_TRUNCATED
    w = workloads.config3(n_samples=16, n_obst=0)
    assert w.grid.shape == (N, N)
    ctx = api.Context(0)
    ctx.set_config(w.cfg)
    ctx.enable_timing(True)
    fmt = lambda v: "%.3f (%.3f .. %.3f)" % (float(np.median(v)), min(v), max(v))
    lines = ["device: " + torch.cuda.get_device_name(0),
             "%d x %d grids at %.2f m; medians of %d calls after a warm-up one, ms (min .. max)" % (N, N, w.res, a.reps),
             "map = the build of the water map (ppgpu_last_water_timing); dirs = pp_k_water_dirs; routes = pp_k_water_routes, one wave per route"]
    serp = rr.serpentine(N, N)
    first = np.argwhere(serp == 0)[0]
    cases = (("config 3", w.grid, float(w.start5[0]), float(w.start5[1]), w.ribbons4),
             ("serpentine", serp, (first[1] + 0.5) * w.res, (first[0] + 0.5) * w.res, None))
    for name, grid, x, y, ribbons in cases:
        t = {"map": [], "dirs": [], "routes": []}
        for rep in range(a.reps + 1):
            ctx.set_grid(grid, w.res)                        # the maps are stale again
            info = ctx.set_water_seed(x, y)
            if ribbons is not None:
                recs = ctx.ribbon_water(ribbons, w.cfg.ribbon_width)
                k = np.maximum(recs["nearest_sample"], 0)
                pts = np.array([[float(s[3][i]), float(s[4][i])] for s, i in ((rr.ribbon_samples(q, w.res), int(i)) for q, i in zip(ribbons, k))])
                pts = np.clip(pts, 0.0, (N - 0.5) * w.res)
                lim2 = int(recs["lim2"][0])
            else:
                far = divmod(int(info["farthest_cell"]), N)
                pts, lim2 = np.array([[(far[1] + 0.5) * w.res, (far[0] + 0.5) * w.res]]), 0
            got, _ = ctx.water_routes(pts, lim2, STRIDE)
            ms_map = ctx.last_water_timing()[0]
            ms_dirs, ms_routes = ctx.last_water_route_timing()
            if rep:
                t["map"].append(ms_map); t["dirs"].append(ms_dirs); t["routes"].append(ms_routes)
        flags = got["first_dir"] >> 8
        wet = (flags & WR_DRY) == 0
        steps = (got["straight_steps"].astype(np.int64) + got["diagonal_steps"])[wet]
        lines.append("  %-10s wet %8d  rounds %d  %d route(s), lim2 %d: %d dry, %d truncated at %d vertices; steps %d .. %d, turns %d .. %d" %
                     (name, info["wet_cells"], info["rounds"], len(got), lim2, int((~wet).sum()), int(((flags & WR_TRUNCATED) != 0).sum()), STRIDE,
                      steps.min() if len(steps) else 0, steps.max() if len(steps) else 0, got["turns"][wet].min() if wet.any() else 0,
                      got["turns"][wet].max() if wet.any() else 0))
        lines.append("  %-10s map %s  dirs %s  routes %s" % ("", fmt(t["map"]), fmt(t["dirs"]), fmt(t["routes"])))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
