#!/usr/bin/env python3
"""What the reachable-water report costs on the device (ppgpu_last_reach_timing: HIP events around the three labelling kernels, around
pp_k_reach_bits and the two passes of the reach-gap map, and around the ribbon walk), next to the distance-map build on the same
handle, on 2048 x 2048 grids: config 3's at keep-out limits 0 and 9, a serpentine, and a percolation grid at 0.59.  Every build
follows a ppgpu_set_grid (the labels are stale then); medians over --reps builds after one warm-up build.  Then, unless --no-replan,
tools/replan_loop.py with plan_reach off and on in alternating runs from the same build.

    python tools/time_reach.py [--reps 20] [--cycles 120] [--runs 3] [--no-replan] [--out profiles/reach.txt]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N = 2048


def _grids(w):
    import reach_replay as rr
    return [("config 3, limit2 0", w.grid, 0), ("config 3, limit2 9", w.grid, 9), ("serpentine", rr.serpentine(N, N), 0),
            ("percolation 0.59", rr.percolation(N, N, 0.59, 3), 0)]


def _device_section(a, lines):
    import torch
    from path_planner_amd import api, workloads
    from path_planner_amd.types import REACH_NONE
    w = workloads.config3(n_samples=16, n_obst=0)
    assert w.grid.shape == (N, N)
    ctx = api.Context(0)
    ctx.set_config(w.cfg)
    ctx.enable_timing(True)
    lines += ["device: " + torch.cuda.get_device_name(0),
              "%d x %d grids at %.2f m; %d ribbons of config 3, ribbon width %.2f; medians of %d builds after a warm-up one, ms (min .. max)" %
              (N, N, w.res, len(w.ribbons4), w.cfg.ribbon_width, a.reps),
              "labels = pp_k_reach_tiles + pp_k_reach_merge + pp_k_reach_flatten; reach gap = pp_k_reach_bits + pp_k_dist_cols + pp_k_dist_rows;",
              "distance map = pp_k_dist_cols + pp_k_dist_rows of the chart on the same handle (ppgpu_last_grid_distance_timing)"]
    fmt = lambda v: "%.4f (%.4f .. %.4f)" % (float(np.median(v)), min(v), max(v))
    for name, grid, limit2 in _grids(w):
        ctx.set_keepout_limit2(limit2)
        ctx.set_grid(grid, w.res)
        labels = ctx.get_grid_labels(N, N).ravel()
        free = labels != REACH_NONE
        big = int(np.bincount(labels[free].astype(np.int64)).argmax())
        seed = ((big % N + 0.5) * w.res, (big // N + 0.5) * w.res)
        t = {"labels": [], "gap": [], "ribbons": [], "dist": []}
        for rep in range(a.reps + 1):
            ctx.set_grid(grid, w.res)                    # the labels, the distance map and the reach set are stale again
            info = ctx.set_reach_seed(*seed)
            recs = ctx.ribbon_reach(w.ribbons4, w.cfg.ribbon_width)
            ms = ctx.last_reach_timing()
            ctx.get_grid_distance(N, N)
            if rep:
                t["labels"].append(ms[0]); t["gap"].append(ms[1]); t["ribbons"].append(ms[2]); t["dist"].append(ctx.last_grid_distance_timing())
        lines.append("  %-20s free %8d  components %6d  reachable %8d  ribbons wholly / partly out %d / %d" %
                     (name, info["free_cells"], info["components"], info["reachable_cells"], int(((recs["flags"] & 2) != 0).sum()),
                      int(((recs["flags"] & 3) == 1).sum())))
        lines.append("  %-20s labels %s  reach gap %s  ribbon walk %s  distance map %s" % ("", fmt(t["labels"]), fmt(t["gap"]), fmt(t["ribbons"]), fmt(t["dist"])))


def _replan_section(a, lines):
    lines.append("tools/replan_loop.py %d (config 5: 100 ms budget), plan_reach 0 and 1 in alternating runs of the same build:" % a.cycles)
    keys = ("wall_ms_p50", "wall_ms_p99", "late_cycles", "mean_expanded", "first_cycle_ms")
    runs = {0: [], 1: []}
    for run in range(2 * a.runs):
        on = run % 2
        env = dict(os.environ, REPLAN_PLAN_REACH=str(on))
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replan_loop.py"), str(a.cycles)], capture_output=True, text=True, env=env, timeout=600)
        if out.returncode != 0:
            lines.append("  plan_reach %d: the run failed: %s" % (on, (out.stdout + out.stderr).strip().splitlines()[-1:]))
            return
        r = json.loads(out.stdout.strip().splitlines()[-1])
        runs[on].append(r)
        lines.append("  plan_reach %d: " % on + "  ".join("%s %s" % (k, r[k]) for k in keys))
    for on in (0, 1):
        lines.append("  plan_reach %d, median of %d runs: p50 %.3f  p99 %.3f  late cycles (sum) %d  expansions per cycle %.1f" %
                     (on, a.runs, np.median([r["wall_ms_p50"] for r in runs[on]]), np.median([r["wall_ms_p99"] for r in runs[on]]),
                      sum(r["late_cycles"] for r in runs[on]), np.median([r["mean_expanded"] for r in runs[on]])))
    e0, e1 = (np.median([r["mean_expanded"] for r in runs[on]]) for on in (0, 1))
    lines.append("  expansions per cycle with the report on: %+.2f %% of those with it off" % (100.0 * (e1 - e0) / e0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cycles", type=int, default=120)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-replan", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    _device_section(a, lines)
    if not a.no_replan:
        _replan_section(a, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
