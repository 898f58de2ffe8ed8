#!/usr/bin/env python3
"""Time of the device's TSP table pass (ppgpu_set_tsp_table, ppgpu_set_dubins_tsp_table) and of the host search it replaces, on the
same random lists.

  tools/tsp_table_time.py gpu  [--out FILE] [--variants NAME,..]   GPU box: HIP-event time of the pass for 1 list and for 2 500 lists of n ribbons
  tools/tsp_table_time.py host [--out FILE] [--variants NAME,..]   any box: wall time of the host's pruned search (tests/hostlib) on the first lists

n = 9, 12, 13, 14, 16; TspPointRobotNoSplitAllRibbons and ...KRibbons with K = 2 (All, K=2), TspDubinsNoSplitAllRibbons and ...KRibbons
with K = 2 (DubinsAll, DubinsK=2: the pass of the Dubins switch, the Dubins-length tables of the listed records included).  Lists: seed 1000 n + heuristic, 200 m box, 30 % of
the ribbons pieces of 1-2.5 ribbon widths.  The pass is asked for exactly n ribbons (min = max = n), so it runs whether or not the
enumeration kernels answer that length too."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (9, 12, 13, 14, 16)
VARIANTS = ((1, 0, "All"), (2, 2, "K=2"), (3, 0, "DubinsAll"), (4, 2, "DubinsK=2"))
MANY = 2500


def lists_for(n, heuristic, count, w=1.5):
    from test_tsp_table import random_list
    rng = np.random.default_rng(1000 * n + heuristic)
    poses = np.column_stack([rng.uniform(0, 200, count), rng.uniform(0, 200, count), rng.uniform(0, 2 * np.pi, count)])
    return poses, [random_list(rng, n, w) for _ in range(count)]


def gpu(out, variants):
    from path_planner_amd import api
    from path_planner_amd.types import make_config
    rows = []
    for heuristic, K, name in variants:
        ctx = api.Context(0)
        ctx.set_config(make_config(heuristic=heuristic, tsp_k=K))
        ctx.enable_timing(True)
        set_range = ctx.set_dubins_tsp_table if heuristic in (3, 4) else ctx.set_tsp_table     # each switch serves its own two heuristics
        set_range(0, 16)                                     # the workspace of the planner's setting; the ranges below keep it
        for n in SIZES:
            poses, lists = lists_for(n, heuristic, MANY)
            set_range(n, n)
            row = {"variant": name, "n": n}
            for label, m in (("one", 1), ("many", MANY)):
                ms = []
                for rep in range(6):
                    before = ctx.tsp_table_stats()
                    ctx.heuristic_host(poses[:m], lists[:m])
                    after = ctx.tsp_table_stats()
                    assert after[0] - before[0] + after[1] - before[1] == m
                    ms.append(ctx.last_tsp_table_timing())
                ms = ms[1:]                                  # the first call of a size also lays out the subset list
                row[label] = {"lists": m, "ms_median": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms), "refused": after[1] - before[1]}
            rows.append(row)
            print(json.dumps(row), flush=True)
        # the pass when the listing kernel finds nothing (lists of 9 ribbons, a pass that takes 16 only): what every launch pays
        poses, lists = lists_for(9, heuristic, MANY)
        set_range(16, 16)
        ms = []
        for rep in range(6):
            ctx.heuristic_host(poses, lists)
            ms.append(ctx.last_tsp_table_timing())
        row = {"variant": name, "n": 0, "nothing_listed": {"records": MANY, "ms_median": float(np.median(ms[1:])), "ms_min": min(ms[1:]), "ms_max": max(ms[1:])}}
        rows.append(row)
        print(json.dumps(row), flush=True)
        ctx.close()
    if out:
        with open(out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def host(out, variants, per=3):
    import hostlib
    hostlib.H.pph_set_ribbon_width(1.5)
    rows = []
    for heuristic, K, name in variants:
        for n in SIZES:
            poses, lists = lists_for(n, heuristic, MANY)
            secs = []
            for i in range(per):
                t0 = time.perf_counter()
                hostlib.ribbons_heuristic(lists[i], heuristic, K, poses[i][0], poses[i][1], poses[i][2])
                secs.append(time.perf_counter() - t0)
            row = {"variant": name, "n": n, "host_ms_per_list": [round(1e3 * s, 3) for s in secs]}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if out:
        with open(out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("where", choices=("gpu", "host"))
    ap.add_argument("--out", default="")
    ap.add_argument("--variants", default="", help="comma-separated names out of " + ", ".join(v[2] for v in VARIANTS) + " (default: all)")
    a = ap.parse_args()
    chosen = [v for v in VARIANTS if not a.variants or v[2] in a.variants.split(",")]
    (gpu if a.where == "gpu" else host)(a.out, chosen)
