#!/usr/bin/env python3
"""One ppgpu_cost_plans_host call against the same legs costed depth by depth with host hand-over.

4 096 plans of 6 legs each from the root of config 3 turned to 16 headings (waypoints a few metres ahead, so that most plans walk all six legs), costed
  (a) by one chain call, and
  (b) depth by depth in the same process: ppgpu_set_vertices + ppgpu_cost_wrapper_edges_host for the legs of one depth, the next
      depth's vertices and ribbon pool built on the host from the records (vectorised numpy), as many round trips as the plan is deep.
Both routes are checked to give the same bytes, warmed up, then timed in alternation (wall clock around the synchronous calls).

    python tools/chain_timing.py [--plans 4096] [--legs 6] [--reps 7] [--stride 16] [--out FILE.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


N_STARTS = 16


def start_vertices(w):
    """The root's pose turned to 16 headings: plans fan out instead of all meeting the same blocked cells ahead of the root."""
    v = np.repeat(w.root(), N_STARTS)
    v["heading"] = np.arange(N_STARTS) * (2 * math.pi / N_STARTS)
    v["ribbon_offset"] = 0                                      # every start vertex shares the root's ribbon list
    return v


def build(w, world, n_plans, n_legs, seed=11):
    import oracle as orc
    from path_planner_amd.types import WRAPPER_EDGE_DTYPE
    cfg = w.cfg
    rng = np.random.default_rng(seed)
    starts = start_vertices(w)
    legs = np.zeros((n_plans, n_legs), dtype=WRAPPER_EDGE_DTYPE)
    for p in range(n_plans):
        sv = p % N_STARTS
        x, y, hdg, t = float(starts["x"][sv]), float(starts["y"][sv]), float(starts["heading"][sv]), float(starts["time"][sv])
        for k in range(n_legs):
            rho = float(rng.choice([cfg.turning_radius, cfg.coverage_turning_radius]))
            for _ in range(8):
                d, kap = float(rng.uniform(4.0, 9.0)), float(rng.uniform(-0.05, 0.05))
                y0 = math.pi / 2 - hdg
                if abs(kap) < 1e-6:
                    kap = 1e-6
                along = [d * f for f in (0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0)]
                px = [x + (math.sin(y0 + kap * a) - math.sin(y0)) / kap for a in along]
                py = [y - (math.cos(y0 + kap * a) - math.cos(y0)) / kap for a in along]
                tx, ty = px[-1], py[-1]
                if not world.is_blocked(px, py).any():      # (the arc, not the Dubins curve: most legs come out feasible, not all)
                    break
            err, p8 = orc.dubins_shortest_path([x, y, y0], [tx, ty, y0 + kap * d], rho)
            assert err == 0
            end = float(orc.O.ppo_wrapper_fill_end_time(p8.ctypes.data, cfg.max_speed, t))
            legs[p, k] = (sv, 1 if rho == cfg.coverage_turning_radius else 0, p8[0:3], p8[3:6], rho, int(p8[7]), 0, cfg.max_speed, t, end)
            x, y, hdg, t = tx, ty, (math.pi / 2 - (y0 + kap * d)) % (2 * math.pi), end
    return legs


def depth_by_depth(ctx, verts, pool, legs, stride):
    from path_planner_amd import types as T
    n_plans, n_legs = legs.shape
    res = np.zeros((n_plans, n_legs), dtype=T.RESULT_DTYPE)
    child = np.zeros((n_plans, n_legs, stride, 4))
    costed = np.zeros(n_plans, dtype=np.int32)
    live = np.arange(n_plans)
    r = c = None
    ends = T.F_THROWS | T.F_DUBINS_ERR | T.F_RIBBON_LOST | T.F_INFEASIBLE | T.F_GOAL
    for d in range(n_legs):
        we = np.ascontiguousarray(legs[live, d])
        if d == 0:
            ctx.set_vertices(verts, pool)
        else:
            nr = ((r["info"] >> 8) & 0xFF).astype(np.int32)
            v = np.zeros(len(live), dtype=T.VERTEX_DTYPE)
            for a, b in (("x", "end_x"), ("y", "end_y"), ("heading", "end_heading"), ("speed", "end_speed"), ("time", "end_time"), ("g", "g"),
                         ("coverage_completed_time", "coverage_completed_time")):
                v[a] = r[b]
            v["ribbon_offset"] = np.cumsum(nr) - nr
            v["ribbon_count"] = nr
            ctx.set_vertices(v, c[np.arange(stride)[None, :] < nr[:, None]])
            we["vertex"] = np.arange(len(live))
        r, c = ctx.cost_wrapper_edges_host(we, stride=stride)
        res[live, d] = r
        child[live, d] = c
        costed[live] = d + 1
        go = ((r["flags"] & ends) == 0) & (((r["info"] >> 8) & 0xFF) <= stride)
        live, r, c = live[go], r[go], c[go]
        if len(live) == 0:
            break
    return res, child, costed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", type=int, default=4096)
    ap.add_argument("--legs", type=int, default=6)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--stride", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import oracle as orc
    from path_planner_amd import api, workloads
    w = workloads.config3(n_samples=512)
    world = orc.World(w.cfg, w.grid, w.res, w.obst)
    legs = build(w, world, a.plans, a.legs)
    offs = np.arange(a.plans + 1, dtype=np.int32) * a.legs
    flat = np.ascontiguousarray(legs.reshape(-1))
    ctx = api.Context(0)
    ctx.set_config(w.cfg)
    ctx.set_grid(w.grid, w.res)
    ctx.set_obstacles(w.obst)
    verts, pool = start_vertices(w), w.ribbons4

    def chain():
        ctx.set_vertices(verts, pool)
        return ctx.cost_plans(offs, flat, a.stride)

    res, child, costed, stop = chain()
    dres, dchild, dcosted = depth_by_depth(ctx, verts, pool, legs, a.stride)
    assert np.array_equal(costed, dcosted)
    done = np.arange(a.legs)[None, :] < costed[:, None]
    assert res.reshape(a.plans, a.legs)[done].tobytes() == dres[done].tobytes(), "the two routes differ"
    assert child.reshape(a.plans, a.legs, a.stride, 4)[done].tobytes() == dchild[done].tobytes(), "the two routes differ (child ribbons)"
    for _ in range(2):                                          # warm-up (the first calls grow the handle's buffers)
        chain()
        depth_by_depth(ctx, verts, pool, legs, a.stride)
    t_chain, t_depth = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter(); chain(); t_chain.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter(); depth_by_depth(ctx, verts, pool, legs, a.stride); t_depth.append(1e3 * (time.perf_counter() - t0))
    out = {
        "plans": a.plans, "legs_per_plan": a.legs, "ribbon_stride": a.stride, "legs_costed": int(costed.sum()),
        "plans_walked_to_the_end": int(np.sum(costed == a.legs)), "stop_codes": np.bincount(stop, minlength=6).tolist(),
        "chain_call_ms": sorted(t_chain), "chain_call_ms_median": float(np.median(t_chain)),
        "depth_by_depth_ms": sorted(t_depth), "depth_by_depth_ms_median": float(np.median(t_depth)),
        "depth_over_chain": float(np.median(t_depth) / np.median(t_chain)),
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
