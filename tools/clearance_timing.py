#!/usr/bin/env python3
"""How long pp_k_trace_clearance takes beside pp_k_trace_steps on the same edge lists, and how long the distance map takes to build.

Kernel time: the two lists of tools/contact_trace_timing.py — the 1 024 edges of tests/sweep_worlds.py's count65 and a few thousand
random edges of config 3 from the root and 30 of its children.  Device arrays, HIP events around each kernel alone
(ppgpu_enable_timing, ppgpu_last_clearance_trace_timing / ppgpu_last_trace_timing), the two kernels alternating, the first launch
of each shape left out.  Map build: the two passes together (ppgpu_last_grid_distance_timing) at config 3's 2048 x 2048 grid and at
an empty one of the same size, the worst case for the row pass's outward walk; every build after a ppgpu_set_grid of its own.

    python tools/clearance_timing.py [--reps 7] [--out FILE.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import sweep_worlds as sw
    import test_gpu_trace as tt
    from path_planner_amd import api, workloads
    from path_planner_amd.types import RESULT_DTYPE, STEP_DTYPE, CLEARANCE_DTYPE, CL_BLOCKED, CL_CAPPED, edge_pack
    lists = []
    w = sw.WORLDS["count65"]()
    lists.append(("count65, 1 024 edges", w.context(), w.edges))
    tw = tt.world_binary()
    rng = np.random.default_rng(9)
    ne = 4096
    vi, ti, cb = rng.integers(0, len(tw.verts), ne), rng.integers(0, len(tw.sx), ne), rng.integers(0, 4, ne)
    far = np.hypot(tw.verts["x"][vi] - tw.sx[ti], tw.verts["y"][vi] - tw.sy[ti]) > 2 * tw.cfg.collision_checking_increment
    lists.append(("config 3, random edges", tw.context(), edge_pack(vi[far], ti[far], cb[far])))
    stride = 1504
    lines = ["device: " + torch.cuda.get_device_name(0), "HIP events around the kernel alone, ms; %d launches after a warm-up one, the two kernels alternating" % a.reps]
    for name, ctx, edges in lists:
        ctx.enable_timing(True)
        n = len(edges)
        d_e = torch.from_numpy(edges.view(np.int64)).to("cuda:0")
        d_res = torch.zeros(n * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        d_counts = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        d_steps = torch.zeros(n * stride * STEP_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        d_cl = torch.zeros(n * CLEARANCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ms_cl, ms_steps = [], []
        for rep in range(a.reps + 1):
            ctx.trace_clearance_list(n, d_e.data_ptr(), d_res.data_ptr(), d_counts.data_ptr(), d_cl.data_ptr(), 2.5)
            tc = ctx.last_clearance_trace_timing()
            ctx.trace_edges_list(n, d_e.data_ptr(), d_res.data_ptr(), stride, d_counts.data_ptr(), d_steps.data_ptr())
            ts = ctx.last_trace_timing()
            if rep:
                ms_cl.append(tc)
                ms_steps.append(ts)
        counts = d_counts.cpu().numpy()
        cl = d_cl.cpu().numpy().view(CLEARANCE_DTYPE)
        lines.append("%s: %d edges, %d steps, margin 2.5 m: %d steps below it, %d edges blocked, %d capped" %
                     (name, n, int(counts.sum()), int(cl["below_steps"].sum()), int(np.count_nonzero(cl["flags"] & CL_BLOCKED)),
                      int(np.count_nonzero(cl["flags"] & CL_CAPPED))))
        lines.append("  pp_k_trace_clearance  median %.4f  (%s)" % (float(np.median(ms_cl)), " ".join("%.4f" % v for v in sorted(ms_cl))))
        lines.append("  pp_k_trace_steps      median %.4f  (%s)" % (float(np.median(ms_steps)), " ".join("%.4f" % v for v in sorted(ms_steps))))
    lines.append("distance map, pp_k_dist_cols + pp_k_dist_rows together, ms; %d builds after a warm-up one, each after its own ppgpu_set_grid "
                 "(pp_k_grid_row_clear + pp_k_grid_clear of the same size: 0.27)" % a.reps)
    g3 = workloads.config3(n_samples=16, n_obst=0).grid
    ctx = api.Context(0)
    ctx.enable_timing(True)
    for name, grid in (("config 3's 2048 x 2048 grid, %.1f %% blocked" % (100.0 * float(np.mean(g3 != 0))), g3), ("empty 2048 x 2048 grid", np.zeros_like(g3))):
        ms = []
        for rep in range(a.reps + 1):
            ctx.set_grid(grid, 0.1)
            _, g2 = ctx.grid_clearance_at(np.array([[102.4, 102.4]]))
            if rep:
                ms.append(ctx.last_grid_distance_timing())
        far = ctx.get_grid_distance(*grid.shape)
        lines.append("  %s: median %.4f  (%s); largest gap2 %d" % (name, float(np.median(ms)), " ".join("%.4f" % v for v in sorted(ms)), int(far.max())))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
