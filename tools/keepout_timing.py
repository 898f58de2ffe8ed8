#!/usr/bin/env python3
"""What a change of the keep-out limit costs on the device: pp_k_keepout_bits plus the rebuild of the chessboard clearance map over
the effective grid (ppgpu_last_keepout_timing: HIP events on the handle's stream around the three kernels), and the wall time of the
whole ppgpu_set_keepout_limit2 call, which also waits for the stream twice.  Config 3's 2048 x 2048 grid; the distance map is built
before the first timed change, so no change pays for it.

    python tools/keepout_timing.py [--reps 7] [--out FILE.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from path_planner_amd import api, workloads
    w = workloads.config3(n_samples=16, n_obst=0)
    ctx = api.Context(0)
    ctx.set_config(w.cfg)
    ctx.enable_timing(True)
    ctx.set_grid(w.grid, w.res)
    ctx.get_grid_distance(*w.grid.shape)
    dist_ms = ctx.last_grid_distance_timing()
    lines = ["device: " + torch.cuda.get_device_name(0),
             "config 3's %d x %d grid at %.2f m, %.1f %% blocked; distance map built once before (%.4f ms); %d changes after a warm-up one" %
             (w.grid.shape[0], w.grid.shape[1], w.res, 100.0 * float(np.mean(w.grid != 0)), dist_ms, a.reps),
             "device: ppgpu_last_keepout_timing, ms (pp_k_keepout_bits + pp_k_grid_row_clear + pp_k_grid_clear; back to 0: the rebuild alone)",
             "call:   wall time of ppgpu_set_keepout_limit2, ms"]
    walk = [(4, 9), (9, 2500), (2500, 0), (0, 4)]
    for was, now in walk:
        dev, wall = [], []
        for rep in range(a.reps + 1):
            ctx.set_keepout_limit2(was)
            t0 = time.perf_counter()
            ctx.set_keepout_limit2(now)
            t1 = time.perf_counter()
            if rep:
                dev.append(ctx.last_keepout_timing())
                wall.append(1e3 * (t1 - t0))
        blocked = float(np.mean(ctx.get_grid_blocked(*w.grid.shape) != 0))
        lines.append("  limit2 %5d -> %5d (%.1f %% of the cells blocked after): device median %.4f (%s)  call median %.4f" %
                     (was, now, 100.0 * blocked, float(np.median(dev)), " ".join("%.4f" % v for v in sorted(dev)), float(np.median(wall))))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
