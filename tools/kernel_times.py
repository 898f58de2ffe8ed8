"""Developer tool (GPU box): per-kernel HIP-event times of one costing launch of the bench workload (config 3, dense from the
root); PPGPU_LIB_OVERRIDE selects a variant library.

    kernel_times.py                  the bench workload as it is: pp_k_pose_sweep, the fused heuristic
    kernel_times.py --gaussian       config 3's 16 obstacles as Gaussian rows {x, y, heading, speed, time} with the default covariance:
                                     pp_k_pose_sweep_gaussian, pp_k_cover_sweep_gaussian and, for the point heuristics, pp_k_heuristic
    kernel_times.py --heuristic N    heuristic N of ppgpu.h (0 MaxDistance, 1 / 2 TspPointRobotNoSplit All / K ribbons, 3 / 4
                                     TspDubinsNoSplit All / K ribbons: pp_k_heuristic_dubins)"""
import argparse, sys, os
sys.path.insert(0, os.getcwd())
import numpy as np, torch
from path_planner_amd import api, workloads
ap = argparse.ArgumentParser()
ap.add_argument("--gaussian", action="store_true")
ap.add_argument("--heuristic", type=int, default=None)
args = ap.parse_args()
w = workloads.config3()
if args.heuristic is not None:
    w.cfg.heuristic = args.heuristic
ctx = api.Context(0)
st = torch.cuda.Stream(); torch.cuda.set_stream(st); ctx.set_stream(st.cuda_stream)
ctx.set_config(w.cfg); ctx.set_grid(w.grid, w.res)
if args.gaussian:
    ctx.set_gaussian_obstacles(np.ascontiguousarray(w.obst[:, :5]))
else:
    ctx.set_obstacles(w.obst)
ctx.set_vertices(w.root(), w.ribbons4)
ctx.sampler_init(w.bounds6, w.seed, w.ribbons4); n = ctx.sampler_add(w.n_samples)
d = torch.zeros(4*n*128, dtype=torch.uint8, device="cuda")
ctx.enable_timing(True)
ts=[]
for i in range(5):
    ctx.cost_edges_dense(0,1,0,n,0xF,d.data_ptr()); ts.append(ctx.last_timing())
what = ("gaussian " if args.gaussian else "") + ("heuristic %d " % args.heuristic if args.heuristic is not None else "")
print(os.environ.get("PPGPU_LIB_OVERRIDE","default"), what, " solve/pose/cover/heur ms:", np.round(np.min(np.array(ts[1:]),axis=0),3))
