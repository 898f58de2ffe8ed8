"""Developer tool (GPU box): N costing launches of the bench workload (config 3, dense from the root) with a configuration mask of
the caller's choice, for a profiler to time — mask 0x1 (configuration 0 only) is the launch with nothing to share of
profiles/shared_sweeps.txt block 5 and profiles/solve_icache.txt.  Prints the launch's counts.

    launch_mask.py [mask] [launches]      (PPGPU_LIB_OVERRIDE picks the library)"""
import sys, os
sys.path.insert(0, os.getcwd())
import torch
from path_planner_amd import api, workloads

mask = int(sys.argv[1], 0) if len(sys.argv) > 1 else 0x1
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 10
w = workloads.config3(n_samples=65536)
ctx = api.Context(0)
ctx.set_config(w.cfg); ctx.set_grid(w.grid, w.res); ctx.set_obstacles(w.obst)
ctx.set_vertices(w.root(), w.ribbons4)
ctx.sampler_init(w.bounds6, w.seed, w.ribbons4); n = ctx.sampler_add(w.n_samples)
ne = api.Context.dense_edge_count(1, n, mask)
d = torch.zeros(ne * 128, dtype=torch.uint8, device="cuda")
ch = torch.zeros(ne * 8 * 4, dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
for _ in range(launches):
    ctx.cost_edges_dense(0, 1, 0, n, mask, d.data_ptr(), ch.data_ptr(), 8)
ctx.synchronize()
print("lib", os.environ.get("PPGPU_LIB_OVERRIDE", "default"), "mask", hex(mask), "edges", ne, "shared", ctx.last_shared_edges(), "cover", ctx.last_cover_edges())
