#!/usr/bin/env python3
"""GPU box (run under rocprofv3 --kernel-trace --stats): the expand-order pipeline on 16 open vertices at several sample counts.
usage: tools/time_expand_order.py [attempts] [k] [one_radius]   (k = 9 by default; one_radius: coverage radius = turning radius).  The line it prints ends in a sha256 of the winners:
two libraries (PPGPU_LIB_OVERRIDE) that compute the same print the same line."""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from path_planner_amd import api, workloads
from path_planner_amd.types import RESULT_DTYPE, VERTEX_DTYPE, F_INFEASIBLE
n_samples = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
k_nearest = int(sys.argv[2]) if len(sys.argv) > 2 else 9
w = workloads.config3()
if "one_radius" in sys.argv[3:]:
    w.cfg.coverage_turning_radius = w.cfg.turning_radius
ctx = api.Context(0)
ctx.set_config(w.cfg); ctx.set_grid(w.grid, w.res); ctx.set_obstacles(w.obst); ctx.set_vertices(w.root(), w.ribbons4)
ctx.sampler_init(w.bounds6, w.seed, w.ribbons4)
for first in range(0, n_samples, 1 << 19):                  # (the sampler takes at most 524 288 attempts per call)
    n = ctx.sampler_add(min(1 << 19, n_samples - first))
e = np.arange(64, dtype=np.uint64) * 4
res, child = ctx.cost_edges_host(e, stride=12)
ok = np.nonzero((res["flags"] & F_INFEASIBLE) == 0)[0][:15]
v = np.zeros(len(ok) + 1, dtype=VERTEX_DTYPE); pool = [np.asarray(w.ribbons4).reshape(-1, 4)]; v[0] = w.root()[0]; off = len(pool[0])
for k, i in enumerate(ok):
    r, nr = res[i], int((res[i]["info"] >> 8) & 0xFF)
    v[k + 1] = (r["end_x"], r["end_y"], r["end_heading"], r["end_speed"], r["end_time"], r["g"], r["coverage_completed_time"], off, nr)
    pool.append(child[i, :nr]); off += nr
ctx.set_vertices(v, np.concatenate(pool))
for _ in range(10):
    idx, fb = ctx.expand_order(len(v), k_nearest)
print("samples", n, "vertices", len(v), "k", k_nearest, "fallbacks", fb, "idx sha256", hashlib.sha256(np.ascontiguousarray(idx).tobytes()).hexdigest()[:16])
