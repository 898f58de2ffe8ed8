#!/usr/bin/env python3
"""How long pp_k_trace_steps takes against its own floor, the bytes it writes.

One launch of 8 192 edges that run the whole horizon (an empty grid, slow-speed edges to far targets: 1 501 steps each, 64 bytes per
step, ~790 MB), timed with HIP events around the kernel alone (ppgpu_enable_timing / ppgpu_last_trace_timing), and in the same
process a hipMemsetAsync over the same number of bytes: the yardstick, not code under test.

    python tools/trace_timing.py [--edges 8192] [--reps 7] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _loaded_hip():
    """The HIP runtime this process already uses (torch's), by path: a second copy of the runtime must not be loaded."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if os.path.basename(path).startswith("libamdhip64.so"):
            return C.CDLL(path)
    raise RuntimeError("no libamdhip64.so is mapped")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from path_planner_amd import api, workloads
    from path_planner_amd.types import RESULT_DTYPE, STEP_DTYPE, edge_pack
    w = workloads.config3(n_samples=4096)
    ctx = api.Context(0)
    ctx.set_config(w.cfg)
    ctx.set_grid(np.zeros_like(w.grid), w.res)               # nothing blocked: every edge runs until the horizon
    ctx.set_obstacles(w.obst)
    ctx.set_vertices(w.root(), w.ribbons4)
    ctx.sampler_init(w.bounds6, w.seed, w.ribbons4)
    n = ctx.sampler_add(w.n_samples)
    s = ctx.get_samples()
    root = w.root()
    far = np.nonzero(np.hypot(s[:, 0] - root["x"][0], s[:, 1] - root["y"][0]) > 25.0)[0]      # > 30 s at 0.5 m/s
    tgt = np.resize(far, a.edges)
    edges = edge_pack(np.zeros(a.edges, dtype=np.uint64), tgt, np.where(np.arange(a.edges) % 2 == 0, 2, 3))
    stride = 1504
    d_e = torch.from_numpy(edges.view(np.int64)).to("cuda:0")
    d_res = torch.zeros(a.edges * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    d_counts = torch.zeros(a.edges, dtype=torch.int32, device="cuda:0")
    d_steps = torch.zeros(a.edges * stride * STEP_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.enable_timing(True)
    ms = []
    for rep in range(a.reps + 1):
        ctx.trace_edges_list(a.edges, d_e.data_ptr(), d_res.data_ptr(), stride, d_counts.data_ptr(), d_steps.data_ptr())
        t = ctx.last_trace_timing()
        if rep:                                                # the first launch grows the workspace
            ms.append(t)
    counts = d_counts.cpu().numpy()
    nbytes = int(counts.sum()) * STEP_DTYPE.itemsize
    hip = _loaded_hip()
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipMemsetAsync.restype = C.c_int
    stream = torch.cuda.current_stream()
    fill = []
    for rep in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = hip.hipMemsetAsync(C.c_void_p(d_steps.data_ptr()), 0, C.c_size_t(nbytes), C.c_void_p(stream.cuda_stream))
        e1.record(stream)
        assert rc == 0, rc
        e1.synchronize()
        if rep:
            fill.append(e0.elapsed_time(e1))
    out = {
        "edges": a.edges, "steps": int(counts.sum()), "steps_per_edge_min": int(counts.min()), "steps_per_edge_max": int(counts.max()),
        "bytes": nbytes,
        "trace_kernel_ms": sorted(ms), "trace_kernel_ms_median": float(np.median(ms)),
        "memset_ms": sorted(fill), "memset_ms_median": float(np.median(fill)),
        "trace_over_memset": float(np.median(ms) / np.median(fill)),
        "trace_GBps": nbytes / np.median(ms) / 1e6, "memset_GBps": nbytes / np.median(fill) / 1e6,
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
