#!/usr/bin/env python3
"""How long pp_k_trace_cover takes beside pp_k_trace_steps on the same edge lists.

The cfg3 world of tests/cover_replay.py (root + 30 children of config 3, 512 samples): its 40 test edges, and the list of
~9 000 random edges tests/test_gpu_cover_trace.py sends through the prepass route.  Host forms for the small list, device arrays
for the large one; HIP events around each kernel alone (ppgpu_enable_timing, ppgpu_last_cover_trace_timing /
ppgpu_last_trace_timing), the first launch of each shape left out.

    python tools/cover_trace_timing.py [--reps 7] [--out FILE.json]
"""
import argparse
import json
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
    import cover_replay as cr
    from path_planner_amd.types import RESULT_DTYPE, STEP_DTYPE, COVER_DTYPE, COVER_SUMMARY_DTYPE, edge_pack
    tw = cr.cover_world("cfg3")
    ctx = tw.context()
    ctx.enable_timing(True)
    stride = 1504
    out = {"device": torch.cuda.get_device_name(0), "lists": []}
    rng = np.random.default_rng(9)
    ne = 9000
    vi, ti, cb = rng.integers(0, len(tw.verts), ne), rng.integers(0, len(tw.sx), ne), rng.integers(0, 4, ne)
    far = np.hypot(tw.verts["x"][vi] - tw.sx[ti], tw.verts["y"][vi] - tw.sy[ti]) > 2 * tw.cfg.collision_checking_increment
    for name, edges in (("cfg3 test edges", tw.edges), ("cfg3 random edges", edge_pack(vi[far], ti[far], cb[far]))):
        n = len(edges)
        d_e = torch.from_numpy(edges.view(np.int64)).to("cuda:0")
        d_res = torch.zeros(n * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        d_counts = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        d_steps = torch.zeros(n * stride * STEP_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        d_cover = torch.zeros(n * stride * COVER_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        d_summ = torch.zeros(n * COVER_SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ms_cover, ms_steps = [], []
        for rep in range(a.reps + 1):                         # alternating; the first pair grows the workspace
            ctx.trace_cover_list(n, d_e.data_ptr(), d_res.data_ptr(), stride, d_counts.data_ptr(), d_cover.data_ptr(), d_summ.data_ptr())
            tc = ctx.last_cover_trace_timing()
            ctx.trace_edges_list(n, d_e.data_ptr(), d_res.data_ptr(), stride, d_counts.data_ptr(), d_steps.data_ptr())
            ts = ctx.last_trace_timing()
            if rep:
                ms_cover.append(tc)
                ms_steps.append(ts)
        counts = d_counts.cpu().numpy()
        summ = d_summ.cpu().numpy().view(COVER_SUMMARY_DTYPE)
        out["lists"].append({
            "list": name, "edges": n, "steps": int(counts.sum()), "events": int(summ["events"].sum()), "changes": int(summ["changes"].sum()),
            "trace_cover_ms": sorted(ms_cover), "trace_cover_ms_median": float(np.median(ms_cover)),
            "trace_steps_ms": sorted(ms_steps), "trace_steps_ms_median": float(np.median(ms_steps)),
        })
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
