#!/usr/bin/env python3
"""How long pp_k_trace_contacts takes beside pp_k_trace_steps on the same edge lists.

Two lists: the 1 024 edges of tests/sweep_worlds.py's count65 (65 boxes: two passes of obstacle rows per edge), and a few thousand
random edges of config 3 (16 boxes: a quarter of the wave in the kernel's second phase) from the root and 30 of its children, the
world of tests/test_gpu_trace.py.  Device arrays, HIP events around each kernel alone (ppgpu_enable_timing,
ppgpu_last_contact_trace_timing / ppgpu_last_trace_timing), the two kernels alternating, the first launch of each shape left out.

    python tools/contact_trace_timing.py [--reps 7] [--out FILE.txt]
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
    from path_planner_amd.types import RESULT_DTYPE, STEP_DTYPE, CONTACT_DTYPE, edge_pack
    lists = []
    w = sw.WORLDS["count65"]()
    lists.append(("count65, 1 024 edges, 65 boxes", w.context(), w.edges))
    tw = tt.world_binary()
    rng = np.random.default_rng(9)
    ne = 4096
    vi, ti, cb = rng.integers(0, len(tw.verts), ne), rng.integers(0, len(tw.sx), ne), rng.integers(0, 4, ne)
    far = np.hypot(tw.verts["x"][vi] - tw.sx[ti], tw.verts["y"][vi] - tw.sy[ti]) > 2 * tw.cfg.collision_checking_increment
    lists.append(("config 3, random edges, 16 boxes", tw.context(), edge_pack(vi[far], ti[far], cb[far])))
    stride = 1504
    lines = ["device: " + torch.cuda.get_device_name(0), "HIP events around the kernel alone, ms; %d launches after a warm-up one, the two kernels alternating" % a.reps]
    for name, ctx, edges in lists:
        ctx.enable_timing(True)
        n, nob = len(edges), ctx.obstacle_count()[0]
        d_e = torch.from_numpy(edges.view(np.int64)).to("cuda:0")
        d_res = torch.zeros(n * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        d_counts = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        d_steps = torch.zeros(n * stride * STEP_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        d_con = torch.zeros(n * nob * CONTACT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ms_con, ms_steps = [], []
        for rep in range(a.reps + 1):
            ctx.trace_contacts_list(n, d_e.data_ptr(), d_res.data_ptr(), d_counts.data_ptr(), d_con.data_ptr())
            tc = ctx.last_contact_trace_timing()
            ctx.trace_edges_list(n, d_e.data_ptr(), d_res.data_ptr(), stride, d_counts.data_ptr(), d_steps.data_ptr())
            ts = ctx.last_trace_timing()
            if rep:
                ms_con.append(tc)
                ms_steps.append(ts)
        counts = d_counts.cpu().numpy()
        con = d_con.cpu().numpy().view(CONTACT_DTYPE)
        lines.append("%s: %d edges, %d steps, %d step-contact pairs, %d records with a hit" %
                     (name, n, int(counts.sum()), int(counts.sum()) * nob, int(np.count_nonzero(con["hit_steps"]))))
        lines.append("  pp_k_trace_contacts  median %.4f  (%s)" % (float(np.median(ms_con)), " ".join("%.4f" % v for v in sorted(ms_con))))
        lines.append("  pp_k_trace_steps     median %.4f  (%s)" % (float(np.median(ms_steps)), " ".join("%.4f" % v for v in sorted(ms_steps))))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
