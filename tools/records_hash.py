"""Developer tool (GPU box): sha256 of the records and child ribbons of one costing launch of the bench workload (config 3, dense
from the root) — to check that a variant build (PPGPU_LIB_OVERRIDE) produces the same bytes as the default one.

    records_hash.py [n_samples] [--heuristic N [--tsp-k K]] [--gaussian]
                                     the costing launch; under heuristic N of ppgpu.h (0 MaxDistance .. 4 Dubins K) and branching K
                                     instead of config 3's own, with the obstacles as Gaussian rows instead of boxes
    records_hash.py --traces         the three edge traces instead: results, counts, records, summaries and final lists of the step,
                                     cover and contact traces over the test worlds (test_gpu_trace's world_binary and custom-covariance
                                     Gaussian world, cover_replay's cfg3, sweep_worlds' count65, contact_replay's edges_world with its
                                     wrapper-form edges), as one slice and with the slice budgets of test_sliced_trace_is_bit_identical"""
import sys, os, hashlib
sys.path.insert(0, os.getcwd())
import numpy as np, torch
from path_planner_amd import api, workloads

LIB = os.environ.get("PPGPU_LIB_OVERRIDE", "default")


def _option(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def costing(n_samples):
    w = workloads.config3(n_samples=n_samples)
    w.cfg.heuristic, w.cfg.tsp_k = _option("--heuristic", w.cfg.heuristic), _option("--tsp-k", w.cfg.tsp_k)
    gaussian = "--gaussian" in sys.argv
    ctx = api.Context(0)
    ctx.set_config(w.cfg); ctx.set_grid(w.grid, w.res)
    if gaussian:
        ctx.set_gaussian_obstacles(np.ascontiguousarray(w.obst[:, :5]))
    else:
        ctx.set_obstacles(w.obst)
    ctx.set_vertices(w.root(), w.ribbons4)
    ctx.sampler_init(w.bounds6, w.seed, w.ribbons4); n = ctx.sampler_add(w.n_samples)
    d = torch.zeros(4 * n * 128, dtype=torch.uint8, device="cuda")
    ch = torch.zeros(4 * n * 8 * 4, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.cost_edges_dense(0, 1, 0, n, 0xF, d.data_ptr(), ch.data_ptr(), 8); ctx.synchronize()
    print(LIB, n, "heuristic %d k %d%s" % (w.cfg.heuristic, w.cfg.tsp_k, " gaussian" if gaussian else ""), hashlib.sha256(d.cpu().numpy().tobytes()).hexdigest()[:16], hashlib.sha256(ch.cpu().numpy().tobytes()).hexdigest()[:16])


def _sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def traces():
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    import contact_replay, cover_replay, sweep_worlds, test_gpu_trace
    stride, ribbons = test_gpu_trace.STRIDE, 16
    worlds = [("world_binary", test_gpu_trace.world_binary()), ("world_gaussian_custom", test_gpu_trace.world_gaussian("custom")),
              ("cover_cfg3", cover_replay.cover_world("cfg3")), ("sweep_count65", sweep_worlds.WORLDS["count65"]()),
              ("edges_world", contact_replay.edges_world())]
    for budget in (None, 24 << 10, 400 << 10):
        if budget is not None:
            os.environ["PPGPU_SLICE_BYTES"] = str(budget)      # (a handle reads it when it is created)
        form = "one slice" if budget is None else "slices of %d KB" % (budget >> 10)
        for name, w in worlds:
            ctx = w.context()
            out = [("steps", ctx.trace_edges(w.edges, stride)), ("cover", ctx.trace_cover(w.edges, stride, ribbon_stride=ribbons)),
                   ("contacts", ctx.trace_contacts(w.edges))]
            if hasattr(w, "wedges"):
                out += [("wrapper steps", ctx.trace_wrapper_edges(w.wedges, stride)),
                        ("wrapper cover", ctx.trace_cover_wrapper_edges(w.wedges, stride, ribbon_stride=ribbons)),
                        ("wrapper contacts", ctx.trace_contacts_wrapper_edges(w.wedges))]
            for kind, arrays in out:
                print("%-22s %-18s %-17s edges %5d steps %8d  %s" % (name, form, kind, len(arrays[1]), int(arrays[1].sum()), _sha(arrays)))
    print(LIB)


if __name__ == "__main__":
    if "--traces" in sys.argv[1:]:
        traces()
    else:
        costing(int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 65536)
