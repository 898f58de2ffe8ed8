"""-m gpu: the worlds of tests/sweep_worlds.py on the device against the oracle.  Three conservative filters sit in front of the exact
box test (omask from pp_k_solve_edges, the chord test of pp_k_plan_skips, the per-chunk culling of the pose sweep) and the cover
sweep sums what they left; a bound that is slightly too small loses a hit on one edge in thousands and changes a long edge's
penalty by less than REL_TOL.  So on binary fleets the penalty must be the oracle's to the bit (hits x 600: every partial sum is an
integer below 2^53, no order of summation can change it), on both routes: PPGPU_PREPASS_MIN_EDGES=0 (skip planner on) and huge
(every chunk sampled).  tests/test_sweep_worlds.py shows on the oracle alone that the worlds hold the cases."""
import numpy as np
import pytest

import sweep_worlds as sw

pytestmark = pytest.mark.gpu

ROUTES = ("0", "1000000000")         # PPGPU_PREPASS_MIN_EDGES: the skip planner runs / every chunk is sampled


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _dense(torch, ctx, w):
    from path_planner_amd import api
    from path_planner_amd.types import RESULT_DTYPE
    ne = api.Context.dense_edge_count(1, w.ns, sw.MASK)
    assert ne == len(w.edges)
    d_res = torch.zeros(ne * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    d_child = torch.zeros(ne * sw.RIBBON_STRIDE * 4, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()      # the fill ran on torch's stream, the library works on its own
    ctx.cost_edges_dense(0, 1, 0, w.ns, sw.MASK, d_res.data_ptr(), d_child.data_ptr(), sw.RIBBON_STRIDE)
    ctx.synchronize()
    return d_res.cpu().numpy().view(RESULT_DTYPE), d_child.cpu().numpy().reshape(ne, sw.RIBBON_STRIDE, 4)


def _run(torch, monkeypatch, w, route):
    """(handle, records, child ribbons) of world w through one route; the handle reads the switches when it is created."""
    monkeypatch.setenv("PPGPU_PREPASS_MIN_EDGES", route)
    ctx = w.context()
    gpu, gchild = _dense(torch, ctx, w)
    return ctx, gpu, gchild


def _against_oracle(what, gpu, gchild, cpu, cchild, exact):
    from parity import compare_results
    from path_planner_amd.types import F_INFEASIBLE
    rep = compare_results(gpu, cpu, gchild, cchild)
    feas = (cpu["flags"] & F_INFEASIBLE) == 0
    lost = feas & (gpu["collision_penalty"] != cpu["collision_penalty"])
    print(what, {k: rep[k] for k in ("n_feasible", "worst_rel", "n_flag_mismatch", "n_info_mismatch")}, "penalties that differ:", int(lost.sum()))
    assert rep["ok"], (what, rep)
    if exact:
        assert np.array_equal(gpu["flags"], cpu["flags"]), what
        assert np.array_equal(gpu["info"], cpu["info"]), what
        bad = np.nonzero(lost)[0]
        assert bad.size == 0, (what, "edges", bad[:8].tolist(), "device hits", (gpu["collision_penalty"][bad[:8]] / 600.0).tolist(),
                               "oracle hits", (cpu["collision_penalty"][bad[:8]] / 600.0).tolist())


def _same_answers(a, b, what):
    for f in ("flags", "info", "collision_penalty"):
        bad = np.nonzero(a[f] != b[f])[0]
        assert bad.size == 0, (what, f, bad[:8].tolist(), a[f][bad[:8]].tolist(), b[f][bad[:8]].tolist())


def _trace_check(ctx, w, gpu, pick, stride):
    """The step trace does not skip: as many records as info says, and its running penalty is the record's, exactly."""
    cpf = w.cfg.collision_penalty_factor
    rec, counts, st = ctx.trace_edges(w.edges[pick], stride)
    assert np.array_equal(counts, (gpu["info"][pick] >> 16).astype(counts.dtype)), "trace records per edge != info >> 16"
    has = np.nonzero(counts > 0)[0]
    last = st[has, counts[has] - 1]
    assert np.array_equal(last["penalty_before"] + last["collision"] * cpf, gpu["collision_penalty"][pick][has]), "running penalty != the record's"
    assert np.all(gpu["collision_penalty"][pick][counts == 0] == 0.0)


TRACED = ("fast", "stacked", "done_inside")


# ---------------------------------------------------------------------------------------------- binary fleets, 1 501 steps
@pytest.mark.parametrize("name", sw.BINARY + ["done_inside"])
def test_binary_fleet_against_oracle(torch_cuda, monkeypatch, name):
    """Both routes: the oracle's flags and info on every edge, its penalty to the bit on every feasible edge, and the same answers
    from both.  `count64+far` against `count64`: a box 10 km away switches
    every kernel to its more-than-64 path and may change no answer."""
    w, cpu, cchild = sw.oracle_records(name)
    outs = []
    for route in ROUTES:
        ctx, gpu, gchild = _run(torch_cuda, monkeypatch, w, route)
        _against_oracle("%s route %s" % (name, route), gpu, gchild, cpu, cchild, exact=True)
        if name in TRACED:
            # (an odd stride: an edge's configuration is its index % 4, so all four speeds and radii are traced)
            ne = len(w.edges)
            stride = (ne // 128) | 1
            pick = np.arange(0, ne, stride)[:128]
            assert len(np.unique(pick % 4)) == 4
            _trace_check(ctx, w, gpu, pick, w.ng)
        if name == "count64+far":
            w64, cpu64, _ = sw.oracle_records("count64")
            _same_answers(cpu, cpu64, "oracle: the far box changed an answer")
            _, g64, _ = _run(torch_cuda, monkeypatch, w64, route)
            _same_answers(gpu, g64, "count64+far against count64, route " + route)
        outs.append(gpu)
    _same_answers(outs[0], outs[1], name + ": skip planner on / off")


# ---------------------------------------------------------------------------------------------- Gaussian counterparts
@pytest.mark.parametrize("name", sw.GAUSSIAN)
def test_gaussian_fleet_against_oracle(torch_cuda, monkeypatch, name):
    """Sums of doubles: the project's tolerance on both routes, nothing tighter."""
    w, cpu, cchild = sw.oracle_records("gaussian_" + name)
    assert not w.binary and float(cpu["collision_penalty"].max()) > 0.0
    for route in ROUTES:
        _, gpu, gchild = _run(torch_cuda, monkeypatch, w, route)
        _against_oracle("gaussian_%s route %s" % (name, route), gpu, gchild, cpu, cchild, exact=False)


# ---------------------------------------------------------------------------------------------- more than 256 chunks per edge
@pytest.mark.parametrize("steps", sw.LONG_STEPS)
def test_long_horizon_against_oracle(torch_cuda, monkeypatch, steps):
    """Time rows of 256, 257 and 258 chunks: pp_k_plan_skips with one edge per workgroup, the pose walk through four and five groups
    of 64 skip bytes, the cover sweep's sums over hundreds of chunks.  16 376: the row fills the planner's one tile of 256 chunks
    exactly.  16 377: a second tile (blockIdx.y = 1) is launched for one chunk, but the longest edge has 16 378 steps, all in the
    first 256 chunks, so that tile's thread leaves at once (the sweep never reaches its chunk): what is checked is that it
    disturbs nothing.  Only 16 500 has edges past step 16 384 (12 of them): there the second tile decides chunks 256 and 257 and
    the walk enters a fifth group."""
    w, cpu, cchild = sw.oracle_records("long%d" % steps)
    assert w.ng == steps + 8
    nsteps = cpu["info"] >> 16
    nch = (nsteps.astype(np.int64) + 63) // 64
    print("long", steps, "chunks of the longest edge", int(nch.max()), "edges past the second group of 64 chunks", int((nch > 128).sum()),
          "past the fourth", int((nch > 256).sum()))
    outs = []
    for route in ROUTES:
        ctx, gpu, gchild = _run(torch_cuda, monkeypatch, w, route)
        _against_oracle("long%d route %s" % (steps, route), gpu, gchild, cpu, cchild, exact=True)
        if steps == 16500:
            beyond = np.nonzero(nsteps > 16384)[0]
            assert beyond.size >= 5
            _trace_check(ctx, w, gpu, beyond[:16], steps + 8)
        outs.append(gpu)
    _same_answers(outs[0], outs[1], "long%d: skip planner on / off" % steps)
