"""-m gpu: the skip planner's span masks and shared boundary poses (pp_k_plan_skips) against the chunkwise planner it replaces
(PPGPU_PLAN_SPANS=0, the same library) and against the oracle.  The planner only decides what the pose sweep need not sample, and what
it stores for a skipped chunk is what sampling would have stored: so both planners must leave the same bytes in every record and
child ribbon, whichever chunks each of them skips (the off-power worlds among them: turning radii without an exact reciprocal, where
both take their d / rho forms).  The worlds of tests/sweep_worlds_spans.py (boxes that graze an edge for a few
steps; time rows of less than one span, exactly one, one or two and a short one) are also held to the oracle with the bar of
tests/test_gpu_sweep_inputs.py: flags and info equal, on binary fleets the penalty of every feasible edge equal to the bit, with the
planner on and with every chunk sampled.  Every launch is a dense one of at most 1 024 edges with PPGPU_PREPASS_MIN_EDGES=0, without
which a launch this small would skip the planner."""
import numpy as np
import pytest

import sweep_worlds as sw
import sweep_worlds_spans as sp
from test_gpu_sweep_inputs import ROUTES, _dense, _against_oracle, _same_answers

pytestmark = pytest.mark.gpu

BOTH = sw.BINARY + ["done_inside", "long16377"] + ["gaussian_" + g for g in sw.GAUSSIAN] + sp.NAMES + sp.OFFPOWER


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _run(torch, monkeypatch, w, route, spans=None):
    """(records, child ribbons) of world w; the handle reads the switches when it is created."""
    monkeypatch.setenv("PPGPU_PREPASS_MIN_EDGES", route)
    if spans is None:
        monkeypatch.delenv("PPGPU_PLAN_SPANS", raising=False)
    else:
        monkeypatch.setenv("PPGPU_PLAN_SPANS", spans)
    return _dense(torch, w.context(), w)


@pytest.mark.parametrize("name", BOTH)
def test_span_planner_leaves_the_chunkwise_planners_bytes(torch_cuda, monkeypatch, name):
    w = sp.WORLDS[name]() if name in sp.WORLDS else sw.WORLDS[name]()
    new, newchild = _run(torch_cuda, monkeypatch, w, "0")
    old, oldchild = _run(torch_cuda, monkeypatch, w, "0", spans="0")
    for f in new.dtype.names:
        a, b = (np.ascontiguousarray(r[f]).view(np.uint8).reshape(len(r), -1) for r in (new, old))
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (name, f, "edges", np.unique(bad)[:8].tolist())
    assert np.array_equal(new.view(np.uint8), old.view(np.uint8)), name
    assert np.array_equal(newchild.view(np.uint8), oldchild.view(np.uint8)), (name, "child ribbons")


@pytest.mark.parametrize("name", sp.NAMES)
def test_span_worlds_against_oracle(torch_cuda, monkeypatch, name):
    w, cpu, cchild = sp.oracle_records(name)
    outs = []
    for route in ROUTES:
        gpu, gchild = _run(torch_cuda, monkeypatch, w, route)
        _against_oracle("%s route %s" % (name, route), gpu, gchild, cpu, cchild, exact=True)
        outs.append(gpu)
    _same_answers(outs[0], outs[1], name + ": skip planner on / off")


@pytest.mark.parametrize("name", ["count64", "count65"])
def test_switch_to_the_many_kernels_still_gives_the_oracles_answers(torch_cuda, monkeypatch, name):
    """64 boxes: the span planner with a full table in LDS.  65: pp_k_plan_skips_many, which is the chunkwise body."""
    w, cpu, cchild = sw.oracle_records(name)
    assert len(w.obst) == int(name[5:])
    gpu, gchild = _run(torch_cuda, monkeypatch, w, "0")
    _against_oracle(name + " span build", gpu, gchild, cpu, cchild, exact=True)
