"""-m gpu: every launch reads the effective grid of a keep-out limit.  Two handles per world: A holds the grid as set plus
ppgpu_set_keepout_limit2, B was given the inflated array (tests/keepout_worlds.py: effective) through ppgpu_set_grid and no limit.
The same bytes are required from both: edge records and child ribbons with and without the prepasses (pp_k_plan_skips and the
approach lanes), step records, the sampler's kept samples.  One world of A is also compared with the oracle on the inflated grid,
so that A does not lean on B alone.  Then A's clearance records, whose gap2 is still that of the grid as set: planning with limit2
and reporting against the same limit2 certify each other."""
import math

import numpy as np
import pytest

import clearance_replay as clr
import grid_worlds as gw
import keepout_worlds as kw

pytestmark = pytest.mark.gpu
ROUTES = ("1000000000", "0")      # PPGPU_PREPASS_MIN_EDGES: the route without prepasses / the skip planner and the approach lanes run
# world -> limit2.  wide: 37 x 83 @ 1 m; walls: 150 x 210 @ 0.25 m, one-cell walls with gaps the band closes; fine: 300 x 700 @ 0.07 m,
# wider than the threshold kernel's tile of 256 columns
WORLDS = {"wide": 4, "walls": 9, "fine": 5}
TRACED = 128                      # edges of the step and clearance traces
_INPUT = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _input(name):
    """(world, limit2, gap2 of its grid, the inflated grid), computed once per process."""
    if name not in _INPUT:
        w = gw.WORLDS[name]()
        k = WORLDS[name]
        g2 = clr.gap2_numpy(w.grid)
        inflated = kw.effective(w.grid, k, g2)
        r, c = int(w.verts[0]["y"] / w.res), int(w.verts[0]["x"] / w.res)
        assert g2[r, c] >= k and not inflated[r, c], "the root lies outside the band"
        assert inflated.sum() > 4 * (w.grid != 0).sum()
        g2.setflags(write=False); inflated.setflags(write=False)
        _INPUT[name] = (w, k, g2, inflated)
    return _INPUT[name]


def _pair(monkeypatch, name, route):
    """(A, B): the handles read the route when they are created."""
    w, k, g2, inflated = _input(name)
    monkeypatch.setenv("PPGPU_PREPASS_MIN_EDGES", route)
    a = w.context()
    a.set_keepout_limit2(k)
    b = w.with_grid(inflated).context()
    assert a.get_keepout_limit2() == k and b.get_keepout_limit2() == 0
    return a, b


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", sorted(WORLDS))
def test_records_and_steps_equal_those_of_the_inflated_grid(torch_cuda, monkeypatch, name, route):
    from path_planner_amd.types import F_INFEASIBLE
    w, k, g2, inflated = _input(name)
    a, b = _pair(monkeypatch, name, route)
    ra, ca = a.cost_edges_host(w.edges, stride=gw.RIBBON_STRIDE)
    rb, cb = b.cost_edges_host(w.edges, stride=gw.RIBBON_STRIDE)
    assert ra.tobytes() == rb.tobytes() and ca.tobytes() == cb.tobytes(), (name, route, np.nonzero(ra != rb)[0][:8].tolist())
    # the band decides something: edges that the grid as set lets through are infeasible here
    plain = w.context()
    r0 = plain.cost_edges_host(w.edges)
    stopped = np.nonzero(((ra["flags"] & F_INFEASIBLE) != 0) & ((r0["flags"] & F_INFEASIBLE) == 0))[0]
    assert len(stopped) > 0 and np.any((ra["flags"] & F_INFEASIBLE) == 0), (name, len(stopped))
    # step records of the edges the band stopped first, then the others
    rest = np.setdiff1d(np.arange(len(w.edges)), stopped)
    pick = np.concatenate([stopped, rest])[:TRACED]
    ta, na, sa = a.trace_edges(w.edges[pick], w.ng)
    tb, nb, sb = b.trace_edges(w.edges[pick], w.ng)
    assert ta.tobytes() == tb.tobytes() == ra[pick].tobytes() and np.array_equal(na, nb) and sa.tobytes() == sb.tobytes(), (name, route)
    print(name, "route", route, "limit2", k, ":", len(stopped), "of", len(w.edges), "edges stopped by the band alone")
    for ctx in (a, b, plain):
        ctx.close()


def test_against_the_oracle_on_the_inflated_grid(torch_cuda, monkeypatch):
    from parity import compare_results
    w, k, g2, inflated = _input("wide")
    cpu, cchild = w.with_grid(inflated).oracle_cost()
    for route in ROUTES:
        monkeypatch.setenv("PPGPU_PREPASS_MIN_EDGES", route)
        a = w.context()
        a.set_keepout_limit2(k)
        gpu, gchild = a.cost_edges_host(w.edges, stride=gw.RIBBON_STRIDE)
        rep = compare_results(gpu, cpu, gchild, cchild)
        print("wide under limit2", k, "route", route, {f: rep[f] for f in ("n", "n_feasible", "worst_rel", "n_flag_mismatch", "n_info_mismatch")})
        assert rep["ok"], rep
        for f in ("flags", "info"):
            assert np.array_equal(gpu[f], cpu[f]), (route, f, np.nonzero(gpu[f] != cpu[f])[0][:8].tolist())
        a.close()


@pytest.mark.parametrize("world,limit2", [("dense30", 1), ("wide_plan", 9)])
def test_sampler_keeps_the_samples_of_the_inflated_grid(torch_cuda, world, limit2):
    """2 000 attempts from one seed.  dense30: 30 % of 37 x 83 cells blocked at random, so that a band of one cell leaves a few
    dozen free cells and the filter works hard; wide's grid with its few pillars under the planning test's limit."""
    from path_planner_amd import api
    w = gw.dense30() if world == "dense30" else gw.wide_plan()[0]
    w.n_samples = 2000
    inflated = kw.effective(w.grid, limit2)
    assert 0 < (inflated == 0).sum() < (w.grid == 0).sum()
    got = []
    for grid, k in ((w.grid, limit2), (inflated, 0), (w.grid, 0)):
        ctx = api.Context(0)
        ctx.set_config(w.cfg); ctx.set_grid(grid, w.res); ctx.set_obstacles(None)
        ctx.set_keepout_limit2(k)
        ctx.set_vertices(w.root(), w.ribbons4)
        ctx.sampler_init(w.bounds6, w.seed, w.ribbons4)
        n = ctx.sampler_add(w.n_samples)
        s = ctx.get_samples()
        assert len(s) == n
        got.append(s)
        ctx.close()
    a, b, plain = got
    assert a.tobytes() == b.tobytes() and 0 < len(a) < len(plain), (len(a), len(b), len(plain))
    # every kept sample lies in a free cell of the effective grid
    r, c = gw.cell_of(a[:, 1], w.res), gw.cell_of(a[:, 0], w.res)
    assert not inflated[r, c].any()


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_clearance_records_certify_the_plan_limit(torch_cuda, name):
    """trace_clearance on A with margin = res * sqrt(limit2): the walk is that of the effective grid, the gap2 that of the grid as
    set.  An edge that is not blocked never steps below the margin; a blocked one does so exactly once, at its last step; and some
    edge is blocked at a step whose own gap2 is above 0: the band stopped it, not a charted cell."""
    from path_planner_amd.types import CL_BLOCKED, CL_EMPTY
    w, k, g2, inflated = _input(name)
    margin = w.res * math.sqrt(float(k))
    assert clr.limit2(w.res, margin) == k
    a = w.context()
    a.set_keepout_limit2(k)
    res, counts, recs = a.trace_clearance(w.edges, margin=margin)
    ok = (recs["flags"] & CL_EMPTY) == 0
    blocked = ok & ((recs["flags"] & CL_BLOCKED) != 0)
    free = ok & ~blocked
    assert blocked.any() and free.any()
    assert np.all(recs["below_steps"][free] == 0) and np.all(recs["first_below_step"][free] == -1) and np.all(recs["gap2"][free] >= k)
    assert np.all(recs["below_steps"][blocked] == 1) and np.array_equal(recs["first_below_step"][blocked], counts[blocked] - 1)
    assert np.array_equal(recs["step"][blocked], counts[blocked] - 1) and np.all(recs["gap2"][blocked] < k)
    band = blocked & (recs["gap2"] > 0)
    assert band.any()
    print(name, "limit2", k, ":", int(blocked.sum()), "blocked edges,", int(band.sum()), "of them at a step with gap2 > 0,", int(free.sum()), "free")
    # ... and the records are the recipe's on the steps of the same handle (S_BLOCKED of the effective grid, gap2 of the grid as set)
    pick = np.concatenate([np.nonzero(band)[0][:TRACED // 2], np.nonzero(free)[0][:TRACED // 2]])
    _, n, steps = a.trace_edges(w.edges[pick], w.ng)
    assert np.array_equal(n, counts[pick])
    for j, e in enumerate(pick):
        want = clr.replay(w.grid, w.res, steps[j, :n[j]], margin, g2)
        for f in ("time", "x", "y", "step", "gap2", "below_steps", "first_below_step", "first_below_time", "flags"):
            assert recs[e][f] == want[f], (name, int(e), f, recs[e][f], want[f])
    a.close()
