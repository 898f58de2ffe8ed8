"""-m gpu: the worlds of tests/grid_worlds.py on the device against the oracle: the static map's packing, lookup and clearance map
on grids that are not square, whose width is no multiple of 32 and whose resolution has no exact reciprocal.  The clearance map is
read back (ppgpu_get_grid_clearance) and must be clearance_numpy's byte for byte: one that is too generous loses a blocked step
next to a single cell, one that is too small only costs the skipped chunks and no parity test would notice.  Costing on both routes
(PPGPU_PREPASS_MIN_EDGES=0: the skip planner runs; huge: every chunk is sampled) must give the oracle's flags and info on every
edge.  The step trace pins the lookup apart from the pose arithmetic: S_BLOCKED of every record against the oracle's isBlocked
applied to the device's own pose.  tests/test_grid_worlds.py shows on the oracle alone that the worlds hold the cases."""
import numpy as np
import pytest

import grid_worlds as gw

pytestmark = pytest.mark.gpu

ROUTES = ("0", "1000000000")         # PPGPU_PREPASS_MIN_EDGES: the skip planner runs / every chunk is sampled
EINVAL = -1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _cfg2():
    from path_planner_amd import workloads
    return workloads.config2(n_samples=256)


def _grid(name):
    if name == "cfg2":
        w = _cfg2()
        return w.grid, w.res
    if name == "dense30":
        w = gw.dense30()
        return w.grid, w.res
    w = gw.WORLDS[name]()
    return w.grid, w.res


# ---------------------------------------------------------------------------------------------- the clearance map
@pytest.mark.parametrize("name", list(gw.WORLDS) + ["dense30", "cfg2"])
def test_clearance_map_is_the_definition(torch_cuda, name):
    from path_planner_amd import api
    grid, res = _grid(name)
    ctx = api.Context(0)
    ctx.set_grid(grid, res)
    dev = ctx.get_grid_clearance(*grid.shape)
    want = gw.clearance_numpy(grid)
    bad = np.argwhere(dev != want)
    print(name, grid.shape, "cells", grid.size, "blocked", int(grid.sum()), "largest clearance", int(want.max()), "cells that differ", len(bad))
    assert len(bad) == 0, (name, bad[:8].tolist(), dev[tuple(bad[:8].T)].tolist(), want[tuple(bad[:8].T)].tolist())


def test_clearance_read_back_refusals(torch_cuda):
    from path_planner_amd import api
    ctx = api.Context(0)
    out = np.full(64, 0xA5, dtype=np.uint8)
    rc = api.LIB.ppgpu_get_grid_clearance(ctx._h, out.ctypes.data, out.size)
    assert rc == EINVAL and api.LIB.ppgpu_last_error().decode() == "grid clearance: no grid is set"
    ctx.set_grid(np.zeros((5, 7), dtype=np.uint8), 4.0)
    rc = api.LIB.ppgpu_get_grid_clearance(ctx._h, out.ctypes.data, 34)
    assert rc == EINVAL and api.LIB.ppgpu_last_error().decode() == "grid clearance: capacity below rows * cols"
    assert api.LIB.ppgpu_get_grid_clearance(ctx._h, None, 64) == EINVAL
    assert np.all(out == 0xA5)
    assert api.LIB.ppgpu_get_grid_clearance(ctx._h, out.ctypes.data, 35) == 0
    assert np.array_equal(out[:35].reshape(5, 7), gw.clearance_numpy(np.zeros((5, 7), dtype=np.uint8))) and np.all(out[35:] == 0xA5)
    ctx.set_grid(None, 0.0)
    assert api.LIB.ppgpu_get_grid_clearance(ctx._h, out.ctypes.data, out.size) == EINVAL


# ---------------------------------------------------------------------------------------------- costing
def _run(monkeypatch, w, route):
    """(handle, records, child ribbons) of world w through one route; the handle reads the switch when it is created."""
    monkeypatch.setenv("PPGPU_PREPASS_MIN_EDGES", route)
    ctx = w.context()
    gpu, gchild = ctx.cost_edges_host(w.edges, stride=gw.RIBBON_STRIDE)
    return ctx, gpu, gchild


def _against_oracle(what, gpu, gchild, cpu, cchild):
    from parity import compare_results
    rep = compare_results(gpu, cpu, gchild, cchild)
    print(what, {k: rep[k] for k in ("n", "n_feasible", "worst_rel", "n_flag_mismatch", "n_info_mismatch")})
    assert rep["ok"], (what, rep)
    for f in ("flags", "info"):
        bad = np.nonzero(gpu[f] != cpu[f])[0]
        assert bad.size == 0, (what, f, bad[:8].tolist(), gpu[f][bad[:8]].tolist(), cpu[f][bad[:8]].tolist())


@pytest.mark.parametrize("name", list(gw.WORLDS))
def test_world_against_oracle_on_both_routes(torch_cuda, monkeypatch, name):
    w, cpu, cchild = gw.oracle_records(name)
    outs = []
    for route in ROUTES:
        _, gpu, gchild = _run(monkeypatch, w, route)
        _against_oracle("%s route %s" % (name, route), gpu, gchild, cpu, cchild)
        outs.append(gpu)
    for f in ("flags", "info"):
        assert np.array_equal(outs[0][f], outs[1][f]), (name, f, "skip planner on / off")


# ---------------------------------------------------------------------------------------------- the lookup, apart from the pose
def _picked(name, w, cpu):
    """At most 128 edges: the straight ones of a boundary world, then all that a cell blocks, then those that leave the map (side by
    side in turn), then the rest."""
    from path_planner_amd.types import F_INFEASIBLE
    cell, sides = gw.edge_classes(name)
    order = list(range(getattr(w, "n_straight", 0))) + cell.tolist()
    by_side = [sides[s].tolist() for s in "WESN"]
    for i in range(max(len(v) for v in by_side)):
        order += [v[i] for v in by_side if i < len(v)]
    order += np.nonzero((cpu["flags"] & F_INFEASIBLE) == 0)[0].tolist()
    seen, pick = set(), []
    for e in order:
        if e not in seen:
            seen.add(e); pick.append(e)
    return np.asarray(pick[:128], dtype=np.int64), len(cell)


@pytest.mark.parametrize("name", list(gw.WORLDS))
def test_trace_blocked_flag_is_the_oracles_lookup_of_the_devices_pose(torch_cuda, name):
    from path_planner_amd.types import S_BLOCKED, F_INFEASIBLE
    w, cpu, _ = gw.oracle_records(name)
    pick, n_cell = _picked(name, w, cpu)
    ctx = w.context()
    rec, counts, st = ctx.trace_edges(w.edges[pick], w.ng)
    assert np.array_equal(counts, (rec["info"] >> 16).astype(counts.dtype)), "trace records per edge != info >> 16"
    assert np.array_equal(rec["info"], cpu["info"][pick]) and np.array_equal(rec["flags"], cpu["flags"][pick])
    valid = np.arange(w.ng)[None, :] < counts[:, None]
    blk = (st["flags"] & S_BLOCKED) != 0
    last = np.arange(w.ng)[None, :] == (counts[:, None] - 1)
    assert not np.any(blk & valid & ~last), "S_BLOCKED before an edge's last record"
    x, y = np.ascontiguousarray(st["x"][valid]), np.ascontiguousarray(st["y"][valid])
    want = w.oracle_world().is_blocked(x, y) != 0
    got = blk[valid]
    bad = np.nonzero(want != got)[0]
    on_line = int((np.abs(x / w.res - np.round(x / w.res)) <= 1e-9 * np.abs(x / w.res)).sum() + (np.abs(y / w.res - np.round(y / w.res)) <= 1e-9 * np.abs(y / w.res)).sum())
    print(name, "traced", len(pick), "cell-blocked among them", min(n_cell, len(pick)), "records", int(valid.sum()), "blocked", int(got.sum()),
          "coordinates on a cell boundary", on_line, "lookups that differ", len(bad))
    assert bad.size == 0, (name, x[bad[:8]].tolist(), y[bad[:8]].tolist(), got[bad[:8]].tolist())
    # every blocked last record belongs to an infeasible edge, and every edge the map stopped has one
    stopped = blk[np.arange(len(pick)), np.maximum(counts - 1, 0)] & (counts > 0)
    assert np.all((rec["flags"][stopped] & F_INFEASIBLE) != 0)
    if name in gw.PILLARS:
        assert int(stopped.sum()) >= 30


# ---------------------------------------------------------------------------------------------- the sampler's map filter
def test_sampler_on_a_dense_non_square_map(torch_cuda):
    import oracle as orc
    from path_planner_amd import api
    w = gw.dense30()
    ctx = api.Context(0)
    ctx.set_config(w.cfg); ctx.set_grid(w.grid, w.res); ctx.set_obstacles(None)
    ctx.set_vertices(w.root(), w.ribbons4)
    ctx.sampler_init(w.bounds6, w.seed, w.ribbons4)
    n = ctx.sampler_add(w.n_samples)
    gs = ctx.get_samples()
    cs = orc.World(w.cfg, w.grid, w.res).add_samples(w.bounds6, w.seed, w.ribbons4, 0, w.n_samples)
    print("dense30: the device kept", n, "the oracle", len(cs), "of", w.n_samples)
    assert n == len(cs) and 0.6 * w.n_samples <= n <= 0.8 * w.n_samples
    assert np.array_equal(gs[:, :3].view(np.uint64), cs[:, :3].view(np.uint64)), "sampler stream must be bit-identical"


# ---------------------------------------------------------------------------------------------- a second grid on the same handle
def test_regrid_on_one_handle(torch_cuda):
    """cfg2's grid (1024 x 1024), then `wide` (37 x 83: every buffer is reused, far larger than needed), then no grid, then `tall`
    (201 x 45): after each step the records and the clearance map are those of a fresh handle, byte for byte.  `wide` and `tall`
    cost their own edges (and give the oracle's flags); cfg2's grid and the base map cost wide's."""
    from path_planner_amd import api
    c2 = _cfg2()
    wide, cpu_wide, _ = gw.oracle_records("wide")
    tall, cpu_tall, _ = gw.oracle_records("tall")

    def load(ctx, grid, res, probe):
        ctx.set_grid(grid, res)
        ctx.set_vertices(probe.verts, probe.rib)
        ctx.set_samples(probe.sx, probe.sy, probe.sh)
        rec, child = ctx.cost_edges_host(probe.edges, stride=gw.RIBBON_STRIDE)
        clear = ctx.get_grid_clearance(*grid.shape) if grid is not None else None
        return rec, child, clear

    def handle():
        ctx = api.Context(0)
        ctx.set_config(wide.cfg); ctx.set_obstacles(None)
        return ctx

    assert bytes(wide.cfg) == bytes(tall.cfg)
    ctx = handle()
    n_inf = {}
    for what, grid, res, probe in (("cfg2", c2.grid, c2.res, wide), ("wide", wide.grid, wide.res, wide), ("none", None, 0.0, wide),
                                   ("tall", tall.grid, tall.res, tall)):
        rec, child, clear = load(ctx, grid, res, probe)
        frec, fchild, fclear = load(handle(), grid, res, probe)
        assert np.array_equal(rec.view(np.uint8), frec.view(np.uint8)), what
        assert np.array_equal(child.view(np.uint64), fchild.view(np.uint64)), what
        if grid is not None:
            assert np.array_equal(clear, fclear) and np.array_equal(clear, gw.clearance_numpy(grid)), what
        n_inf[what] = int((rec["flags"] & 1).sum())
        if what in ("wide", "tall"):
            cpu = cpu_wide if what == "wide" else cpu_tall
            assert np.array_equal(rec["flags"], cpu["flags"]) and np.array_equal(rec["info"], cpu["info"]), what
    print("regrid: infeasible edges on cfg2 / wide / no grid / tall:", n_inf)
    assert n_inf["none"] < n_inf["wide"] and n_inf["cfg2"] != n_inf["wide"]      # the map on the handle is the one set last
