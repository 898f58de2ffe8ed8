"""-m gpu: the pose sweep's walk over the chunks the skip planner left to sample, one sampled chunk per trip.  The oracle's records
and the step trace's running penalty (pp_k_trace_steps does not skip) wherever the walk could go wrong: chunks that are not
adjacent, the heading carried from lane 63 to lane 0 or taken from the planner's word, an edge that ends or is blocked on the last
lane of a chunk, on lane 0 of the next, in a chunk of one step, and an edge whose skip bytes come in two groups of 64."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _dense(torch, ctx, nv, n, mask, stride=8):
    from path_planner_amd import api
    from path_planner_amd.types import RESULT_DTYPE
    ne = api.Context.dense_edge_count(nv, n, mask)
    d_res = torch.zeros(ne * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    d_child = torch.zeros(ne * stride * 4, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()      # the fill ran on torch's stream, the library works on its own
    ctx.cost_edges_dense(0, nv, 0, n, mask, d_res.data_ptr(), d_child.data_ptr(), stride)
    ctx.synchronize()
    return d_res.cpu().numpy().view(RESULT_DTYPE), d_child.cpu().numpy().reshape(ne, stride, 4)


# ---------------------------------------------------------------------------------------------- both routes, config 3
_CFG3 = {}


def _cfg3_oracle(w, samples):
    """The oracle's records of config 3's first 2 048 kept samples, computed once and shared by the two routes."""
    if not _CFG3:
        import oracle as orc
        from path_planner_amd.types import edge_pack
        n = len(samples)
        world = orc.World(w.cfg, w.grid, w.res, w.obst)
        e = edge_pack(np.zeros(4 * n, dtype=np.uint64), np.repeat(np.arange(n), 4), np.tile(np.arange(4), n))
        cpu, cchild = world.cost_edges(w.root(), w.ribbons4, samples[:, 0], samples[:, 1], samples[:, 2], e, stride=8, threads=8)
        cpu.setflags(write=False); cchild.setflags(write=False)
        _CFG3["samples"], _CFG3["cpu"], _CFG3["cchild"] = samples.copy(), cpu, cchild
    assert np.array_equal(samples, _CFG3["samples"]), "the sampler drew other samples than on the first route"
    return _CFG3["cpu"], _CFG3["cchild"]


@pytest.mark.parametrize("threshold", ["0", "1000000000"])
def test_both_routes_match_oracle_at_2048_samples(torch_cuda, monkeypatch, threshold):
    """Config 3, 2 048 samples (8 192 edges), mask 0xF, against the oracle.  Threshold 0: the skip planner runs, the walk goes
    through chunks that are not adjacent and the heading before a chunk comes from the planner's word.  Threshold huge: no chunk is
    skipped, the walk goes through adjacent chunks and the heading is carried from lane 63 to lane 0 (the radius-8 edges may not
    cover while turning)."""
    from path_planner_amd import api, workloads
    from parity import compare_results
    w = workloads.config3(n_samples=2048)
    monkeypatch.setenv("PPGPU_PREPASS_MIN_EDGES", threshold)
    ctx = api.Context(0)       # (the handle reads the switches when it is created)
    ctx.set_config(w.cfg); ctx.set_grid(w.grid, w.res); ctx.set_obstacles(w.obst); ctx.set_vertices(w.root(), w.ribbons4)
    ctx.sampler_init(w.bounds6, w.seed, w.ribbons4)
    ctx.sampler_add(2048)
    n = ctx.sampler_add(512)       # (the sampler keeps some nine draws in ten: the first 2 048 it kept are costed)
    assert n >= 2048
    gpu, gchild = _dense(torch_cuda, ctx, 1, 2048, 0xF)
    assert len(gpu) == 8192
    cpu, cchild = _cfg3_oracle(w, ctx.get_samples()[:2048, :3])
    rep = compare_results(gpu, cpu, gchild, cchild)
    nonturn = gpu["info"][(np.arange(8192) % 2) == 0] >> 16
    print("threshold", threshold, {k: rep[k] for k in ("n_feasible", "worst_rel", "n_flag_mismatch", "n_info_mismatch")},
          "steps per edge: max", int((gpu["info"] >> 16).max()), "radius-8 edges beyond one chunk", int((nonturn > 64).sum()))
    assert rep["ok"], rep


# ---------------------------------------------------------------------------------------------- where the walk can go wrong
STOPS = (1, 63, 64, 65, 127, 128)       # the first blocked step of the straight fast edge of vertex i
INC, VMAX = 0.05, 2.5                   # a fast edge advances 0.05 m per step of 0.02 s
Y0, DY = 3.05, 3.2                      # the vertices' rows


class _Lanes:
    """A 256 x 256 grid at 0.1 m.  Seven vertices heading east on rows of their own, at the start time: vertex i < 6 meets a blocked
    column whose first cell holds step STOPS[i] of its straight fast edge and no step before it (0.05 m per step, two steps per
    cell: the vertex starts a quarter or three quarters of a cell into its own, so that the wanted step is the first in the column's
    cell); vertex 6 meets none.  Sample i is straight ahead of vertex i, the other samples are drawn over the map; every vertex
    is costed against every sample (1 792 (vertex, sample) pairs of 4 edges).  One standing box across all rows, whose west face the
    straight edges cross at step 90: inside the second chunk.  `steps`: how many steps an edge that nothing stops executes — the
    horizon ends the sweep there (64: one chunk; 65: a second chunk of one step; 128: an exact pair; 129, 130: a third chunk of one
    or two steps), the time grid itself being 7 entries longer."""

    def __init__(self, steps):
        from path_planner_amd.types import make_config, VERTEX_DTYPE, H_MAX_DISTANCE, edge_pack
        dt = INC / VMAX
        self.cfg = make_config(start_state_time=1.0, time_horizon=(steps - 0.5) * dt, heuristic=H_MAX_DISTANCE)
        self.res = 0.1
        self.grid = np.zeros((256, 256), dtype=np.uint8)
        self.rib = np.asarray([[4.0, 24.0, 22.0, 24.0], [3.0, Y0 + 2 * DY + 0.2, 20.0, Y0 + 2 * DY + 0.2]], dtype=np.float64)
        nv = len(STOPS) + 1
        self.verts = np.zeros(nv, dtype=VERTEX_DTYPE)
        rng = np.random.default_rng(11)
        ns = 256
        self.sx, self.sy, self.sh = rng.uniform(1.0, 24.6, ns), rng.uniform(1.0, 24.6, ns), rng.uniform(0, 2 * np.pi, ns)
        for i in range(nv):
            y = Y0 + DY * i
            odd = i < len(STOPS) and STOPS[i] % 2 == 1
            x0 = 3.0 + (0.075 if odd else 0.025)
            self.verts[i] = (x0, y, np.pi / 2, VMAX, 1.0, 0.0, -1.0, 0, len(self.rib))
            if i < len(STOPS):
                col = int((x0 + INC * STOPS[i] + 1e-9) / self.res)
                assert int((x0 + INC * (STOPS[i] - 1) + 1e-9) / self.res) == col - 1
                row = int(y / self.res)
                self.grid[row - 4:row + 5, col:col + 3] = 1
            self.sx[i], self.sy[i], self.sh[i] = x0 + 16.0, y, np.pi / 2
        # x, y, heading, speed, time, width, length: a standing box 2 m x 40 m (grown by 1 m on every side by the strict test),
        # west face at x = 3.025 + 90 * 0.05 + 0.02
        self.obst = np.asarray([[3.025 + 90 * INC + 0.02 + 2.0, 12.8, 0.0, 0.0, 1.0, 2.0, 40.0]], dtype=np.float64)
        self.nv, self.ns = nv, ns
        v = np.repeat(np.arange(nv), ns * 4)
        s = np.tile(np.repeat(np.arange(ns), 4), nv)
        c = np.tile(np.arange(4), nv * ns)
        self.edges = edge_pack(v, s, c)
        # vertex i towards sample i at full speed: configuration 0 (radius 8: may not cover while turning, its heading bits matter)
        # and configuration 1 (coverage radius)
        self.straight = np.array([[(i * ns + i) * 4 + c for c in (0, 1)] for i in range(nv)])

    def context(self):
        from path_planner_amd import api
        ctx = api.Context(0)
        ctx.set_config(self.cfg); ctx.set_grid(self.grid, self.res); ctx.set_obstacles(self.obst)
        ctx.set_vertices(self.verts, self.rib)
        ctx.set_samples(self.sx, self.sy, self.sh)
        return ctx


_ORACLE = {}


def _oracle(steps):
    """The oracle's records of one shape, computed once."""
    if steps not in _ORACLE:
        import oracle as orc
        L = _Lanes(steps)
        world = orc.World(L.cfg, L.grid, L.res, L.obst)
        cpu, cchild = world.cost_edges(L.verts, L.rib, L.sx, L.sy, L.sh, L.edges, stride=8, threads=8)
        cpu.setflags(write=False); cchild.setflags(write=False)
        _ORACLE[steps] = (L, cpu, cchild)
    return _ORACLE[steps]


@pytest.mark.parametrize("steps", [64, 65, 128, 129, 130])
def test_chunk_ends_against_oracle_and_trace(torch_cuda, steps):
    from path_planner_amd.types import F_INFEASIBLE
    from parity import compare_results
    L, cpu, cchild = _oracle(steps)
    # the shape is what the docstring says it is (the oracle's own step counts)
    ref_steps = cpu["info"] >> 16
    assert int(ref_steps.max()) == steps, (int(ref_steps.max()), steps)
    for i, st in enumerate(STOPS):
        for e in L.straight[i]:
            if st < steps:        # (the blocked step is counted: Edge.cpp:144-147)
                assert ref_steps[e] == st + 1 and (cpu["flags"][e] & F_INFEASIBLE), (i, st, int(ref_steps[e]), int(cpu["flags"][e]))
            else:
                assert ref_steps[e] == steps and not (cpu["flags"][e] & F_INFEASIBLE), (i, st, int(ref_steps[e]))
    assert np.all(ref_steps[L.straight[-1]] == steps)
    if steps > 91:
        through = np.concatenate([L.straight[i] for i in range(L.nv) if i >= len(STOPS) or STOPS[i] > 91])
        assert np.all(cpu["collision_penalty"][through] > 0), "the straight edges cross the box's face in the second chunk"
    cpf = L.cfg.collision_penalty_factor
    stride = steps + 8
    ctx = L.context()
    gpu, gchild = _dense(torch_cuda, ctx, L.nv, L.ns, 0xF)
    rep = compare_results(gpu, cpu, gchild, cchild)
    print("steps", steps, {k: rep[k] for k in ("n_feasible", "worst_rel", "n_flag_mismatch", "n_info_mismatch")})
    assert rep["ok"], rep
    assert np.array_equal(gpu["flags"], cpu["flags"]) and np.array_equal(gpu["info"], cpu["info"])
    rec, counts, st = ctx.trace_edges(L.edges, stride)
    assert np.array_equal(counts, (gpu["info"] >> 16).astype(counts.dtype)), "trace records per edge != info >> 16"
    has = np.nonzero(counts > 0)[0]
    last = st[has, counts[has] - 1]
    assert np.array_equal(last["penalty_before"] + last["collision"] * cpf, gpu["collision_penalty"][has]), "running penalty != the record's"
    assert np.all(gpu["collision_penalty"][counts == 0] == 0.0)


# ---------------------------------------------------------------------------------------------- more than 64 chunks per edge
def test_more_than_64_chunks_per_edge(torch_cuda):
    """Config 3's world with a horizon of 4 200 steps (66 chunks: the skip bytes of an edge come in two groups of 64) and 128
    samples, against the oracle's records."""
    from path_planner_amd import api, workloads
    from path_planner_amd.types import edge_pack
    from parity import compare_results
    import oracle as orc
    w = workloads.config3(n_samples=128)
    w.cfg.time_horizon = 4200.5 * (w.cfg.collision_checking_increment / w.cfg.max_speed)
    ctx = api.Context(0)
    ctx.set_config(w.cfg); ctx.set_grid(w.grid, w.res); ctx.set_obstacles(w.obst); ctx.set_vertices(w.root(), w.ribbons4)
    ctx.sampler_init(w.bounds6, w.seed, w.ribbons4)
    n = ctx.sampler_add(w.n_samples)
    gpu, gchild = _dense(torch_cuda, ctx, 1, n, 0xF)
    world = orc.World(w.cfg, w.grid, w.res, w.obst)
    cs = world.add_samples(w.bounds6, w.seed, w.ribbons4, 0, w.n_samples)
    ne = len(gpu)
    e = edge_pack(np.zeros(ne, dtype=np.uint64), np.repeat(np.arange(n), 4), np.tile(np.arange(4), n))
    cpu, cchild = world.cost_edges(w.root(), w.ribbons4, cs[:, 0], cs[:, 1], cs[:, 2], e, stride=8, threads=8)
    steps = gpu["info"] >> 16
    print("steps per edge: max", int(steps.max()), "edges beyond 4 096 steps", int((steps > 4096).sum()))
    assert int(steps.max()) >= 4160, "no edge reaches the second group of skip bytes"
    rep = compare_results(gpu, cpu, gchild, cchild)
    assert rep["ok"], rep
