"""-m gpu: pp_k_solve_edges solves the curve of a (vertex, sample, radius) once for both speeds in dense launches.  The records of
such a launch must be, byte for byte, those of launches that take the one-lane-per-edge path (a single configuration per launch,
an explicit edge list), whatever the mask, the vertex and sample ranges and the slicing; and the pose sweep, which takes "can any
obstacle come near this edge" from the setup record, must agree with the oracle with no, few and more than 64 obstacles."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


# (Launches of different sizes are compared byte for byte here: conftest.py runs the prepasses on every launch, whatever its size;
# without them the float fields carry other rounding noise, see test_small_launches_without_prepasses.)
STRIDE = 8


def _dense(torch, ctx, v0, nv, s0, ns, mask):
    from path_planner_amd import api
    from path_planner_amd.types import RESULT_DTYPE
    ne = api.Context.dense_edge_count(nv, ns, mask)
    d_res = torch.zeros(ne * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    d_child = torch.zeros(ne * STRIDE * 4, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()      # the fill ran on torch's stream, the library works on its own
    ctx.cost_edges_dense(v0, nv, s0, ns, mask, d_res.data_ptr(), d_child.data_ptr(), STRIDE)
    ctx.synchronize()
    return d_res.cpu().numpy().view(RESULT_DTYPE), d_child.cpu().numpy().reshape(ne, STRIDE, 4)


def _listed(torch, ctx, edges):
    from path_planner_amd.types import RESULT_DTYPE
    ne = len(edges)
    d_e = torch.from_numpy(edges.view(np.int64)).to("cuda:0")
    d_res = torch.zeros(ne * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    d_child = torch.zeros(ne * STRIDE * 4, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.cost_edges_list(ne, d_e.data_ptr(), d_res.data_ptr(), d_child.data_ptr(), STRIDE)
    ctx.synchronize()
    return d_res.cpu().numpy().view(RESULT_DTYPE), d_child.cpu().numpy().reshape(ne, STRIDE, 4)


def _context(w, n_samples, verts=None, pool=None):
    from path_planner_amd import api
    ctx = api.Context(0)
    ctx.set_config(w.cfg)
    ctx.set_grid(w.grid, w.res)
    ctx.set_obstacles(w.obst)
    ctx.set_vertices(w.root() if verts is None else verts, w.ribbons4 if pool is None else pool)
    ctx.sampler_init(w.bounds6, w.seed, w.ribbons4)
    n = ctx.sampler_add(n_samples)
    return ctx, n


def _children_as_vertices(w, res, child, pick):
    """Open vertices made from costed edges: each with its own time (hence time grid), ribbon list and coverage time."""
    from path_planner_amd.types import VERTEX_DTYPE
    v = np.zeros(len(pick) + 1, dtype=VERTEX_DTYPE)
    pool = [np.asarray(w.ribbons4, dtype=np.float64).reshape(-1, 4)]
    v[0] = w.root()[0]
    off = len(pool[0])
    for k, e in enumerate(pick):
        r = res[e]
        nr = int((r["info"] >> 8) & 0xFF)
        v[k + 1] = (r["end_x"], r["end_y"], r["end_heading"], r["end_speed"], r["end_time"], r["g"],
                    r["coverage_completed_time"], off, nr)
        pool.append(child[e, :nr])
        off += nr
    return v, np.concatenate(pool)


def _pick_children(res, count):
    """`count` feasible non-goal edges that end at different times, alternating fast and slow ones."""
    from path_planner_amd.types import F_INFEASIBLE, F_GOAL
    feas = np.nonzero(((res["flags"] & F_INFEASIBLE) == 0) & ((res["flags"] & F_GOAL) == 0))[0]
    pick, times = [], set()
    for want_slow in [i % 2 for i in range(count)]:
        for e in feas:
            t = float(res["end_time"][e])
            if ((e % 4) >> 1) == want_slow and t not in times:
                pick.append(int(e))
                times.add(t)
                break
    assert len(pick) == count, "the workload did not give enough distinct children"
    return np.asarray(pick)


def _configs(mask):
    return [c for c in range(4) if (mask >> c) & 1]


def _assert_dense_is_single_configurations(torch, ctx, v0, nv, s0, ns, mask, singles):
    """records of the `mask` launch == the records of the one-configuration launches, position for position"""
    res, child = _dense(torch, ctx, v0, nv, s0, ns, mask)
    cfgs = _configs(mask)
    assert len(res) == nv * ns * len(cfgs)
    for rank, c in enumerate(cfgs):
        if c not in singles:
            singles[c] = _dense(torch, ctx, v0, nv, s0, ns, 1 << c)
        sres, schild = singles[c]
        assert res[rank::len(cfgs)].tobytes() == sres.tobytes(), "mask %#x, configuration %d: records differ" % (mask, c)
        assert child[rank::len(cfgs)].tobytes() == schild.tobytes(), "mask %#x, configuration %d: child ribbons differ" % (mask, c)
    return res, child


def test_every_mask_equals_the_single_configuration_launches(torch_cuda):
    """0xF (two pairs), 0x5 and 0xA (one pair), 0x3 and 0xC (two edges, no pair), 0x7, 0xB, 0xD, 0xE (a pair and a single) against
    0x1, 0x2, 0x4, 0x8, which have no partner and run one lane per edge."""
    from path_planner_amd import workloads
    from path_planner_amd.types import F_INFEASIBLE
    w = workloads.config3(n_samples=600)
    ctx, n = _context(w, 600)
    singles = {}
    for mask in (0xF, 0x5, 0xA, 0x3, 0x7, 0xC, 0xB, 0xD, 0xE):
        res, _ = _assert_dense_is_single_configurations(torch_cuda, ctx, 0, 1, 0, n, mask, singles)
    assert np.count_nonzero((singles[0][0]["flags"] & F_INFEASIBLE) == 0) > 50      # real edges, not a world of refusals
    # the two speeds of a radius do differ (so a record written with its partner's speed would show)
    assert singles[0][0].tobytes() != singles[2][0].tobytes() and singles[1][0].tobytes() != singles[3][0].tobytes()


def test_several_vertices_and_a_sample_range(torch_cuda):
    """nv > 1 with a time grid per vertex, v0 > 0 and s0 > 0: the partner of a work item is found from the launch's own (vertex,
    sample) count, not from the context's."""
    from path_planner_amd import workloads
    w = workloads.config3(n_samples=400)
    ctx, n = _context(w, 400)
    res, child = _dense(torch_cuda, ctx, 0, 1, 0, n, 0xF)
    verts, pool = _children_as_vertices(w, res, child, _pick_children(res, 4))
    assert len(set(verts["time"].tolist())) == len(verts)
    ctx.set_vertices(verts, pool)
    for v0, nv, s0, ns in ((0, 5, 0, n), (1, 3, 37, 201), (2, 2, n - 65, 65), (4, 1, 1, 1)):
        singles = {}
        for mask in (0xF, 0xA, 0x7):
            _assert_dense_is_single_configurations(torch_cuda, ctx, v0, nv, s0, ns, mask, singles)


def test_partners_in_different_slices(torch_cuda, monkeypatch):
    """PPGPU_SLICE_BYTES cuts the launch into slices of consecutive work items; the partner of an edge lies half the launch (0xF) or
    a third of it (0x7) further on.  Budgets from "every partner in another slice" to "the cut goes through the pairs": a slow
    edge whose partner is in its slice writes both records, any other edge its own."""
    from path_planner_amd import workloads
    w = workloads.config2()
    ctx, n = _context(w, 700)
    whole = {mask: _dense(torch_cuda, ctx, 0, 1, 0, n, mask) for mask in (0xF, 0x7, 0x5)}
    singles = {}
    _assert_dense_is_single_configurations(torch_cuda, ctx, 0, 1, 0, n, 0xF, singles)
    # a 0xF launch of 2 800 edges takes about 28 MiB of workspace
    for mib in (1, 3, 7, 11, 16, 20, 24):
        monkeypatch.setenv("PPGPU_SLICE_BYTES", str(mib << 20))
        ctx2, n2 = _context(w, 700)
        assert n2 == n
        for mask, (wres, wchild) in whole.items():
            cres, cchild = _dense(torch_cuda, ctx2, 0, 1, 0, n, mask)
            assert wres.tobytes() == cres.tobytes() and wchild.tobytes() == cchild.tobytes(), "mask %#x in slices of %d MiB" % (mask, mib)


@pytest.mark.parametrize("n_obst,near", [(0, False), (16, False), (16, True), (100, False)])
def test_pose_sweep_takes_the_obstacle_answer_from_the_record(torch_cuda, n_obst, near):
    """Dense from two vertices with different start times (consecutive edges of the launch change vertex and speed), with no
    obstacle, 16 (one per lane, the record's mask decides whether any can come near: once spread over the map, where they stay
    clear of every edge, once crowded around the start, where the edges run into them) and 100 (more than 64: always "some can", the
    per-chunk culling decides): as the oracle computes them, and the same bytes as the same edges given as an explicit list."""
    from path_planner_amd import workloads
    from path_planner_amd.types import edge_pack
    from parity import compare_results
    import oracle as orc
    w = workloads.config3(n_samples=384, n_obst=n_obst)
    if near:
        x0, y0 = float(w.root()["x"][0]), float(w.root()["y"][0])
        w.obst = workloads.obstacles(n_obst, 5, 60.0, time=float(w.root()["time"][0]), keep_free=(30.0, 30.0, 12.0))
        w.obst[:, 0] += x0 - 30.0
        w.obst[:, 1] += y0 - 30.0
    ctx, n = _context(w, 384)
    world = orc.World(w.cfg, w.grid, w.res, w.obst)
    cs = world.add_samples(w.bounds6, w.seed, w.ribbons4, 0, 384)
    assert n == cs.shape[0]
    res, child = _dense(torch_cuda, ctx, 0, 1, 0, n, 0xF)
    verts, pool = _children_as_vertices(w, res, child, _pick_children(res, 2))
    assert verts["time"][1] != verts["time"][2]
    ctx.set_vertices(verts, pool)
    gpu, gchild = _dense(torch_cuda, ctx, 1, 2, 0, n, 0xF)
    ne = len(gpu)
    assert ne == 2 * n * 4
    pos = np.arange(ne)
    vi, ti, cb = 1 + pos // (4 * n), (pos // 4) % n, pos % 4
    # the reference never builds an edge shorter than the collision-check increment: a child and the sample it was built from
    far = np.hypot(verts["x"][vi] - cs[ti, 0], verts["y"][vi] - cs[ti, 1]) > w.cfg.collision_checking_increment
    assert far.sum() > ne - 16
    edges = edge_pack(vi, ti, cb)
    lres, lchild = _listed(torch_cuda, ctx, edges)
    assert gpu.tobytes() == lres.tobytes() and gchild.tobytes() == lchild.tobytes()
    # ... and in an order in which no two consecutive edges share their vertex and speed
    perm = np.random.default_rng(11).permutation(ne)
    pres, pchild = _listed(torch_cuda, ctx, edges[perm].copy())
    assert gpu[perm].tobytes() == pres.tobytes() and gchild[perm].tobytes() == pchild.tobytes()
    cpu, cchild = world.cost_edges(verts, pool, cs[:, 0], cs[:, 1], cs[:, 2], edges[far].copy(), stride=STRIDE, threads=8)
    rep = compare_results(gpu[far], cpu, gchild[far], cchild)
    print(n_obst, near, rep, "edges with a penalty:", int(np.count_nonzero(cpu["collision_penalty"] > 0)))
    assert rep["ok"], rep
    assert rep["n_feasible"] > 100
    if near or n_obst > 64:
        assert np.count_nonzero(cpu["collision_penalty"] > 0) > 50         # the obstacles are met
