"""-m gpu: who computes h (pp_h_route, path_planner_amd/csrc/pp_device.h).  The smallest child lists on either side of every boundary
of the rule, each costed under the switches that send it down another route — the cover sweep's wave, the finish lane's list, the quiet
lane, pp_k_heuristic_lanes, the 9..12 pass, the overflow flag and the table pass behind it, the unfused kernels — against the oracle's
literal recursion; and the launch counters those routes hand to one another, across a sliced trace."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H_MAX, H_ALL, H_K, H_DUBINS_ALL, H_DUBINS_K = range(5)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def route_world(heur, k, n, ns, near=True, jitter=False):
    """No grid, no obstacles, one root with n ribbons of which at most the first lies within its horizon (near), so that an edge
    crosses one ribbon at most: ns targets, the even ones south of that ribbon (most of their edges leave the list alone), the odd ones
    north of it (their edges cross it: a split, a trimmed end or nothing, by radius and speed).  The others follow the formula of
    test_lane_heuristic_is_the_wave_heuristic, 230 m further east."""
    from path_planner_amd.types import make_config
    from path_planner_amd.workloads import root_vertex
    rng = np.random.default_rng(1000 * heur + 100 * n + k)
    cfg = make_config(start_state_time=2.0, heuristic=heur, tsp_k=k)
    rib = np.asarray([[270 + 9 * i, 50 + 5 * (i % 3), 274 + 9 * i + 3 * (i % 2), 96 - 4 * (i % 4)] for i in range(n)], dtype=np.float64)
    if near:
        rib[0] = [55.0, 45.0, 85.0, 45.0]
    if jitter:           # off the integer lattice, where two ribbons can be exactly equally far from a third's end (the table pass refuses ties)
        rib += rng.uniform(-0.4, 0.4, rib.shape)
    root = root_vertex(70.0, 30.0, 0.3, 2.5, 2.0, rib)
    north = (np.arange(ns) % 2) == 1
    sx = np.where(north, rng.uniform(62, 78, ns), rng.uniform(45, 95, ns))
    sy = np.where(north, rng.uniform(55, 70, ns), rng.uniform(5, 35, ns))
    return cfg, rib, root, sx, sy, rng.uniform(0, 2 * np.pi, ns)


def dense_edges(ns, mask):
    """The edge list a dense launch of one vertex, ns targets and the configurations of mask costs, in its order."""
    from path_planner_amd.types import edge_pack
    cfgs = np.array([c for c in range(4) if (mask >> c) & 1])
    return edge_pack(np.zeros(len(cfgs) * ns, dtype=np.uint64), np.repeat(np.arange(ns), len(cfgs)), np.tile(cfgs, ns))


# A far Gaussian obstacle: the Gaussian model's own kernels run (no lane kernels, the unfused pp_k_heuristic), its penalty is nothing
FAR_GAUSSIAN = np.array([[900.0, 900.0, 0.0, 0.0, 2.0]])

# (heuristic, K, ribbons, targets, configuration mask, child stride or 0 = ribbons + 2, model, near).  Targets and mask size the case by
# the oracle (All: 0.1 s per edge at 7 ribbons, 0.5 s at 8; K = 2: 0.7 s at 12; K = 3: 1 s at 10, 7 s at 11; a flagged list costs nothing).
ROUTE_CASES = [
    (H_ALL, 0, 5, 60, 0xF, 0, "binary", True), (H_ALL, 0, 6, 25, 0xF, 0, "binary", True), (H_ALL, 0, 7, 4, 0xF, 0, "binary", True),
    (H_ALL, 0, 8, 2, 0xF, 0, "binary", True), (H_ALL, 0, 9, 60, 0xF, 0, "binary", True),
    (H_K, 2, 6, 60, 0xF, 0, "binary", True), (H_K, 2, 7, 60, 0xF, 0, "binary", True), (H_K, 2, 8, 60, 0xF, 0, "binary", True),
    (H_K, 2, 9, 30, 0xF, 0, "binary", True), (H_K, 2, 12, 3, 0x3, 0, "binary", True), (H_K, 2, 13, 60, 0xF, 0, "binary", True),
    # K = 3: 6^8 prefixes at 11 ribbons stay below 2^21, 6^9 at 12 do not — the rule's boundary is 11 | 12; one edge at 11 (7 s of oracle)
    (H_K, 3, 6, 60, 0xF, 0, "binary", True), (H_K, 3, 10, 1, 0x3, 0, "binary", True), (H_K, 3, 11, 1, 0x1, 0, "binary", True),
    (H_K, 3, 12, 60, 0xF, 0, "binary", True),
    (H_K, 0, 3, 60, 0xF, 0, "binary", True), (H_K, 0, 9, 60, 0xF, 0, "binary", True),
    (H_MAX, 0, 8, 60, 0xF, 0, "binary", True), (H_MAX, 0, 31, 60, 0xF, 0, "binary", True), (H_MAX, 0, 32, 60, 0xF, 0, "binary", True),
    (H_MAX, 0, 40, 60, 0xF, 0, "binary", True),
    # the Dubins heuristics: out of reach of every ribbon (collinear split pieces sit on the Dubins mod-2pi discontinuity, DESIGN.md
    # Appendix C); 9 ribbons: the oracle mirrors the flag and h = 0
    (H_DUBINS_ALL, 0, 3, 30, 0xF, 0, "binary", False), (H_DUBINS_K, 2, 3, 30, 0xF, 0, "binary", False),
    (H_DUBINS_ALL, 0, 9, 30, 0xF, 0, "binary", False), (H_DUBINS_K, 2, 9, 30, 0xF, 0, "binary", False),
    (H_K, 2, 7, 60, 0xF, 0, "gaussian", True),                                       # the unfused pp_k_heuristic
    (H_K, 2, 7, 60, 0xF, 7, "binary", True), (H_K, 2, 7, 60, 0xF, 6, "binary", True),     # a child slot of n, and of n - 1: the truncated list
]


def _case_id(c):
    heur, k, n, ns, mask, stride, model, near = c
    return "%s%s-n%d%s%s" % (("max", "all", "k", "dubins_all", "dubins_k")[heur], k if heur in (H_K, H_DUBINS_K) else "", n,
                            "-stride%d" % stride if stride else "", "-gaussian" if model == "gaussian" else "")


def _context(cfg, rib, root, sx, sy, sh, model):
    from path_planner_amd import api
    ctx = api.Context(0)         # (the handle reads the switches when it is created)
    ctx.set_config(cfg)
    ctx.set_grid(None, 0.5)
    if model == "gaussian":
        ctx.set_gaussian_obstacles(FAR_GAUSSIAN)
    else:
        ctx.set_obstacles(None)
    ctx.set_vertices(root, rib)
    ctx.set_samples(sx, sy, sh)
    return ctx


def _oracle(cfg, model, tsp_limit=8):
    import oracle as orc
    world = orc.World(cfg, None, 0.5, gauss=FAR_GAUSSIAN) if model == "gaussian" else orc.World(cfg, None, 0.5, None)
    orc.O.ppo_world_set_tsp_limit(world.h, tsp_limit)
    return world


@pytest.mark.parametrize("case", ROUTE_CASES, ids=_case_id)
def test_every_route_boundary_against_the_oracle(torch_cuda, monkeypatch, case):
    """One dense launch per case and setting.  Lane finish and lane heuristic on, both off: the same record and child bytes; without
    the prepasses (the small-launch path: other windows) rounding noise at most.  The records are the oracle's, every edge compared."""
    from test_gpu_parity import _dense, _same_up_to_run_rounding
    from path_planner_amd.types import F_THROWS
    from parity import compare_results
    heur, k, n, ns, mask, stride, model, near = case
    stride = stride or n + 2
    cfg, rib, root, sx, sy, sh = route_world(heur, k, n, ns, near)
    outs = []
    for lanes, threshold in (("1", "0"), ("0", "0"), ("1", "1000000000")):
        monkeypatch.setenv("PPGPU_LANE_FINISH", lanes)
        monkeypatch.setenv("PPGPU_LANE_HEURISTIC", lanes)
        monkeypatch.setenv("PPGPU_PREPASS_MIN_EDGES", threshold)
        outs.append(_dense(torch_cuda, _context(cfg, rib, root, sx, sy, sh, model), 1, ns, mask, stride=stride))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    _same_up_to_run_rounding(outs[0], outs[2])
    gpu, gchild = outs[0]
    edges = dense_edges(ns, mask)
    cpu, cchild = _oracle(cfg, model).cost_edges(root, rib, sx, sy, sh, edges, stride=stride)
    rep = compare_results(gpu, cpu, gchild, cchild)
    assert rep["ok"], rep
    assert rep["n_feasible"] == len(edges) and rep["n_word_ties"] == 0, rep       # no edge dropped from the comparison
    live = (gpu["flags"] & F_THROWS) == 0
    nr = (gpu["info"] >> 8) & 255
    m = min(n, stride)
    kept = live & (nr == n) & np.all(gchild[:, :m].reshape(len(edges), -1) == rib[:m].reshape(-1), axis=1)
    print(_case_id(case), "child ribbon counts", np.bincount(nr[live]), "kept", int(kept.sum()), "changed", int((live & ~kept).sum()))
    assert np.count_nonzero(live & (nr == n)) >= 1, "no live edge with a child list of %d ribbons" % n
    if heur in (H_DUBINS_ALL, H_DUBINS_K) and n > 8:         # beyond the Dubins enumeration: the flag and h = 0, on every live edge
        from path_planner_amd.types import F_RIBBON_OVF
        assert np.all(gpu["flags"][live] & F_RIBBON_OVF) and np.all(gpu["h"][live] == 0.0) and np.array_equal(gpu["f"][live], gpu["g"][live])
    if n in (7, 8):
        assert kept.any() and (live & ~kept).any(), "the case needs an edge that kept its vertex's list and one that changed it"


@pytest.mark.parametrize("heur,k,n,mask", [(H_ALL, 0, 9, 0x1), (H_K, 2, 13, 0x3)])
def test_table_pass_takes_what_the_rule_flags(torch_cuda, heur, k, n, mask):
    """What the rule sends to overflow is what the table pass takes: with ppgpu_set_tsp_table(0, 16) the flagged records get the value of
    the reference's unbounded recursion, with the switch off they keep the flag and h = 0.  Out of reach of every ribbon; one edge for
    All with 9 ribbons (9 s of the oracle's recursion), two for K = 2 with 13 (2.6 s each)."""
    from test_gpu_parity import _dense
    from path_planner_amd.types import F_RIBBON_OVF
    from parity import compare_results
    ns = 1
    cfg, rib, root, sx, sy, sh = route_world(heur, k, n, ns, near=False, jitter=True)
    ctx = _context(cfg, rib, root, sx, sy, sh, "binary")
    off, off_child = _dense(torch_cuda, ctx, 1, ns, mask, stride=n + 2)
    assert np.all(((off["info"] >> 8) & 255) == n)
    assert np.all(off["flags"] & F_RIBBON_OVF) and np.all(off["h"] == 0.0) and np.array_equal(off["f"], off["g"])
    ctx.set_tsp_table(0, 16)
    on, on_child = _dense(torch_cuda, ctx, 1, ns, mask, stride=n + 2)
    assert ctx.tsp_table_stats() == (len(on), 0)
    cpu, cchild = _oracle(cfg, "binary", tsp_limit=0).cost_edges(root, rib, sx, sy, sh, dense_edges(ns, mask), stride=n + 2)
    rep = compare_results(on, cpu, on_child, cchild)
    assert rep["ok"] and rep["n_feasible"] == len(on), rep
    assert not np.any(on["flags"] & F_RIBBON_OVF) and np.all(on["h"] > 0)


def test_trace_resolve_leaves_the_launch_counters(torch_cuda, monkeypatch):
    """ppgpu_last_cover_edges reads the launch's counters.  A trace of a sliced launch solves the edges again, slice by slice, and must
    not reset them: the count after cost_edges_host, after a sliced trace of the same list, and on an unsliced handle are one number
    (with timing on, as ppgpu.h says of sliced launches)."""
    from path_planner_amd import workloads
    from test_gpu_parity import _setup
    w = workloads.config3(n_samples=75)
    counts = []
    for budget in ("200000", None):                        # ~3.6 KB of workspace per edge: some fifty edges per slice, or one slice
        if budget:
            monkeypatch.setenv("PPGPU_SLICE_BYTES", budget)
        else:
            monkeypatch.delenv("PPGPU_SLICE_BYTES")
        ctx, world, n, cs = _setup(w, 75)
        ctx.enable_timing(True)
        edges = dense_edges(n, 0xF)
        ctx.cost_edges_host(edges, stride=8)
        counts.append(ctx.last_cover_edges())
        if budget:
            ctx.trace_edges(edges, 64)
            counts.append(ctx.last_cover_edges())
    print("edges", len(edges), "cover edges", counts)
    assert counts[0] == counts[1] == counts[2] and 0 < counts[0] <= len(edges), counts
